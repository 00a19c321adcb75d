"""CPU checks of tests/mlp_mixed.py (no GPU): the tile map against the kernels' block loop written out, the
input recipes' class structure, the function-preserving weight rescale against the float64 oracle, and the
numpy model of the split layer-0 GEMM against a plain fp32 layer 0, both against float64 per class.

The model yields the ASSERTED SETS of tests/test_gpu_mlp_mixed.py (tests/golden/mlp_mixed_sets.npz): the
rungs F of the far-point ladder, and the largest rescale exponent K, for which the coupled classes' layer-0
error stays within 2x the fp32 layer-0 error on the same class when f16 subnormal operands are flushed (the
pessimistic assumption). The file is written when it is missing and compared otherwise, so the sets the GPU
test asserts are the ones this model gives, never fitted to the kernels.
"""
import os

import numpy as np
import pytest

import mlp_mixed as mm
from oracle import mlp_ref
from weights import mlp_weights

W = mlp_weights(mlp_ref.param_shapes(True, False), 77)


@pytest.mark.parametrize("N,ncu", [(1, 0), (200, 0), (512, 256), (64 * 8 + 40, 8), (64 * 8 + 1, 8), (64 * 16 + 200, 16),
                                   (64 * 9, 8), (64 * 256 + 40, 256), (64 * 12 + 5, 4)])
def test_tile_map_matches_block_loop(N, ncu):
    """fwd_kernel's loop: blocks b < nfull start at 64 b and hold slots m < 64 (column tile qof(m) = m >> 4),
    the others start at 64 nfull + 16 (b - nfull) and hold one column tile."""
    nfull, ntail = mm.split_blocks(N, ncu)
    block, q, tile, tail = mm.tile_map(N, ncu)
    seen = np.zeros(N, int)
    groups = {}
    for b in range(nfull + ntail):
        p0, npt = (b * 64, 64) if b < nfull else (nfull * 64 + (b - nfull) * 16, 16)
        for m in range(npt):
            p = p0 + m
            if p < N:
                seen[p] += 1
                assert (block[p], q[p], tail[p]) == (b, m >> 4 if b < nfull else 0, b >= nfull)
                groups.setdefault((b, m >> 4), []).append(p)
    assert (seen == 1).all()
    for pts in groups.values():  # the points of one (block, column tile) share one id, and nobody else has it
        assert len(set(tile[pts])) == 1 and (tile == tile[pts[0]]).sum() == len(pts)
    assert (tile == np.arange(N) // 16).all()
    if (N, ncu) in ((64 * 8 + 40, 8), (64 * 256 + 40, 256)):
        assert (nfull, ntail) == (ncu, 4)
    if ncu == 0 or N <= 64 * ncu:
        assert ntail == 0


@pytest.mark.parametrize("placement", ["every", "quarter", "tail"])
def test_recipes(placement):
    r1 = mm.far_recipe(placement, 1e1, ncu=8)
    r6 = mm.far_recipe(placement, 1e6, ncu=8)
    cls, x = r6["cls"], r6["x"]
    N = x.shape[0]
    assert N <= 512 + 40 and (r1["cls"] == cls).all() and (r1["x_clean"] == r6["x_clean"]).all()
    assert (r1["x"][cls != mm.FAR] == x[cls != mm.FAR]).all()
    _, _, tile, tail = mm.tile_map(N, 8)
    far_tiles = set(tile[cls == mm.FAR])
    for p in range(N):
        assert (tile[p] in far_tiles) == (cls[p] != mm.NEAR_FREE)
    for tl in far_tiles:
        assert (cls[tile == tl] == mm.FAR).sum() == 1
    ax = np.abs(x)
    assert (ax[cls == mm.FAR] >= 0.7e6).all() and (ax[cls == mm.FAR] <= 1e6).all()
    assert (ax[cls == mm.TINY_COUPLED] >= 1e-4 * 0.999).all() and (ax[cls == mm.TINY_COUPLED] <= 1e-2).all()
    assert (ax[(cls == mm.NEAR_COUPLED) | (cls == mm.NEAR_FREE)] <= 1.3).all()
    assert (np.abs(r6["x_clean"][cls != mm.TINY_COUPLED]) <= 1.3).all()
    present = {c for c in range(4) if (cls[r6["eval"]] == c).any()}
    assert present == ({0, 1, 2} if placement == "every" else {0, 1, 2, 3})
    if placement == "tail":
        assert tail[cls == mm.FAR].all() and (cls == mm.FAR).sum() == 1
        assert (cls[: N - 104] == mm.NEAR_FREE).all()


@pytest.mark.parametrize("K", [1, 4, 12])
def test_rescale_preserves_function_and_scales_gradients(K):
    rng = np.random.default_rng(3)
    N = 96
    x = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
    t = rng.uniform(0, 1, (N, 1)).astype(np.float32)
    w2, c = mm.rescale_weights(W, K)
    spans = [np.log2(c[L].reshape(16, 16).max(1) / c[L].reshape(16, 16).min(1)).max() for L in range(8)]
    assert max(spans) == 2 * K or K == 12, spans  # some n-tile spans the whole 2^2K (16 draws of 2K + 1 values)
    out, ca = mlp_ref.forward(W, x, t, True, False)
    out2, cb = mlp_ref.forward(w2, x, t, True, False)
    for k in ("d_xyz", "d_rot", "d_scale"):
        assert np.abs(out2[k] - out[k]).max() <= 1e-12 * np.abs(out[k]).max(), k
    for L in range(8):
        assert ((cb["z"][L] > 0) == (ca["z"][L] > 0)).all()
    g = {k: rng.standard_normal(out[k].shape) for k in ("d_xyz", "d_rot", "d_scale")}
    ga = mlp_ref.backward(W, ca, out, g, True, False)
    gb = mlp_ref.backward(w2, cb, out2, g, True, False)
    f = mm.grad_factors(W, c)
    for k in ga:
        back = gb[k] / f[k]  # in the base network's units
        assert np.abs(back - ga[k]).max() <= 1e-12 * np.abs(ga[k]).max(), k


def _far_errors(F, placement="every"):
    r = mm.far_recipe(placement, F)
    ref = mm.layer0_ref(W, r["x"], r["t"])
    e = {}
    for name, z in (("flush", mm.layer0_split_model(W, r["x"], r["t"], True)),
                    ("keep", mm.layer0_split_model(W, r["x"], r["t"], False)),
                    ("fp32", mm.layer0_fp32(W, r["x"], r["t"]))):
        e[name] = mm.class_max(np.abs(z - ref), r["cls"])
    return e


def _k_errors(K):
    """Layer-0 errors of the rescaled network in the base network's units (row i divided by c_i), max over
    near points: a small row must not hide under a large one."""
    rng = np.random.default_rng(17)
    x = rng.uniform(-1.3, 1.3, (128, 3)).astype(np.float32)
    t = rng.uniform(0, 1, (128, 1)).astype(np.float32)
    w2, c = mm.rescale_weights(W, K)
    ref = mm.layer0_ref(w2, x, t)
    return {name: float((np.abs(z - ref) / c[0][None, :]).max())
            for name, z in (("flush", mm.layer0_split_model(w2, x, t, True)),
                            ("keep", mm.layer0_split_model(w2, x, t, False)), ("fp32", mm.layer0_fp32(w2, x, t)))}


def _sets():
    coupled = ("near_coupled", "tiny_coupled")
    fe = [_far_errors(F) for F in mm.LADDER]
    ke = [_k_errors(K) for K in mm.K_LADDER]
    ok_f = [all(e["flush"][c] <= 2.0 * e["fp32"][c] for c in coupled) for e in fe]
    ok_k = [e["flush"] <= 2.0 * e["fp32"] for e in ke]
    rungs = mm.asserted_prefix(mm.LADDER, ok_f)
    ks = mm.asserted_prefix(mm.K_LADDER, ok_k)
    rec = dict(F_asserted=np.array(rungs, np.float64), K_max=np.array(ks[-1] if ks else 0),
               ladder=np.array(mm.LADDER), k_ladder=np.array(mm.K_LADDER),
               k_err=np.array([[e["flush"], e["keep"], e["fp32"]] for e in ke]))
    for c in mm.CLASSES[:3]:
        rec["far_err_" + c] = np.array([[e["flush"][c], e["keep"][c], e["fp32"][c]] for e in fe])
    return rec


def test_model_sets_match_golden(golden_dir):
    rec = _sets()
    path = os.path.join(golden_dir, mm.SETS_FILE)
    if not os.path.exists(path):
        np.savez(path, **rec)
    gold = np.load(path)
    assert list(gold["F_asserted"]) == list(rec["F_asserted"]) and int(gold["K_max"]) == int(rec["K_max"])
    for k in rec:  # the recorded errors (columns: flush, keep, fp32) reproduce
        assert np.allclose(gold[k], rec[k], rtol=1e-6, atol=0), k
    # the model distinguishes what it should: with subnormals kept it is never worse than with them flushed,
    # and far points leave the fp32 layer's error on the coupled classes alone
    for c in ("near_coupled", "tiny_coupled"):
        e = rec["far_err_" + c]
        assert (e[:, 1] <= e[:, 0] * (1 + 1e-12)).all()
        assert e[:, 2].max() <= 4.0 * e[:, 2].min()


def test_model_control_class_is_untouched_by_far_points():
    """near_free rows of the model: bitwise what the far-free scene gives (per-tile scales)."""
    r = mm.far_recipe("quarter", 1e6)
    free = r["cls"] == mm.NEAR_FREE
    for flush in (True, False):
        a = mm.layer0_split_model(W, r["x"], r["t"], flush)
        b = mm.layer0_split_model(W, r["x_clean"], r["t"], flush)
        assert (a[free] == b[free]).all() and not (a[~free] == b[~free]).all()


def test_model_sees_the_scale_rule_mutants():
    """The model under a wrong scale rule misses the 2x bar where the right rule meets it: x_emb's bound
    floor at 2^20 instead of 1 (near points in far-free tiles), and one weight scale per image instead of
    per n-tile on the tile-wise rescale (rescale_tilewise: each n-tile narrow, the image spanning 2^22),
    whether f16 subnormals are flushed or kept. (rescale_weights draws k_i per row, so nearly every n-tile
    holds a row near 2^K and the tile's scale equals the image's: it cannot separate the two.)"""
    r = mm.far_recipe("quarter", 1e1)
    ref = mm.layer0_ref(W, r["x"], r["t"])
    fp = mm.class_max(np.abs(mm.layer0_fp32(W, r["x"], r["t"]) - ref), r["cls"])["near_free"]
    good = mm.class_max(np.abs(mm.layer0_split_model(W, r["x"], r["t"], True) - ref), r["cls"])["near_free"]
    bad = mm.class_max(np.abs(mm.layer0_split_model(W, r["x"], r["t"], True, xe_floor=2.0 ** 20) - ref),
                       r["cls"])["near_free"]
    assert good <= 2.0 * fp < bad, (good, fp, bad)
    w2, c = mm.rescale_tilewise(W)
    ref = mm.layer0_ref(w2, r["x_clean"], r["t"])
    n = lambda z: float((np.abs(z - ref) / c[0][None, :]).max())  # noqa: E731  (rows in the base network's units)
    fp = n(mm.layer0_fp32(w2, r["x_clean"], r["t"]))
    for flush in (True, False):
        good = n(mm.layer0_split_model(w2, r["x_clean"], r["t"], flush))
        bad = n(mm.layer0_split_model(w2, r["x_clean"], r["t"], flush, w_scale="image"))
        assert good <= 2.0 * fp < bad, (flush, good, fp, bad)


def test_tilewise_rescale_preserves_function():
    rng = np.random.default_rng(4)
    x = rng.uniform(-1.3, 1.3, (64, 3)).astype(np.float32)
    t = rng.uniform(0, 1, (64, 1)).astype(np.float32)
    w2, c = mm.rescale_tilewise(W)
    k = np.log2(c[0]).reshape(16, 16)
    assert (k.max(1) - k.min(1)).max() <= 2 and k.max() - k.min() >= 2 * mm.KT
    out, ca = mlp_ref.forward(W, x, t, True, False)
    out2, cb = mlp_ref.forward(w2, x, t, True, False)
    for h in ("d_xyz", "d_rot", "d_scale"):
        assert np.abs(out2[h] - out[h]).max() <= 1e-12 * np.abs(out[h]).max(), h
    assert np.abs(cb["z"][0] / c[0] - ca["z"][0]).max() <= 1e-12 * np.abs(ca["z"][0]).max()
