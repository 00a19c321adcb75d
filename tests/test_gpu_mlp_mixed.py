"""The fused deformation MLP on inputs that mix magnitudes inside one scale group of the split-f16 path
(tests/mlp_mixed.py), both arithmetics against the float64 oracle, every error taken PER CLASS of points so a
degraded near point cannot hide under a far one. Oracle gradients use each kernel's own relu' masks
(helpers.mlp_relu_masks); the forward is checked with saved activations and under torch.no_grad().

Bars (the project's, test_gpu_mlp.py): per point |err| <= 2e-5 + 1e-4 |ref|; per class the split path's max
error <= 2x the exact-fp32 path's on the same class + 1e-6; parameter gradients within 1e-4 of the tensor's
max and within 2x the exact path's error (the rescaled-weights rule, per weight row, adds 1e-6 of the
row's max).
They are asserted on the sets tests/test_mlp_mixed_ref.py derives from the numpy model of the split GEMM under
the flush assumption (tests/golden/mlp_mixed_sets.npz: F <= 1e3, K <= 4); rungs above are run, checked to be
finite and recorded (helpers.write_stats) beside the model's two predictions.
"""
import os

import numpy as np
import pytest
import torch

import mlp_mixed as mm
from helpers import _S_H, mlp_relu_masks, write_stats
from oracle import mlp_ref
from weights import mlp_weights

pytestmark = pytest.mark.gpu

ARITH = {"split": False, "exact": True}
T0 = 0.37
_SETS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", mm.SETS_FILE))
F_SET = tuple(float(f) for f in _SETS["F_asserted"])
K_MAX = int(_SETS["K_max"])
W = mlp_weights(mlp_ref.param_shapes(True, False), 77)
HEADS = ("d_xyz", "d_rot", "d_scale")


def _net(w, exact):
    from deformgs.deform_network import DeformNetworkBaseline
    net = DeformNetworkBaseline(is_blender=True, exact_fp32=exact).cuda()
    net.load_state_dict({k: torch.from_numpy(a) for k, a in w.items()})
    return net


def _times(t, tmode):
    """(numpy (N, 1) times, the tensor the network gets): "expanded" is the stride-0 frame time of training
    (the folded kernels), "random" per-point times (per-point timenet)."""
    N = t.shape[0]
    if tmode == "expanded":
        return np.full((N, 1), T0, np.float32), torch.full((1, 1), T0, device="cuda").expand(N, -1)
    return t, torch.from_numpy(t).cuda()


def _ref_raw(out):
    return np.concatenate([out[k] for k in HEADS], 1)


def _forward_both(net, x, tt):
    """raw outputs with saved activations (autograd on) and under no_grad, as numpy, plus the live tensor."""
    xt = torch.from_numpy(x).cuda()
    raw = net.raw(xt, tt)
    with torch.no_grad():
        ng = net.raw(xt, tt)
    return raw, raw.detach().cpu().numpy(), ng.cpu().numpy()


def _param_grads(net, w, raw, G, c, out, exact, tmode):
    """{name: (|got - ref| array, ref)} for the upstream gradient G on the raw outputs."""
    masks = mlp_relu_masks(raw, G.shape[0], True, exact, th_saved=exact or tmode == "random")
    (raw * torch.from_numpy(G).float().cuda()).sum().backward()
    g = {"d_xyz": G[:, 0:3], "d_rot": G[:, 3:7], "d_scale": G[:, 7:10]}
    ref = mlp_ref.backward(w, c, out, g, True, False, relu_masks=masks)
    return {k: (np.abs(p.grad.cpu().numpy() - ref[k]), ref[k]) for k, p in net.named_parameters()}


def _no_expiry():
    from deformgs import _lib
    assert _lib.load().dgs_debug_guard_expiries() == 0


def _bar(ref):
    return 2e-5 + 1e-4 * np.abs(ref)


def _model_row(name, i):
    return {c: dict(zip(("flush", "keep", "fp32"), map(float, _SETS[f"{name}_{c}"][i]))) for c in mm.CLASSES[:3]}


# ------------------------------------------------------------------------------------------------
# far points
# ------------------------------------------------------------------------------------------------
def _far_case(r, tmode, with_grads):
    """One scene on both arithmetics -> (per-arith dict(out / ng class errors, bar misses, near_free equality,
    finite, grads), ...). The float64 forward is shared by the two arithmetics; for the tail placement it
    covers the classified rows only (the forward is per point)."""
    ev, cls, N = r["eval"], r["cls"], r["x"].shape[0]
    t_np, tt = _times(r["t"], tmode)
    out, c = mlp_ref.forward(W, r["x"][ev], t_np[ev], True, False)
    ref = _ref_raw(out)
    free = cls == mm.NEAR_FREE
    res = {}
    for arith, exact in ARITH.items():
        net = _net(W, exact)
        raw, o, ng = _forward_both(net, r["x"], tt)
        _, oc, ngc = _forward_both(net, r["x_clean"], tt)
        e = dict(finite=bool(np.isfinite(o).all() and np.isfinite(ng).all()),
                 free_equal=bool((o[free] == oc[free]).all() and (ng[free] == ngc[free]).all()), n_free=int(free.sum()))
        for name, v in (("out", o), ("ng", ng)):
            err = np.abs(v[ev] - ref)
            e[name] = mm.class_max(err, cls[ev])
            e[name + "_miss"] = mm.class_max((err > _bar(ref)).astype(float), cls[ev])
        if with_grads:
            G = np.random.default_rng(7).standard_normal((N, 10))
            gr = _param_grads(net, W, raw, G, c, out, exact, tmode)
            e["grad"] = {k: float(d.max()) for k, (d, _) in gr.items()}
            e["grad_max"] = {k: float(np.abs(g).max()) for k, (_, g) in gr.items()}
        res[arith] = e
    return res


def _record_far(head, res, model):
    """One line per scene: per class the saved-forward errors of both arithmetics (`ng_same`: the no_grad
    forward gave the same class maxima), the parameter-gradient errors and the reference maxima once; the
    layer-0 model's predictions (flush / keep / fp32) once per rung, beside the case it models."""
    rec = dict(head, asserted=head["F"] in F_SET)
    for arith in ARITH:
        e = res[arith]
        rec[arith] = dict(out=e["out"], ng_same=e["ng"] == e["out"], free_equal=e["free_equal"], finite=e["finite"])
    if "grad" in res["split"]:  # parameter gradients: the worst split / exact ratio and the worst errors of the tensor's max
        gs, ge, gm = res["split"]["grad"], res["exact"]["grad"], res["split"]["grad_max"]
        k = max(gs, key=lambda n: gs[n] / max(ge[n], 1e-300))
        rec["grad"] = dict(worst_ratio=gs[k] / max(ge[k], 1e-300), tensor=k, split_rel=max(gs[n] / gm[n] for n in gs),
                           exact_rel=max(ge[n] / gm[n] for n in gs))
    if model is not None:
        rec["model_layer0"] = model
    write_stats("mlp_mixed_far", rec)


def _check_far(res, tag):
    for arith in ARITH:
        e = res[arith]
        assert e["finite"], (tag, arith)
        assert e["free_equal"], (tag, arith, "near_free rows differ from the run without far points")
        for name in ("out", "ng"):
            assert all(v == 0.0 for v in e[name + "_miss"].values()), (tag, arith, name, e[name + "_miss"], e[name])
    for name in ("out", "ng"):
        for cl, es in res["split"][name].items():
            assert es <= 2.0 * res["exact"][name][cl] + 1e-6, (tag, name, cl, es, res["exact"][name][cl])
    if "grad" in res["split"]:
        for k, es in res["split"]["grad"].items():
            gmax = max(res["split"]["grad_max"][k], 1e-30)
            for arith in ARITH:
                assert res[arith]["grad"][k] <= 1e-4 * gmax, (tag, arith, k, res[arith]["grad"][k], gmax)
            assert es <= 2.0 * res["exact"]["grad"][k], (tag, k, es, res["exact"]["grad"][k], gmax)


@pytest.mark.parametrize("tmode", ["expanded", "random"])
@pytest.mark.parametrize("placement", ["every", "quarter"])
def test_far_points(placement, tmode):
    """A far point in every tile / in one tile of four, N = 200, the whole ladder. Asserted rungs: every class
    meets the per-point bar and the 2x rule, near_free rows are bitwise the rows of the run without far
    points (per-tile scales), parameter gradients from an N(0, 1) upstream gradient meet theirs.
    Rungs above: finite, recorded."""
    for i, F in enumerate(mm.LADDER):
        res = _far_case(mm.far_recipe(placement, F), tmode, True)
        _record_far(dict(placement=placement, tmode=tmode, F=F), res,
                    _model_row("far_err", i) if (placement, tmode) == ("every", "random") else None)
        if F in F_SET:
            _check_far(res, (placement, tmode, F))
        else:
            assert res["split"]["finite"] and res["exact"]["finite"], (placement, tmode, F)
    _no_expiry()


@pytest.mark.parametrize("tmode", ["expanded", "random"])
def test_far_point_in_tail_block(tmode):
    """N = 64 CUs + 40: the last round is one block, run as 16-point tail blocks (block_split), the far point
    in the second of them. Forward only; the last 104 points (one 64-point block and the tail) are
    classified, the filler rows in front count as near_free for the bitwise check."""
    from deformgs import _lib
    ncu = torch.cuda.get_device_properties(0).multi_processor_count - _lib.load().dgs_mlp_reserved_cus()
    for F in mm.LADDER:
        res = _far_case(mm.far_recipe("tail", F, ncu=ncu), tmode, False)
        _record_far(dict(placement="tail", tmode=tmode, F=F, ncu=ncu), res, None)
        if F in F_SET:
            _check_far(res, ("tail", tmode, F))
        else:
            assert res["split"]["finite"] and res["exact"]["finite"], (tmode, F)
    assert _lib.load().dgs_debug_guard_expiries() == 0


# ------------------------------------------------------------------------------------------------
# rescaled weights
# ------------------------------------------------------------------------------------------------
def _row_norm(d, ref, rowf):
    """max over rows of (max |err| / max |ref|) per row: weights by row; a bias in the base network's units
    (element i times c_i = divided by its gradient factor), normalised by the tensor's max."""
    if d.ndim == 1:
        return float((d / rowf).max() / max(np.abs(ref / rowf).max(), 1e-30))
    rmax = np.abs(ref).max(1)
    live = rmax > 0
    assert (d[~live] == 0).all()  # a dead unit's row: exactly zero on both sides
    return float((d[live].max(1) / rmax[live]).max())


_RESCALE = {}


def _rescale_case(K, tmode):
    """One (K, time mode) on both arithmetics, computed once for the forward and the gradient test."""
    if (K, tmode) in _RESCALE:
        return _RESCALE[(K, tmode)]
    rng = np.random.default_rng(23)
    N = 200
    x = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
    t_np, tt = _times(rng.uniform(0, 1, (N, 1)).astype(np.float32), tmode)
    G = rng.standard_normal((N, 10))
    w2, c = mm.rescale_weights(W, K)
    out, cache = mlp_ref.forward(w2, x, t_np, True, False)
    ref = _ref_raw(out)
    f = mm.grad_factors(W, c)
    res = {}
    for arith, exact in ARITH.items():
        base = _forward_both(_net(W, exact), x, tt)[1]
        net = _net(w2, exact)
        raw, o, ng = _forward_both(net, x, tt)
        gr = _param_grads(net, w2, raw, G, cache, out, exact, tmode)
        res[arith] = dict(out=float(np.abs(o - ref).max()), ng=float(np.abs(ng - ref).max()),
                          miss=int((np.abs(o - ref) > _bar(ref)).sum() + (np.abs(ng - ref) > _bar(ref)).sum()),
                          equals_base=bool((o == base).all()), finite=bool(np.isfinite(o).all() and np.isfinite(ng).all()),
                          grad={k: _row_norm(d, g, f[k]) for k, (d, g) in gr.items()})
    rec = dict(tmode=tmode, K=K, asserted=K <= K_MAX, **res)
    if tmode == "random":  # the case the layer-0 model is of
        rec["model_layer0"] = dict(zip(("flush", "keep", "fp32"), map(float, _SETS["k_err"][mm.K_LADDER.index(K)])))
    write_stats("mlp_mixed_rescale", rec)
    _no_expiry()
    _RESCALE[(K, tmode)] = res
    return res


@pytest.mark.parametrize("tmode", ["expanded", "random"])
@pytest.mark.parametrize("K", mm.K_LADDER)
def test_rescaled_weights_forward(K, tmode):
    """Rows of every trunk layer times 2^k, k in [-K, K], undone in the consumers' columns (rescale_weights):
    the same function with n-tiles and activation tiles spanning 2^2K. K <= K_MAX: the exact path's outputs are
    bitwise the base network's, and the split path meets the per-point bar and the 2x rule. K above: finite,
    recorded."""
    res = _rescale_case(K, tmode)
    assert res["split"]["finite"] and res["exact"]["finite"], K
    if K > K_MAX:
        return
    assert res["exact"]["equals_base"], (K, "exact path: power-of-two row scales must be bitwise neutral")
    for arith in ARITH:
        assert res[arith]["miss"] == 0, (K, arith, res[arith])
    for name in ("out", "ng"):
        assert res["split"][name] <= 2.0 * res["exact"][name] + 1e-6, (K, name, res["split"][name], res["exact"][name])


K4_MISS = ("timenet.0.weight", "timenet.2.weight", "linear.2.weight")


def _grad_rule(res, K, k):
    es, ee = res["split"]["grad"][k], res["exact"]["grad"][k]
    assert es <= 2.0 * ee + 1e-6, (K, k, es, ee)


@pytest.mark.parametrize("tmode", ["expanded", "random"])
@pytest.mark.parametrize("K", [K for K in mm.K_LADDER if K <= K_MAX])
def test_rescaled_weights_gradients(K, tmode):
    """K <= K_MAX: every parameter gradient, normalised PER WEIGHT ROW by that row's reference max (a small row
    must not hide under a large one; a bias in the base network's units), is within 2x the exact path's +
    1e-6 of the row's max. Measured on MI355X: K = 1, 2 worst split / exact ratio 1.49; K = 4 meets the rule
    with per-point times, and with the frame-uniform t on every tensor but the three of K4_MISS, which
    test_rescaled_weights_gradients_k4_uniform_t holds one by one."""
    res = _rescale_case(K, tmode)
    for k in res["split"]["grad"]:
        if not ((K, tmode) == (4, "expanded") and k in K4_MISS):
            _grad_rule(res, K, k)


@pytest.mark.xfail(strict=True, reason=(
    "K = 4, frame-uniform t, split / exact gradient error per row on MI355X: timenet.0.weight 2.87e-5 vs 1.10e-5 "
    "(2.6x), timenet.2.weight 1.69e-5 vs 6.34e-6 (2.67x), linear.2.weight 6.40e-6 vs 2.45e-6 (2.6x): the dX chain's "
    "bound max_col sum |W| x max |dZ| grows with the rescale's 2^2K while the dZ rows it covers span 2^2K "
    "(DESIGN.md, accuracy)"))
@pytest.mark.parametrize("tensor", K4_MISS)
def test_rescaled_weights_gradients_k4_uniform_t(tensor):
    _grad_rule(_rescale_case(4, "expanded"), 4, tensor)


def _saved_h(output, N, exact, L):
    """Layer L's saved activations (N, 256) of the fused node reached from `output` (helpers.mlp_relu_masks
    reads the same rows for its masks)."""
    seen, todo, node = set(), [output.grad_fn], None
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "FusedDeformMLP" in type(fn).__name__:
            node = fn
            break
        todo.extend(f for f, _ in fn.next_functions)
    assert node is not None
    _, saved = node.saved_tensors
    block = 32 if exact else 64
    Ns = (N + block - 1) // block * block
    return saved[: 2416 * Ns].view(2416, Ns)[_S_H[L]:_S_H[L] + 256, :N].T.cpu().numpy()


@pytest.mark.parametrize("tmode", ["expanded", "random"])
def test_tilewise_rescaled_layer(tmode):
    """linear.0's rows times 2^(k_t + k_i), k_t one offset per 16-row n-tile over [-10, 10], k_i in {-1, 0, 1}
    (rescale_tilewise; linear.1's columns undo it): every n-tile is narrow while the image spans 2^22, so
    one weight scale per n-tile keeps every row at full precision and one per image would not. Layer 0's own
    saved activations, normalised per row by the row's reference max: split <= 2x exact (the consumer's
    activation tile spans the 2^22 on the B side, so the outputs past it are only checked to be finite and
    recorded). The exact path's outputs are bitwise the base network's."""
    rng = np.random.default_rng(53)
    N = 200
    x = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
    t_np, tt = _times(rng.uniform(0, 1, (N, 1)).astype(np.float32), tmode)
    w2, _ = mm.rescale_tilewise(W)
    out, cache = mlp_ref.forward(w2, x, t_np, True, False)
    h0 = np.maximum(cache["z"][0], 0.0)
    e, outs = {}, {}
    for arith, exact in ARITH.items():
        raw, o, _ = _forward_both(_net(w2, exact), x, tt)
        got = _saved_h(raw, N, exact, 0).astype(np.float64)
        flip = (got > 0) != (h0 > 0)  # a pre-activation within rounding of 0: either side of the ReLU
        e[arith] = mm.row_norm_max(np.where(flip, 0.0, got - h0), h0)
        outs[arith] = dict(h0=e[arith], flips=int(flip.sum()), out=float(np.abs(o - _ref_raw(out)).max()),
                           finite=bool(np.isfinite(o).all()))
        if exact:
            assert (o == _forward_both(_net(W, True), x, tt)[1]).all()
    write_stats("mlp_mixed_tilewise", dict(tmode=tmode, KT=mm.KT, **outs))
    assert outs["split"]["finite"] and outs["exact"]["finite"]
    assert max(outs[a]["flips"] for a in ARITH) <= 2
    assert e["split"] <= 2.0 * e["exact"], e
    _no_expiry()


# ------------------------------------------------------------------------------------------------
# wide-range upstream gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tmode", ["expanded", "random"])
def test_wide_range_upstream_gradient(tmode):
    """dOut as a training step hands it over: 70 % of the rows exactly zero, the others N(0, 1) times a
    row magnitude log-uniform over [1e-10, 1e-3] (seven decades inside one dOut / dZ column tile). Every
    parameter gradient's error, normalised by the tensor's max: split <= 2x exact."""
    rng = np.random.default_rng(31)
    N = 333
    x = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
    t_np, tt = _times(rng.uniform(0, 1, (N, 1)).astype(np.float32), tmode)
    G = rng.standard_normal((N, 10)) * 10.0 ** rng.uniform(-10, -3, (N, 1))
    G[rng.permutation(N)[: int(0.7 * N)]] = 0.0
    out, c = mlp_ref.forward(W, x, t_np, True, False)
    e = {}
    for arith, exact in ARITH.items():
        net = _net(W, exact)
        raw = net.raw(torch.from_numpy(x).cuda(), tt)
        gr = _param_grads(net, W, raw, G, c, out, exact, tmode)
        e[arith] = {k: float(d.max() / np.abs(g).max()) for k, (d, g) in gr.items()}
    write_stats("mlp_mixed_wide_dout", dict(tmode=tmode, **e))
    for k in e["split"]:
        assert e["split"][k] <= 2.0 * e["exact"][k], (k, e["split"][k], e["exact"][k])
    _no_expiry()


def test_wide_range_upstream_gradient_active_set():
    """The same kind of dOut through the active-row path (csrc/mlp_active.h: dgs_deform_backward_active after
    the no-save forward; test_gpu_mlp_active.py's harness over the C ABI): the 30 % nonzero rows are compacted,
    so OTHER rows share each dOut / dZ column-tile scale than in the full backward, and the activations are
    recomputed on them. The path exists for the split arithmetic with a frame-uniform t only
    (dgs_deform_active_supported). Against float64 with the relu' masks of the saving forward, normalised by
    the tensor's max: active <= 2x the exact-fp32 path's error on the same dOut + 2^-23 (one fp32 ulp of the
    tensor's largest element). The floor is the output format's: a gradient is stored in fp32, so it carries
    up to half an ulp whatever computed it, and two fp32 summation orders of the same ~100 terms differ by
    about one; below that a ratio of two errors compares rounding luck. It matters for the heads' 3- and
    4-element biases only (measured, of the tensor's max: gaussian_scaling.bias active 1.26e-7, full backward
    5.7e-8, exact 3.2e-8; gaussian_warp.bias 3.8e-8 / 8.3e-8 / 1.7e-8); the other 23 tensors are at 0.47 .. 1.81
    of the exact path's error without it. test_wide_range_upstream_gradient carries no floor."""
    from test_gpu_mlp_active import T0 as TA, _Net
    N = 333
    net = _Net("blender", N)
    rng = np.random.default_rng(37)
    G = rng.standard_normal((N, 10)) * 10.0 ** rng.uniform(-10, -3, (N, 1))
    G[rng.permutation(N)[: int(0.7 * N)]] = 0.0
    Gt = torch.from_numpy(G).float().cuda()
    G = Gt.double().cpu().numpy()  # the fp32 values the kernels get
    t_np = np.full((N, 1), TA, np.float32)
    out, c = mlp_ref.forward(net.w, net.x_np, t_np, True, False)
    g = {"d_xyz": G[:, 0:3], "d_rot": G[:, 3:7], "d_scale": G[:, 7:10]}
    _, g_full, masks = net.full(Gt)
    _, g_act, m = net.act(Gt)
    assert m == int((G != 0).any(1).sum()) == N - int(0.7 * N)
    ref = mlp_ref.backward(net.w, c, out, g, True, False, relu_masks=masks)
    exact = _net(net.w, True)
    raw = exact.raw(net.x, torch.full((1, 1), TA, device="cuda").expand(N, -1))
    ge = _param_grads(exact, net.w, raw, G, c, out, True, "expanded")
    e = {"active": {}, "full": {}, "exact": {}}
    for name, got, gf in zip(net.names, g_act, g_full):
        gmax = np.abs(ref[name]).max()
        e["active"][name] = float(np.abs(got.cpu().numpy() - ref[name]).max() / gmax)
        e["full"][name] = float(np.abs(gf.cpu().numpy() - ref[name]).max() / gmax)
        e["exact"][name] = float(ge[name][0].max() / np.abs(ge[name][1]).max())
    write_stats("mlp_mixed_wide_dout_active", dict(N=N, M=m, **e))
    for k in e["active"]:
        assert e["active"][k] <= 2.0 * e["exact"][k] + 2.0 ** -23, (k, e["active"][k], e["exact"][k])


# ------------------------------------------------------------------------------------------------
# non-finite rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tmode", ["expanded", "random"])
@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 3e38])
def test_non_finite_row(bad, arith, tmode):
    """One point of a tile has xyz = NaN, +Inf or 3e38 (finite, but 2 * 3e38 overflows its encodings and
    its bound is past scale_for's clamp). Rows outside that tile: bitwise the clean run's. Inside the tile
    every output of a finite-input row is within the per-point bar or non-finite: a finite value outside
    the bar fails. (The split path poisons the tile: NaN for its 16 points; the fp32 path keeps
    the neighbours and the bad row comes out NaN.)"""
    rng = np.random.default_rng(41)
    N, p = 200, 37
    x = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
    t_np, tt = _times(rng.uniform(0, 1, (N, 1)).astype(np.float32), tmode)
    xb = x.copy()
    xb[p] = bad
    _, _, tile, _ = mm.tile_map(N)
    inside = tile == tile[p]
    with np.errstate(all="ignore"):
        ref = _ref_raw(mlp_ref.forward(W, xb, t_np, True, False)[0])
    net = _net(W, ARITH[arith])
    _, oc, ngc = _forward_both(net, x, tt)
    _, ob, ngb = _forward_both(net, xb, tt)
    for v, vc in ((ob, oc), (ngb, ngc)):
        assert (v[~inside] == vc[~inside]).all() and np.isfinite(v[~inside]).all()
        rows = inside & np.isfinite(xb).all(1)
        fin = np.isfinite(v[rows])
        with np.errstate(invalid="ignore"):
            off = fin & ~(np.abs(v[rows] - ref[rows]) <= _bar(ref[rows]))
        assert not off.any(), (arith, bad, "finite outputs outside the bar", int(off.sum()), v[rows][off][:4])
    _no_expiry()
