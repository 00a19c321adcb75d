"""Mixed magnitudes inside one scale group of the split-f16 deformation MLP: the tile map of the fused
kernels, seeded input recipes that put far, near and tiny points into one 16-point column tile, a
function-preserving rescale of the trunk's weights, and a numpy model of one split GEMM (layer 0).

The split path (csrc/mlp_split_*.h) shares one power-of-two scale among the 16 points of a column tile (every
B operand) and among the 16 rows of an n-tile (every A operand); the fp32 path and the float64 oracle treat
every point and every weight row on its own. tests/test_mlp_mixed_ref.py checks these helpers on the CPU and
derives the asserted sets; tests/test_gpu_mlp_mixed.py runs the kernels on them.
"""
import numpy as np

from oracle import mlp_ref

BM = 64  # points per workgroup block (mlp_split_core.h BM), four column tiles of 16 (qof: m >> 4)
TAIL_MAX_LAST = 128

CLASSES = ("far", "near_coupled", "tiny_coupled", "near_free")
FAR, NEAR_COUPLED, TINY_COUPLED, NEAR_FREE = range(4)
LADDER = (1e1, 1e2, 1e3, 1e4, 1e5, 1e6)
K_LADDER = (1, 2, 4, 6, 8, 10, 12)
SETS_FILE = "mlp_mixed_sets.npz"


# ------------------------------------------------------------------------------------------------
# tile map
# ------------------------------------------------------------------------------------------------
def split_blocks(N, ncu):
    """mlp_split_core.h split_blocks: (64-point blocks, 16-point tail blocks). The last round of 64-point
    blocks runs as four times as many 16-point blocks when it would occupy at most a quarter of the ncu
    CUs; ncu = 0 keeps 64-point blocks."""
    nb = -(-N // BM)
    if ncu <= 0 or nb == 0:
        return nb, 0
    rounds = -(-nb // ncu)
    last = nb - ncu * (rounds - 1)
    if rounds < 2 or last > TAIL_MAX_LAST or 4 * last > ncu:
        return nb, 0
    return nb - last, 4 * last


def tile_map(N, ncu=0):
    """Per point index p < N: (block, q, tile, tail). block: the launch block that computes p (64-point
    blocks first, then the 16-point tail blocks: fwd_kernel's `b`); q: its column tile inside the block
    (qof of its slot; 0 in a tail block); tile: a launch-wide id of the 16 points that share every
    B-operand scale with p; tail: whether the block is a 16-point tail block. Blocks start on multiples of
    64 and tail blocks on multiples of 16, so tile == p // 16 under either decomposition: that is why the
    tail decomposition computes bitwise what 64-point blocks compute."""
    nfull, _ = split_blocks(N, ncu)
    p = np.arange(N)
    tail = p >= nfull * BM
    block = np.where(tail, nfull + (p - nfull * BM) // 16, p // BM)
    q = np.where(tail, 0, (p % BM) // 16)
    tile = np.where(tail, nfull * 4 + (block - nfull), block * 4 + q)
    return block, q, tile, tail


# ------------------------------------------------------------------------------------------------
# input recipes
# ------------------------------------------------------------------------------------------------
def _fill(rng, cls, F):
    """xyz by class. far: each coordinate +-F * U[0.7, 1]; tiny: +-10^U[-4, -2]; near: U[-1.3, 1.3]."""
    N = cls.shape[0]
    sign = rng.choice([-1.0, 1.0], (N, 3))
    near = rng.uniform(-1.3, 1.3, (N, 3))
    far = sign * F * rng.uniform(0.7, 1.0, (N, 3))
    tiny = sign * 10.0 ** rng.uniform(-4.0, -2.0, (N, 3))
    x = np.where((cls == FAR)[:, None], far, np.where((cls == TINY_COUPLED)[:, None], tiny, near))
    return x.astype(np.float32), near.astype(np.float32)


def far_recipe(placement, F, seed=0, ncu=0):
    """One seeded scene: dict(x (N, 3) float32, x_clean (the same points with every far point replaced by a
    near one: no tile holds a far point), cls (N,) class index, t (N, 1) per-point times, eval (indices
    whose class is checked), ncu).

    placement "every": N = 200 (three blocks and a ragged one of 8 points), one far point in every tile
    (no near_free class); "quarter": N = 200, a far point in every fourth tile (tiles 1, 5, 9): the others
    hold the control class; "tail": N = 64 ncu + 40, so the last round is one block that runs as 16-point
    tail blocks (ncu > 0: the device's CU count; 16 full points, 16, 8, none), a far point inside the second
    tail block; only the last 104 points (the last 64-point block and the tail) are classified (eval), the
    rest are near filler. The draws do not depend on F except the far points' magnitude."""
    rng = np.random.default_rng(1000 + seed)
    if placement == "tail":
        assert ncu >= 4
        N = BM * ncu + 40
        assert split_blocks(N, ncu) == (ncu, 4)
    else:
        N = 200
    _, _, tile, tail = tile_map(N, ncu)
    ntile = int(tile.max()) + 1
    slot = rng.integers(0, 16, ntile)  # where in its tile the far point sits
    if placement == "every":
        far_tiles = np.arange(ntile)
    elif placement == "quarter":
        far_tiles = np.arange(1, ntile, 4)
    else:
        far_tiles = np.array([4 * ncu + 1])
    cls = np.full(N, NEAR_FREE)
    for tl in far_tiles:
        idx = np.nonzero(tile == tl)[0]
        cls[idx] = np.where(np.arange(idx.size) % 2 == 0, NEAR_COUPLED, TINY_COUPLED)
        cls[idx[min(slot[tl], idx.size - 1)]] = FAR
    x, near = _fill(rng, cls, F)
    x_clean = np.where((cls == FAR)[:, None], near, x)
    t = rng.uniform(0, 1, (N, 1)).astype(np.float32)
    ev = np.arange(N - 104, N) if placement == "tail" else np.arange(N)
    if placement == "tail":
        assert tail[cls == FAR].all()
    return dict(x=x, x_clean=x_clean, cls=cls, t=t, eval=ev, ncu=ncu, placement=placement, F=F)


def class_max(err, cls, idx=None):
    """{class name: max of err over the class's points} (err: (N,) or (N, k); idx: the points considered)."""
    err = np.asarray(err, np.float64).reshape(err.shape[0], -1).max(1)
    sel = np.zeros(err.shape[0], bool)
    sel[np.arange(err.shape[0]) if idx is None else idx] = True
    return {CLASSES[c]: float(err[sel & (cls == c)].max()) for c in range(4) if (sel & (cls == c)).any()}


# ------------------------------------------------------------------------------------------------
# function-preserving weight rescale
# ------------------------------------------------------------------------------------------------
def rescale_weights(w, K, seed=0):
    """ReLU is positively homogeneous: row i of linear.L (weight and bias) times c = 2^k_i and column i of
    every consumer (linear.L+1, whose skip layer linear.5 takes h in its LAST 256 columns, after x_emb |
    t_emb; the heads after linear.7) times 2^-k_i leaves the network function unchanged, and every scaling
    is exact in fp32. k_i: integers uniform in [-K, K], so an n-tile's rows and an activation tile's
    features span up to 2^2K. Returns (weights, c) with c[L] the (256,) float64 factors of layer L."""
    rng = np.random.default_rng(5000 + 31 * seed + K)
    out = {k: v.copy() for k, v in w.items()}
    c = [2.0 ** rng.integers(-K, K + 1, 256) for _ in range(8)]
    heads = [k[:-7] for k in w if k.endswith(".weight") and not k.startswith(("linear.", "timenet."))]
    for L in range(8):
        cf = c[L].astype(np.float32)
        out[f"linear.{L}.weight"] = out[f"linear.{L}.weight"] * cf[:, None]
        out[f"linear.{L}.bias"] = out[f"linear.{L}.bias"] * cf
        for name in ([f"linear.{L + 1}"] if L < 7 else heads):
            wt = out[name + ".weight"]
            wt[:, wt.shape[1] - 256:] = wt[:, wt.shape[1] - 256:] / cf[None, :]
    for k in out:
        assert out[k].dtype == np.float32 and np.isfinite(out[k]).all()
    return out, c


KT = 10  # rescale_tilewise: an n-tile's offset k_t in [-KT, KT]


def rescale_tilewise(w, layer=0, seed=0):
    """The same function-preserving rescale of ONE trunk layer with the exponent k_t + k_i: k_t one offset per
    16-row n-tile, the 16 values of round(linspace(-KT, KT)) in a seeded order, k_i in {-1, 0, 1} per row. Each
    n-tile keeps a range of 2^2 while the image spans 2^(2 KT + 2): a weight scale per n-tile (k_pack) loses
    nothing, one scale per image leaves the small tiles' rows 2^20 below the bound. The layer's own output,
    row by row, shows the difference (the consumer's activation tile spans the same range on the B side, so
    the network outputs past it are recorded, not asserted). Returns (weights, c) as rescale_weights, c = 1
    on the other layers."""
    rng = np.random.default_rng(7000 + seed)
    kt = rng.permutation(np.round(np.linspace(-KT, KT, 16)).astype(int))
    k = np.repeat(kt, 16) + rng.integers(-1, 2, 256)
    c = [np.ones(256) for _ in range(8)]
    c[layer] = 2.0 ** k
    cf = c[layer].astype(np.float32)
    out = {n: v.copy() for n, v in w.items()}
    out[f"linear.{layer}.weight"] = out[f"linear.{layer}.weight"] * cf[:, None]
    out[f"linear.{layer}.bias"] = out[f"linear.{layer}.bias"] * cf
    heads = [n[:-7] for n in w if n.endswith(".weight") and not n.startswith(("linear.", "timenet."))]
    for name in ([f"linear.{layer + 1}"] if layer < 7 else heads):
        wt = out[name + ".weight"]
        wt[:, wt.shape[1] - 256:] = wt[:, wt.shape[1] - 256:] / cf[None, :]
    for n in out:
        assert np.isfinite(out[n]).all()
    return out, c


def row_norm_max(err, ref):
    """max over the rows (features) of max |err| / max |ref| per row; err, ref: (N, rows). Dead rows (ref all
    zero) must carry no error."""
    rmax = np.abs(ref).max(0)
    live = rmax > 0
    assert (err[:, ~live] == 0).all()
    return float((np.abs(err)[:, live].max(0) / rmax[live]).max())


def grad_factors(w, c):
    """{parameter: array broadcastable to it} with grad(rescaled network) = grad(base network) * factor:
    dZ of layer L's row i shrinks by c[L][i], the activation feeding column j from layer L-1 grows by
    c[L-1][j] (the x_emb | t_emb columns and the timenet are untouched)."""
    f = {}
    for name, v in w.items():
        if name.startswith("timenet."):
            f[name] = np.ones(v.shape)
            continue
        L = int(name.split(".")[1]) if name.startswith("linear.") else 8
        row = 1.0 / c[L] if L < 8 else np.ones(v.shape[0])
        if name.endswith(".bias"):
            f[name] = row
            continue
        col = np.ones(v.shape[1])
        if L > 0:
            col[v.shape[1] - 256:] = c[L - 1]
        f[name] = row[:, None] * col[None, :]
    return f


# ------------------------------------------------------------------------------------------------
# numpy model of one split GEMM: layer 0
# ------------------------------------------------------------------------------------------------
def scale_exp(m):
    """mlp_split_core.h scale_for: the exponent field of the bound's float32 bits, clamped to +-60; the
    scale is 2^(14 - e) (bound -> [2^14, 2^15)). Taken on the bits: a NaN or an infinity has field 255."""
    bits = np.asarray(m, np.float32).view(np.uint32)
    e = ((bits >> 23) & 255).astype(np.int64) - 127
    return np.clip(e, -60, 60)


def split16(x, S, flush):
    """hsplit2: s = x S in fp32, hi = f16(s), lo = f16(s - hi) (s - hi is exact in fp32), as float64.
    flush: f16 subnormals (0 < |v| < 2^-14) of either half read as zero."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(x, np.float32) * np.asarray(S, np.float32)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    if flush:
        hi = np.where(np.abs(hi) < 2.0 ** -14, 0.0, hi)
        lo = np.where(np.abs(lo) < 2.0 ** -14, 0.0, lo)
    return hi, lo


def layer0_inputs(w, x, t):
    """(x_emb, t_emb) of the blender network as the kernels stage them: fp32 values (here the float64
    oracle's, rounded once)."""
    _, c = mlp_ref.forward(w, x, t, True, False)
    return c["xe"].astype(np.float32), c["te"].astype(np.float32)


def layer0_split_model(w, x, t, flush, ncu=0, w_scale="ntile", xe_floor=1.0):
    """z0 = W0 . [x_emb | t_emb] + b0 by the split path's rules (the per-point-time kernel, k_fwd<.., false>:
    one GEMM over two scale groups), float32 (N, 256):
      - A: one scale per 16-row n-tile from the tile's max |w| over the whole K (k_pack);
      - B: x_emb one scale per column tile from max(1, max |xyz|), t_emb one from the tile's max |t_emb|
        (fwd_block staging), both through scale_for's exponent clamp;
      - hi / lo through np.float16, the products hh + hl + lh (ll dropped) accumulated in float64 (the MFMA
        accumulates in fp32: the model leaves that rounding out, so it shows the representation error alone);
      - the epilogue (undo the scales, add the bias) rounded to fp32 once.
    flush: whether an f16 subnormal operand reads as zero. Nobody has measured which of the two the f16 MFMA
    (v_mfma_f32_16x16x32_f16) does on gfx950; tests/test_gpu_mlp_mixed.py records the kernels' errors beside
    both predictions. The asserted sets take flush = True, the pessimistic one.
    w_scale / xe_floor: the mutants of the scale rules ("image": one weight scale for the whole matrix;
    xe_floor = 2^20 instead of 1)."""
    W0 = w["linear.0.weight"].astype(np.float32)
    b0 = w["linear.0.bias"].astype(np.float64)
    xe, te = layer0_inputs(w, x, t)
    N = x.shape[0]
    _, _, tile, _ = tile_map(N, ncu)
    if w_scale == "ntile":
        ea = np.repeat(scale_exp(np.abs(W0).reshape(16, -1).max(1)), 16)
    else:
        ea = np.full(256, scale_exp(np.abs(W0).max()))
    Sa = 2.0 ** (14 - ea)
    ah, al = split16(W0, Sa[:, None].astype(np.float32), flush)
    z = np.zeros((N, 256))
    for tl in np.unique(tile):
        idx = np.nonzero(tile == tl)[0]
        acc = np.zeros((idx.size, 256))
        xb = np.float32(max(xe_floor, np.abs(x[idx]).max()))
        for cols, v, bound in ((slice(0, 63), xe[idx], xb), (slice(63, 93), te[idx], np.abs(te[idx]).max())):
            Sb = 2.0 ** (14 - scale_exp(bound))
            bh, bl = split16(v, np.float32(Sb), flush)
            p = bh @ ah[:, cols].T + bl @ ah[:, cols].T + bh @ al[:, cols].T
            acc += p / (Sa[None, :] * Sb)
        z[idx] = acc
    return (z + b0).astype(np.float32)


def layer0_fp32(w, x, t):
    """The plain fp32 layer 0: the same fp32 inputs, one fp32 multiply-add per feature in feature order
    (a fixed order: the asserted sets must not depend on a BLAS)."""
    W0 = w["linear.0.weight"].astype(np.float32)
    xe, te = layer0_inputs(w, x, t)
    h = np.concatenate([xe, te], 1)
    acc = np.broadcast_to(w["linear.0.bias"].astype(np.float32), (x.shape[0], 256)).copy()
    for k in range(h.shape[1]):
        acc += h[:, k:k + 1] * W0[None, :, k]
    return acc


def layer0_ref(w, x, t):
    """float64 z0 from the float64 encodings (the oracle's)."""
    _, c = mlp_ref.forward(w, x, t, True, False)
    return c["z"][0]


def asserted_prefix(ladder, ok):
    """The rungs up to (not including) the first one that misses."""
    out = []
    for r, o in zip(ladder, ok):
        if not o:
            break
        out.append(r)
    return out
