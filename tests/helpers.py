"""Shared test helpers: scenes, camera settings, and HIP-vs-oracle comparisons."""
import math

import numpy as np
import torch

from deformgs.synthetic import synth_camera, synth_gaussians
from oracle.raster import OracleRaster, make_settings


def scene(N, H, W, seed=0, cam_index=0, scale_boost=0.0, device="cpu", bg=(0.0, 0.0, 0.0), sh_degree=3, sh_coeffs=16):
    """sh_coeffs: the SH coefficients per Gaussian (M <= 16: the first M rows of the degree-3 set, so
    scenes of different M share every other input)."""
    g = synth_gaussians(N, seed=seed, device="cpu")
    g["scaling"] = g["scaling"] + scale_boost
    cam = synth_camera(W, H, index=cam_index, device="cpu")
    inputs = dict(
        means3D=g["xyz"],
        shs=torch.cat([g["features_dc"], g["features_rest"]], 1)[:, :sh_coeffs].contiguous(),
        opacities=torch.sigmoid(g["opacity"]),
        scales=torch.exp(g["scaling"]),
        rotations=torch.nn.functional.normalize(g["rotation"]),
    )
    rs = dict(H=H, W=W, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2),
              bg=torch.tensor(bg, dtype=torch.float32), scale_modifier=1.0,
              viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree,
              campos=cam.camera_center)
    return inputs, rs, cam


def oracle_run(inputs, rs, dcolor=None, ddepth=None, use_cov=False, use_colors=False):
    s = make_settings(rs["H"], rs["W"], rs["tanfovx"], rs["tanfovy"], rs["bg"].numpy(), rs["scale_modifier"],
                      rs["viewmatrix"].numpy(), rs["projmatrix"].numpy(), rs["sh_degree"], rs["campos"].numpy())
    kw = dict(means3D=inputs["means3D"].numpy(), opacities=inputs["opacities"].numpy())
    if use_colors:
        kw["colors_precomp"] = inputs["colors"].numpy()
    else:
        kw["shs"] = inputs["shs"].numpy()
    if use_cov:
        kw["cov3D_precomp"] = inputs["cov3D"].numpy()
    else:
        kw["scales"] = inputs["scales"].numpy()
        kw["rotations"] = inputs["rotations"].numpy()
    o = OracleRaster(s, **kw)
    g = o.backward(dcolor, ddepth) if dcolor is not None else None
    return o, g


def settings_for_gpu(rs, device="cuda"):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=rs["H"], image_width=rs["W"], tanfovx=rs["tanfovx"], tanfovy=rs["tanfovy"],
        bg=rs["bg"].to(device), scale_modifier=rs["scale_modifier"], viewmatrix=rs["viewmatrix"].to(device),
        projmatrix=rs["projmatrix"].to(device), sh_degree=rs["sh_degree"], campos=rs["campos"].to(device),
        prefiltered=False, debug=False)


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def frac_close(a, b, atol, rtol):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ok = np.abs(a - b) <= atol + rtol * np.abs(b)
    return float(ok.mean())


# saved-activation rows of the fused MLP (csrc/mlp_shared.h: S_H0.., S_H4.., S_TH), feature-major [rows][Ns]
_S_H = [0, 256, 512, 768, 1120, 1376, 1632, 1888]
_S_TH = 2160


def mlp_relu_masks(output, N, blender, exact, th_saved=True):
    """The fused MLP kernel's own relu' masks {layer: bool (N, 256), "th": ...} read back from the
    activations it saved for backward (autograd ctx of the fused node reached from `output`).
    th_saved=False: the forward ran with DGS_MLP_UNIFORM_T (one-element or stride-0 t), which keeps
    no per-point TH rows; the oracle then uses its own TH masks."""
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
    assert node is not None, "fused MLP node not found in the autograd graph"
    _, saved = node.saved_tensors
    block = 32 if exact else 64
    Ns = (N + block - 1) // block * block
    rows = 2416 if blender else 2144
    sv = saved[: rows * Ns].view(rows, Ns)[:, :N].cpu().numpy()
    masks = {i: (sv[r:r + 256] > 0).T for i, r in enumerate(_S_H)}
    if blender and th_saved:
        masks["th"] = (sv[_S_TH:_S_TH + 256] > 0).T
    return masks


# ------------------------------------------------------------------------------------------------
# Integer outputs and gradient tails vs the oracle (radii / num_rendered exact, every
# out-of-tolerance gradient element accounted for). The rasterizer makes discrete decisions on fp32
# values: radius = ceil(3 sqrt(lambda_max)), the tile rectangle = trunc((px -+ r) / 16), the z <= 0.2
# cull, and per pixel the alpha / transmittance thresholds. Two fp32 implementations of the same
# math (the GPU's fma contraction and exp2-form exponent vs the oracle's plain C) agree on such a
# decision unless its input sits within a few ulps of the threshold; these helpers find those inputs
# in the oracle's own trace, so the tests can require exact equality everywhere else.
# ------------------------------------------------------------------------------------------------
def _rect(px, py, rad, gx, gy):
    """oracle/raster_ref.c tile rectangle (float32 arithmetic in the C expression order)."""
    f = np.float32
    r = rad.astype(f)
    x0 = np.minimum(gx, np.maximum(0, np.trunc((px - r) / f(16)))).astype(np.int64)
    y0 = np.minimum(gy, np.maximum(0, np.trunc((py - r) / f(16)))).astype(np.int64)
    x1 = np.minimum(gx, np.maximum(0, np.trunc(((px + r) + f(16) - f(1)) / f(16)))).astype(np.int64)
    y1 = np.minimum(gy, np.maximum(0, np.trunc(((py + r) + f(16) - f(1)) / f(16)))).astype(np.int64)
    return x0, y0, x1, y1


def integer_ambiguity(o, eps_rad=4e-6, delta_px=1e-3, eps_z=1e-6):
    """Per Gaussian: which integer decisions of the oracle's preprocess sit within fp32 reach of
    their threshold. Returns dict(rad_amb, cull_amb, rect_amb (bool N), area_lo / area_hi (int N: the
    tile count over the ambiguous alternatives), tile_mask (bool tiles: tiles any ambiguous
    alternative rectangle covers))."""
    H, W = o.s.image_height, o.s.image_width
    gx, gy = (W + 15) // 16, (H + 15) // 16
    raw = o.preprocess_raw()
    radf, vz, pxy = raw["radf"], raw["vz"], raw["pxy"]
    px, py = pxy[:, 0], pxy[:, 1]
    live = radf > 0  # passed the z and det culls (a radius exists)
    rad = np.ceil(radf).astype(np.int64)
    frac = radf - np.floor(radf)
    rad_amb = live & ((frac <= eps_rad * np.maximum(radf, 1.0)) | (1.0 - frac <= eps_rad * np.maximum(radf, 1.0)))
    cull_amb = np.abs(vz - np.float32(0.2)) <= eps_z
    alts = [rad]
    alts.append(np.where(rad_amb, np.where(frac < 0.5, rad + 1, rad - 1), rad))
    area0 = None
    lo = hi = None
    tmask = np.zeros(gx * gy, bool)
    amb = np.zeros_like(live)
    d = np.float32(delta_px)
    for r in alts:
        for ox, oy in ((0, 0), (d, 0), (-d, 0), (0, d), (0, -d), (d, d), (-d, -d), (d, -d), (-d, d)):
            x0, y0, x1, y1 = _rect(px + np.float32(ox), py + np.float32(oy), r, gx, gy)
            area = np.where(live, (x1 - x0) * (y1 - y0), 0)
            if area0 is None:
                area0, ref_rect = area, (x0, y0, x1, y1)
                lo, hi = area.copy(), area.copy()
                continue
            diff = live & ((x0 != ref_rect[0]) | (y0 != ref_rect[1]) | (x1 != ref_rect[2]) | (y1 != ref_rect[3]))
            amb |= diff
            lo, hi = np.minimum(lo, area), np.maximum(hi, area)
            for i in np.nonzero(diff)[0]:  # tiles in one rectangle and not the other
                m = np.zeros((gy, gx), bool)
                m[ref_rect[1][i]:ref_rect[3][i], ref_rect[0][i]:ref_rect[2][i]] = True
                m2 = np.zeros((gy, gx), bool)
                m2[y0[i]:y1[i], x0[i]:x1[i]] = True
                tmask |= (m ^ m2).reshape(-1)
    if cull_amb.any():  # a Gaussian on the z cull: present in one and absent in the other
        lo = np.where(cull_amb, 0, lo)
        hi = np.where(cull_amb, np.maximum(hi, area0), hi)
    return dict(rad_amb=rad_amb, cull_amb=cull_amb, rect_amb=amb | cull_amb, area_lo=lo, area_hi=hi,
                area=area0, tile_mask=tmask, gx=gx, gy=gy)


def check_integer_outputs(o, radii_gpu, nr_gpu, stats=None):
    """radii equal to the oracle's except where the radius ceil or the z cull is fp32-ambiguous;
    num_rendered equal to the oracle's up to the tile counts of rect-ambiguous Gaussians (exactly
    equal when there is none). Returns the ambiguity dict."""
    amb = integer_ambiguity(o)
    radii_gpu = np.asarray(radii_gpu)
    mism = radii_gpu != o.radii
    explained = amb["rad_amb"] | amb["cull_amb"] | amb["rect_amb"]
    slack = int((amb["area_hi"] - amb["area_lo"]).sum())
    if stats is not None:
        stats.update(radii_mismatch=int(mism.sum()), radii_unexplained=int((mism & ~explained).sum()),
                     rad_amb=int(amb["rad_amb"].sum()), rect_amb=int(amb["rect_amb"].sum()),
                     nr_gpu=int(nr_gpu) if nr_gpu is not None else None, nr_oracle=int(o.num_rendered),
                     nr_slack=slack)
    assert not (mism & ~explained).any(), (
        "radii differ from the oracle on Gaussians whose radius is not fp32-ambiguous",
        np.nonzero(mism & ~explained)[0][:10])
    if nr_gpu is not None:
        assert abs(int(nr_gpu) - int(o.num_rendered)) <= slack, (int(nr_gpu), int(o.num_rendered), slack)
    return amb


def tail_flags(o, amb=None, eps=1e-5):
    """Gaussians (and pixels) whose gradient (value) may legitimately differ from the oracle's by
    more than rounding: a near-threshold blend decision in their pixel (oracle or_flip_flags), a
    near-threshold gradient mask of their own preprocess (the EWA frustum clamp, the SH colour clamp:
    or_preprocess_flags), or a fp32-ambiguous radius / rectangle / cull (integer_ambiguity)."""
    g, px = o.flip_flags(eps)
    g = g | o.preprocess_flags(eps)
    if amb is not None:
        g = g | amb["rad_amb"] | amb["rect_amb"] | amb["cull_amb"]
        H, W = px.shape
        tm = amb["tile_mask"].reshape(amb["gy"], amb["gx"])
        px = px | np.kron(tm, np.ones((16, 16), bool))[:H, :W]
    return g, px


# The tail sets: the checks ASSERT against the near-threshold decisions within a relative 1e-5 of
# their threshold (1e-4 flagged ~47 % of the Gaussians at the bench size, while every
# recorded outlier already sat within 1e-5); the 1e-4 and 1e-6 sets are computed too and their flagged
# and unexplained counts recorded beside it (how close to their thresholds the outliers sit).
ASSERT_EPS = 1e-5
RECORD_EPS = (1e-4, 1e-5, 1e-6)
# Pixel VALUES are held to the 1e-4 set: a pixel's transmittance carries the relative error of every
# (1 - alpha) factor in front of it, which is the alpha's error times alpha / (1 - alpha) (up to 99x at
# the 0.99 clamp), so the T (1 - alpha) < 1e-4 stop of two fp32 implementations can differ for inputs
# 1e-5 .. 1e-4 from the threshold (measured: at 55k-100k @ 800^2, 1-5 of the 6-14 pixels off by > 1e-4
# sit there; none outside the 1e-4 set). The gradients are held to the 1e-5 set.
IMAGE_EPS = 1e-4


def tail_sets(o, amb=None):
    """{eps: (gflag, pflag)} for RECORD_EPS."""
    return {e: tail_flags(o, amb, e) for e in RECORD_EPS}


def check_image(img, o, sets, stats=None, name="image"):
    """mean |err| <= 1e-5, >= 99.9 % of values within 1e-4, and every value off by more than 1e-4 at
    a pixel with a near-threshold decision (sets[IMAGE_EPS])."""
    err = np.abs(np.asarray(img) - o.color)
    bad = (err > 1e-4).any(0)
    pflag = sets[IMAGE_EPS][1]
    if stats is not None:
        stats[name] = dict(mean=float(err.mean()), bad_px=int(bad.sum()), unexplained=int((bad & ~pflag).sum()),
                           flagged_px=int(pflag.sum()))
        for e, (_, pf) in sets.items():
            stats[name][f"flagged_px@{e:g}"] = int(pf.sum())
            stats[name][f"unexplained@{e:g}"] = int((bad & ~pf).sum())
    assert err.mean() <= 1e-5 and (err <= 1e-4).mean() >= 0.999, err.mean()
    assert not (bad & ~pflag).any(), ("image values off by > 1e-4 at pixels without a near-threshold decision",
                                      np.argwhere(bad & ~pflag)[:10])


def check_gaussian_grad(a, b, sets, name, stats=None, atol_frac=2e-3, rtol=1e-3, max_bad_frac=1e-4, min_bad=4,
                        max_ratio=10.0):
    """Per-Gaussian gradient rows a (GPU) vs b (oracle), tolerance atol_frac of the tensor's max +
    rtol relative (float32 kernels vs the oracle). Asserted (bars at what is measured):
      - at most max_bad_frac (1e-4) of the elements outside the tolerance (at least min_bad = 4
        elements allowed, so a single near-threshold Gaussian of a few-thousand-Gaussian case counts
        as what it is: one Gaussian);
      - every element outside the tolerance on a Gaussian of the 1e-5 tail set (sets[ASSERT_EPS]);
      - no element off by more than max_ratio (10) times its tolerance, flagged or not (a single
        alpha / transmittance decision moves a gradient by a bounded amount; measured <= 2.9).
    sets: {eps: (gflag, pflag)} (tail_sets); flagged and unexplained counts recorded for every eps."""
    gflag = sets[ASSERT_EPS][0]
    N = gflag.shape[0]
    a = np.asarray(a, np.float64).reshape(N, -1)
    b = np.asarray(b, np.float64).reshape(N, -1)
    tol = atol_frac * max(np.abs(b).max(), 1e-30) + rtol * np.abs(b)
    ratio = np.abs(a - b) / tol
    bad = ratio > 1.0
    bad_g = bad.any(1)
    unexplained = bad_g & ~gflag
    nbad = int(bad.sum())
    worst = float(ratio.max())
    if stats is not None:
        stats[name] = dict(bad_frac=float(bad.mean()), bad_elems=nbad, bad_gauss=int(bad_g.sum()),
                           flagged=int(gflag.sum()), unexplained=int(unexplained.sum()),
                           worst_unexplained=float(ratio[unexplained].max()) if unexplained.any() else 0.0,
                           worst_ratio=worst, rel=rel_err(a, b))
        for e, (gf, _) in sets.items():
            stats[name][f"flagged@{e:g}"] = int(gf.sum())
            stats[name][f"unexplained@{e:g}"] = int((bad_g & ~gf).sum())
    assert nbad <= max(max_bad_frac * bad.size, min_bad), (name, nbad, bad.size, rel_err(a, b))
    assert not unexplained.any(), (name, "gradient outside tolerance on Gaussians with no near-threshold decision",
                                   np.nonzero(unexplained)[0][:10])
    assert worst <= max_ratio, (name, "gradient off by more than 10x its tolerance", worst)


def write_stats(tag, stats):
    """Append the parity statistics of one test to gpurun_out/parity_stats.jsonl (when that directory
    exists: GPU runs), for the record in profiles/."""
    import json
    import os
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, "parity_stats.jsonl"), "a") as f:
            f.write(json.dumps({"test": tag, **stats}, default=float) + "\n")
