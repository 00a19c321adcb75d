"""The render-input kernels (csrc/inputs.hip: k_inputs_fwd / k_inputs_bwd) called directly, against the
glue of renderer.render()'s generic branch in float64 on the CPU, for every SH layout a GaussianModel
can have (features_rest of 0 / 3 / 8 / 15 rows: sh_degree 0 .. 3); and models of degree 0 / 1 / 2 through
render(), the training step and render_frames().

What is data movement is held bitwise: shs = cat(f_dc, f_rest), the dc / rest gradients (slices of the
upstream SH gradient), means3D = xyz + d_xyz (one fp32 add), and the deformation-gradient columns
(copies of the upstream gradients). The activations are a handful of fp32 operations per element and
are held to 8 fp32 ulps of the element's scale (expf, a division and a sqrtf chained, each within
1 - 2 ulps, doubled where the result sits at the bottom of its binade); where 8 ulps is not met the bar
is twice the error of torch's own fp32 CPU evaluation of the same glue against float64, measured on the
same inputs. The scale of an element is the largest magnitude among the terms summed into it:
  scales    = exp(scaling) + d_scaling        max(exp(scaling), |d_scaling|)
  rotations = q / |q| + d_rotation            max(|q_i| / |q|, |d_rotation_i|)
  opacities = sigmoid(opacity)                itself
  g_scaling = g exp(scaling)                  itself
  g_rotation = (g - y (y.g)) / |q|            |g| / max(|q|, 1e-12)  (the difference cancels)
  g_opacity = g (1 - s) s                     |g| s  (1 - s carries s's rounding error against 1)
"""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import write_stats

pytestmark = pytest.mark.gpu

PS = (1, 5, 257, 1031)
M_RESTS = (0, 3, 8, 15)
NAMES = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")
ULP_BAR = 8.0


def _draw(P, M_rest, seed, width=10):
    """Parameters of the magnitudes of deformgs.synthetic, deformation rows of a trained network's and
    random upstream gradients for the five outputs (CPU fp32)."""
    gen = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    op = torch.rand(P, 1, generator=gen) * 0.9 + 0.05
    x = dict(xyz=torch.rand(P, 3, generator=gen) * 2.6 - 1.3, f_dc=0.5 * n(P, 1, 3), f_rest=0.05 * n(P, M_rest, 3),
             scaling=math.log(0.02) + 0.1 * n(P, 3), rotation=n(P, 4), opacity=torch.log(op / (1 - op)))
    d = 0.01 * n(P, width)
    up = dict(means=n(P, 3), shs=n(P, 1 + M_rest, 3), opac=n(P, 1), scales=n(P, 3), rots=n(P, 4))
    return x, d, up


def _reference(x, d, up, dtype, se3=False):
    """gaussian_renderer/__init__.py:70-112 as renderer.render()'s generic branch states it, on the CPU in
    `dtype`: (outputs, gradients of the six parameters and the deformation rows)."""
    from deformgs.rigid import screw_from_raw
    p = {k: v.to(dtype, copy=True).requires_grad_(True) for k, v in x.items()}
    dd = d.to(dtype, copy=True).requires_grad_(True) if d is not None else None
    r0, s0 = (6, 10) if se3 else (3, 7)
    if se3:
        M = screw_from_raw(dd[:, 0:3], dd[:, 3:6])
        means = torch.bmm(M[:, :3, :3], p["xyz"].unsqueeze(-1)).squeeze(-1) + M[:, :3, 3]
    else:
        means = p["xyz"] + dd[:, 0:3] if dd is not None else p["xyz"] * 1
    scales = torch.exp(p["scaling"])
    rots = torch.nn.functional.normalize(p["rotation"])
    if dd is not None:
        scales = scales + dd[:, s0:s0 + 3]
        rots = rots + dd[:, r0:r0 + 4]
    outs = dict(means=means, shs=torch.cat((p["f_dc"], p["f_rest"]), 1), opac=torch.sigmoid(p["opacity"]),
                scales=scales, rots=rots)
    loss = sum((outs[k] * up[k].to(dtype)).sum() for k in outs)
    leaves = list(p.values()) + ([dd] if dd is not None else [])
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = dict(zip(NAMES + ("deform",), gs))
    return {k: v.detach() for k, v in outs.items()}, grads


def _elem_scales(x, d, up, se3=False):
    """The scale of every element compared in ulps (module docstring), float64."""
    r0, s0 = (6, 10) if se3 else (3, 7)
    es = torch.exp(x["scaling"].double())
    q = x["rotation"].double()
    n = q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    s = torch.sigmoid(x["opacity"].double())
    ds = d[:, s0:s0 + 3].double().abs() if d is not None else torch.zeros_like(es)
    dr = d[:, r0:r0 + 4].double().abs() if d is not None else torch.zeros_like(q)
    return dict(scales=torch.maximum(es, ds), rots=torch.maximum((q / n).abs(), dr), opac=s,
                scaling=(up["scales"].double() * es).abs(),
                rotation=(up["rots"].double().norm(dim=1, keepdim=True) / n).expand(-1, 4),
                opacity=up["opac"].double().abs() * s)


@functools.lru_cache(maxsize=None)
def _case(P, M_rest, deform, se3=False):
    """Inputs, the float64 reference and torch's fp32 CPU evaluation (the yardstick), computed once and
    shared by the variants; the parameters and upstream gradients do not depend on `deform`."""
    x, d, up = _draw(P, M_rest, 1000 * P + M_rest, 13 if se3 else 10)
    if se3:  # the raw screw head of tests/test_gpu_render.py's _raw13
        from test_gpu_render import _raw13
        d = _raw13(P, 1000 * P + M_rest, "cpu").detach()
    if not deform:
        d = None
    return x, d, up, _reference(x, d, up, torch.float64, se3), _reference(x, d, up, torch.float32, se3), \
        _elem_scales(x, d, up, se3)


def _ulps(got, ref, scale):
    if got.numel() == 0:
        return 0.0
    ulp = np.spacing(scale.numpy().astype(np.float32)).astype(np.float64)
    return float((np.abs(got.double().numpy() - ref.numpy()) / ulp).max())


def _run_apply(x, d, up, se3=False, with_sh=True, need=NAMES + ("deform",)):
    """_GaussianInputs.apply on the GPU -> (outputs, gradients) as CPU tensors (None where absent)."""
    from deformgs.renderer import _GaussianInputs
    p = {k: v.cuda().requires_grad_(k in need) for k, v in x.items()}
    dd = d.cuda().requires_grad_("deform" in need) if d is not None else None
    means, shs, opac, scales, rots = _GaussianInputs.apply(p["xyz"], p["f_dc"], p["f_rest"], p["scaling"],
                                                           p["rotation"], p["opacity"], dd, se3, with_sh)
    outs = dict(means=means, shs=shs, opac=opac, scales=scales, rots=rots)
    live = [k for k in outs if outs[k] is not None]
    torch.autograd.backward([outs[k] for k in live], [up[k].cuda() for k in live])
    grads = {k: (None if p[k].grad is None else p[k].grad.cpu()) for k in NAMES}
    grads["deform"] = None if dd is None or dd.grad is None else dd.grad.cpu()
    return {k: (None if v is None else v.detach().cpu()) for k, v in outs.items()}, grads


SENTINEL_IN, SENTINEL_G = 1e30, -12345.678


def _run_c_stride12(x, d, up):
    """The C entry points with deformation rows of stride 12: columns 10 / 11 hold a huge value on the way
    in (never read) and a sentinel in the gradient buffer (never written)."""
    from deformgs import _lib
    lib = _lib.load()
    P, M_rest = x["xyz"].shape[0], x["f_rest"].shape[1]
    t = {k: v.cuda() for k, v in x.items()}
    u = {k: v.cuda() for k, v in up.items()}
    d12 = torch.full((P, 12), SENTINEL_IN, device="cuda")
    d12[:, :10] = d.cuda()
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")  # noqa: E731
    o = dict(means=e(P, 3), shs=e(P, 1 + M_rest, 3), opac=e(P, 1), scales=e(P, 3), rots=e(P, 4))
    ptr, st = _lib.ptr, _lib.stream_ptr(torch.device("cuda"))
    _lib.check(lib.dgs_gaussian_inputs_forward(
        P, M_rest, ptr(t["xyz"]), ptr(t["f_dc"]), ptr(t["f_rest"]), ptr(t["scaling"]), ptr(t["rotation"]),
        ptr(t["opacity"]), ptr(d12), 12, ptr(o["means"]), ptr(o["shs"]), ptr(o["scales"]), ptr(o["rots"]),
        ptr(o["opac"]), st), "gaussian_inputs_forward")
    g = dict(xyz=e(P, 3), f_dc=e(P, 1, 3), f_rest=e(P, M_rest, 3), scaling=e(P, 3), rotation=e(P, 4), opacity=e(P, 1))
    g12 = torch.full((P, 12), SENTINEL_G, device="cuda")
    _lib.check(lib.dgs_gaussian_inputs_backward(
        P, M_rest, ptr(t["scaling"]), ptr(t["rotation"]), ptr(t["opacity"]), ptr(u["means"]), ptr(u["shs"]),
        ptr(u["scales"]), ptr(u["rots"]), ptr(u["opac"]), ptr(g["xyz"]), ptr(g["f_dc"]), ptr(g["f_rest"]),
        ptr(g["scaling"]), ptr(g["rotation"]), ptr(g["opacity"]), ptr(g12), 12, st), "gaussian_inputs_backward")
    torch.cuda.synchronize()
    g12 = g12.cpu()
    assert torch.equal(g12[:, 10:], torch.full((P, 2), SENTINEL_G)), "columns past the 10 deformation outputs written"
    grads = {k: v.cpu() for k, v in g.items()}
    grads["deform"] = g12[:, :10].contiguous()
    return {k: v.cpu() for k, v in o.items()}, grads


def _compare(tag, case, outs, grads, se3=False, with_sh=True, need=NAMES + ("deform",)):
    """Bitwise where the kernels move data, ulps of the element's scale elsewhere (module docstring);
    records the measured maxima of the kernel and of torch's fp32 evaluation before asserting."""
    x, d, up, (o64, g64), (o32, g32), sc = case
    r0, s0 = (6, 10) if se3 else (3, 7)
    if with_sh:
        assert torch.equal(outs["shs"], torch.cat((x["f_dc"], x["f_rest"]), 1))
    else:
        assert outs["shs"] is None
    for k, ref in (("f_dc", up["shs"][:, :1]), ("f_rest", up["shs"][:, 1:])):
        if with_sh and k in need:
            assert grads[k].shape == x[k].shape and torch.equal(grads[k], ref), k
        else:
            assert grads[k] is None, k
    if not se3:
        assert torch.equal(outs["means"], x["xyz"] + d[:, 0:3] if d is not None else x["xyz"])
        if "xyz" in need:
            assert torch.equal(grads["xyz"], up["means"])
    gd = grads["deform"]
    if d is not None and "deform" in need:
        assert gd.shape == d.shape
        assert torch.equal(gd[:, r0:r0 + 4], up["rots"]) and torch.equal(gd[:, s0:s0 + 3], up["scales"])
        if not se3:
            assert torch.equal(gd[:, 0:3], up["means"])
    else:
        assert gd is None
    for k in NAMES:
        assert (grads[k] is None) == (k not in need or (k in ("f_dc", "f_rest") and not with_sh)), k
    stats, fails = {}, []
    pairs = [("scales", outs["scales"], o64["scales"], o32["scales"]), ("rots", outs["rots"], o64["rots"], o32["rots"]),
             ("opac", outs["opac"], o64["opac"], o32["opac"])]
    pairs += [(k, grads[k], g64[k], g32[k]) for k in ("scaling", "rotation", "opacity") if k in need]
    for k, got, r64, r32 in pairs:
        assert got.shape == r64.shape and bool(torch.isfinite(got).all()), k
        mine, torch32 = _ulps(got, r64, sc[k]), _ulps(r32, r64, sc[k])
        stats[k] = dict(kernel_ulps=mine, torch_fp32_ulps=torch32)
        if mine > max(ULP_BAR, 2.0 * torch32):
            fails.append((k, mine, torch32))
    if se3:  # the bars of test_se3_matrices_match_rigid_utils: values 2e-6 absolute, gradients 1e-4 of the max
        stats["means_abs"] = float((outs["means"].double() - o64["means"]).abs().max())
        se3_g = [("xyz", grads["xyz"], g64["xyz"]), ("raw", gd[:, :6], g64["deform"][:, :6])]
        for k, got, ref in se3_g:
            stats[k + "_rel"] = float((got.double() - ref).abs().max() / ref.abs().max())
    write_stats(f"inputs_vs_f64[{tag}]", stats)
    print(f"inputs_vs_f64[{tag}]", stats)
    assert not fails, fails
    if se3:
        assert stats["means_abs"] < 2e-6 and stats["xyz_rel"] < 1e-4 and stats["raw_rel"] < 1e-4, stats


def test_shapes_cover_the_kernel_paths():
    """The facts about the shapes that the cases below rely on (k_inputs_*: one thread per 16-byte SH
    unit, then one thread per Gaussian, 256 per workgroup)."""
    for C in (1, 9):  # a last unit of 3 floats: the scalar tail
        assert (5 * 3 * C) % 4 == 3
    for M_rest in M_RESTS:
        C = 1 + M_rest
        assert ((257 * 3 * C + 3) // 4) % 256 != 0      # the SH / activation boundary inside a workgroup
        assert (1031 * 3 * C + 3) // 4 > 512 and 1031 > 512  # several workgroups of each kind
    assert [3 * (1 + m) % 4 for m in M_RESTS] == [3, 0, 3, 0]  # rows of 3 and 27 floats straddle units


@pytest.mark.parametrize("M_rest", M_RESTS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("variant", ["plain", "rows10", "stride12", "no_sh", "need_a", "need_b"])
def test_inputs_match_float64(variant, P, M_rest):
    """plain: no deformation; rows10: a contiguous (P, 10) deformation output; stride12: the C entry
    points on rows of stride 12; no_sh: with_sh=False (the split-SH rasterizer's form: no shs, no dc /
    rest gradients); need_a / need_b: needs_input_grad false for a subset (null gradient outputs)."""
    deform = variant != "plain"
    case = _case(P, M_rest, deform)
    x, d, up = case[:3]
    kw = {}
    if variant == "stride12":
        outs, grads = _run_c_stride12(x, d, up)
    else:
        if variant == "no_sh":
            kw = dict(with_sh=False)
        elif variant == "need_a":
            kw = dict(need=("xyz", "f_rest", "rotation", "deform"))
        elif variant == "need_b":
            kw = dict(need=("f_dc", "scaling", "opacity"))
        outs, grads = _run_apply(x, d, up, **kw)
    _compare(f"P={P},M_rest={M_rest},{variant}", case, outs, grads, **kw)


@pytest.mark.parametrize("M_rest", (3, 15))
@pytest.mark.parametrize("P", (5, 257))
def test_inputs_se3_match_float64(P, M_rest):
    """6-DoF rows [w_r v_r d_rot d_scale]: means3D = R xyz + p of deformgs.rigid.screw_from_raw in
    float64, at the bars of test_se3_matrices_match_rigid_utils; everything else as the plain kernel."""
    case = _case(P, M_rest, True, True)
    x, d, up = case[:3]
    outs, grads = _run_apply(x, d, up, se3=True)
    _compare(f"P={P},M_rest={M_rest},se3", case, outs, grads, se3=True)


@pytest.mark.parametrize("deform", [False, True])
def test_rotation_norm_clamp(deform):
    """rotation = 0 exactly and |rotation| = 1e-20 (below normalize's eps = 1e-12): forward q / 1e-12,
    backward g / 1e-12, as torch.nn.functional.normalize in float64 on the same rows."""
    P, M_rest = 70, 3
    x, d, up = _draw(P, M_rest, 7)
    x["rotation"][0:4] = 0.0
    x["rotation"][4:8] = torch.tensor([[1e-20, 0, 0, 0], [0, 6e-21, 8e-21, 0], [0, 0, 0, -1e-20],
                                       [5e-21, -5e-21, 5e-21, 5e-21]])
    if not deform:
        d = None
    case = (x, d, up, _reference(x, d, up, torch.float64), _reference(x, d, up, torch.float32), _elem_scales(x, d, up))
    # the reference on these rows is what the kernel's clamp branch states
    o64, g64 = case[3]
    dr = d[:8, 3:7].double() if deform else 0.0
    assert torch.allclose(o64["rots"][:8], x["rotation"][:8].double() / 1e-12 + dr, rtol=1e-15, atol=0)
    assert torch.allclose(g64["rotation"][:8], up["rots"][:8].double() / 1e-12, rtol=1e-15, atol=0)
    outs, grads = _run_apply(x, d, up)
    _compare(f"P={P},M_rest={M_rest},clamp,{'rows10' if deform else 'plain'}", case, outs, grads)
    if not deform:
        assert torch.count_nonzero(outs["rots"][0:4]) == 0
    got, want = grads["rotation"][:8].double(), up["rots"][:8].double() / 1e-12
    assert float(((got - want).abs() / want.abs()).max()) < 2.0 ** -22


@pytest.mark.parametrize("M_rest", (0, 3))
def test_inputs_empty(M_rest):
    """P = 0: empty outputs and gradients, and neither kernel is launched (the library's launch counters
    stand still; they move for P = 1)."""
    from deformgs import _lib
    lib = _lib.load()
    counts = lambda: (lib.dgs_timing_launches(b"inputs_fwd"), lib.dgs_timing_launches(b"inputs_bwd"))  # noqa: E731
    lib.dgs_timing_enable(1)
    try:
        x, d, up = _draw(0, M_rest, 1)
        before = counts()
        outs, grads = _run_apply(x, d, up)
        assert counts() == before
        assert [tuple(outs[k].shape) for k in ("means", "shs", "opac", "scales", "rots")] == \
            [(0, 3), (0, 1 + M_rest, 3), (0, 1), (0, 3), (0, 4)]
        for k in NAMES:
            assert grads[k].shape == x[k].shape, k
        assert tuple(grads["deform"].shape) == (0, 10)
        x, d, up = _draw(1, M_rest, 1)
        _run_apply(x, d, up)
        assert counts() == (before[0] + 1, before[1] + 1)
    finally:
        lib.dgs_timing_enable(0)


# ---- models of sh_degree 0 / 1 / 2 through render(), the training step and render_frames() ----
def _low_model(N, degree, seed, active=None, train=False):
    from deformgs.gaussian_model import GaussianModel
    from deformgs.synthetic import synth_gaussians
    g = synth_gaussians(N, seed=seed, device="cuda", sh_degree=degree)
    gm = GaussianModel(degree)
    gm.from_tensors(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"],
                    active_sh_degree=active)
    assert tuple(gm._features_rest.shape) == (N, (degree + 1) ** 2 - 1, 3)
    if train:
        from deformgs.arguments import OptimizationParams
        gm.training_setup(OptimizationParams())
    return gm


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_fused_inputs_match_torch_glue_low_degree(degree):
    """test_fused_inputs_match_torch_glue (tests/test_gpu_render.py) for GaussianModel(0 / 1 / 2): the fused
    input kernels with the SH concatenation and the plain rasterizer on M = 1 / 4 / 9 rows, vs the torch
    glue, at that test's tolerances."""
    from deformgs import renderer
    from deformgs.arguments import PipelineParams
    from deformgs.synthetic import synth_camera
    from diff_gaussian_rasterization import split_sh_ok
    seed = 5

    def _grads(gm, out, pkg, gt):  # tests/test_gpu_render.py's, with a gradient of (N, 0, 3) allowed to be absent
        loss = (pkg["render"] - gt).abs().mean() + 0.1 * pkg["depth"].mean()
        ps = [gm._xyz, gm._features_dc, gm._features_rest, gm._scaling, gm._rotation, gm._opacity, out]
        for p in ps:
            p.grad = None
        loss.backward()
        return [p.grad.clone() if p.grad is not None else torch.zeros_like(p) for p in ps]

    gm = _low_model(3000, degree, seed)
    cam = synth_camera(160, 128, index=seed, fid=0.3, device=torch.device("cuda"))
    out = (torch.randn(3000, 10, generator=torch.Generator().manual_seed(seed)) * 0.01).cuda().requires_grad_(True)
    pipe, bg = PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device="cuda")
    gt = torch.rand(3, 128, 160, device="cuda")
    dx, dr, ds = out[:, 0:3], out[:, 3:7], out[:, 7:10]
    assert torch.is_tensor(renderer._fused_deform_rows(gm, dx, dr, ds)) and renderer._fused_ok(gm)
    assert not split_sh_ok(gm._features_dc, gm._features_rest)
    cx, cr, cs = out[:, 0:3] * 1.0, out[:, 3:7] * 1.0, out[:, 7:10] * 1.0
    assert renderer._fused_deform_rows(gm, cx, cr, cs) is None
    a = renderer.render(cam, gm, pipe, bg, dx, dr, ds)
    ga = _grads(gm, out, a, gt)
    b = renderer.render(cam, gm, pipe, bg, cx, cr, cs)
    gb = _grads(gm, out, b, gt)
    assert int((a["radii"] > 0).sum()) > 500
    torch.testing.assert_close(a["render"], b["render"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(a["depth"], b["depth"], rtol=1e-5, atol=1e-5)
    assert torch.equal(a["radii"], b["radii"])
    for n, x, y in zip(["xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "deform"], ga, gb):
        assert x.shape == y.shape, n
        if y.numel() == 0:  # degree 0: features_rest is (N, 0, 3)
            continue
        scale = y.abs().max().clamp_min(1e-12)
        assert ((x - y).abs().max() / scale) < 2e-4, n


TRAIN_CASES = [
    # id, max degree, active degree at the start, iterations, prune after, oneupSHdegree after
    ("degree1", 1, 1, 6, 3, None),
    ("degree2-oneup", 2, 0, 3, None, 1),  # (M, D) = (9, 0) -> (9, 1) inside one run
]


@pytest.mark.parametrize("name,degree,active,iters,prune_after,oneup_after", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_training_steps_low_degree(name, degree, active, iters, prune_after, oneup_after):
    """A model of sh_degree < 3 cannot take the native step (split-SH needs (P, 15, 3)): train_step runs
    the autograd path, fused input kernels + plain rasterizer. Several steps with Adam (and a prune)
    follow the torch-glue path's (renderer.set_fused(False)) losses to 1e-5 relative and parameters to
    2e-4 in norm, the bars of test_native_step_overflow_redo_and_adam."""
    from deformgs import native_step, renderer
    from deformgs.arguments import OptimizationParams, PipelineParams
    from deformgs.deform_model import DeformModelBaseline
    from deformgs.synthetic import synth_camera
    from deformgs.train_step import optimizer_step, train_step
    from test_gpu_native_step import _params
    dev = torch.device("cuda", 0)
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    cams = [synth_camera(240, 200, index=k, fid=0.1 * k, device=dev) for k in range(3)]
    gts = [torch.rand((3, 200, 240), generator=torch.Generator().manual_seed(k)).to(dev) for k in range(3)]
    runs = {}
    was = renderer._FUSED["on"]
    try:
        for fused in (True, False):
            renderer.set_fused(fused)
            gs = _low_model(6000, degree, 1, active=active, train=True)
            torch.manual_seed(1)
            deform = DeformModelBaseline(is_blender=True, is_6dof=False, device=dev)
            net = deform.deform
            with torch.no_grad():
                for h in (net.gaussian_warp, net.gaussian_rotation, net.gaussian_scaling):
                    h.weight.mul_(0.01)
                    h.bias.mul_(0.01)
            deform.train_setting(OptimizationParams())
            assert not native_step.usable(gs, deform, pipe, gts[0])
            losses = []
            for it in range(iters):
                loss, pkg, _ = train_step(gs, deform, cams[it % 3], gts[it % 3], pipe, bg, False)
                assert int((pkg["radii"] > 0).sum()) > 500
                losses.append(float(loss.detach()))
                optimizer_step(gs, deform, 3000 + it)
                if it == prune_after:
                    keep = torch.ones(gs._xyz.shape[0], dtype=torch.bool, device=dev)
                    keep[::7] = False
                    gs.prune_points(~keep)
                if it == oneup_after:
                    gs.oneupSHdegree()
                    assert gs.active_sh_degree == active + 1
            torch.cuda.synchronize()
            assert getattr(gs, "_dgs_native", None) is None
            runs[fused] = (losses, [p.detach().clone() for p in _params(gs, deform)])
    finally:
        renderer.set_fused(was)
    la, lb = np.array(runs[True][0]), np.array(runs[False][0])
    assert np.all(np.isfinite(la)) and np.all(np.abs(la - lb) <= 1e-5 * np.abs(lb)), (la, lb)
    for a, b in zip(runs[True][1], runs[False][1]):
        assert a.shape == b.shape
        assert float((a - b).norm()) <= 2e-4 * max(float(b.norm()), 1e-30)


def test_render_frames_refuses_low_degree():
    """render_frames() needs the split-SH layout: for a model of sh_degree 1 it raises its documented
    ValueError naming (P,15,3)."""
    from deformgs.render_frames import render_frames
    from deformgs.synthetic import synth_camera
    gm = _low_model(500, 1, 2)
    cam = synth_camera(64, 48, index=0, fid=0.0, device=torch.device("cuda"))
    with pytest.raises(ValueError, match=r"\(P,15,3\)"):
        render_frames([cam], gm, None, torch.zeros(3, device="cuda"))
