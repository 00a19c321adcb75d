"""render_frames (dgs_render_frames: forward-only frame renderer) against the per-frame path
deform.step + render() under no_grad, on the small scene of tests/render_frames_scene.py.

Bitwise checks carry no tolerance: the blend order is fixed by the sorted tile lists, the network and
glue kernels are the per-frame path's own, and k_blend_img keeps k_blend_fwd's arithmetic."""
import ctypes
import functools

import pytest
import torch

import render_frames_scene as S
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

VARIANTS = {
    # name: (sh_degree, is_blender, is_6dof, has_network, background)
    "sh3": (3, True, False, True, (0.0, 0.0, 0.0)),
    "sh0": (0, True, False, True, (0.0, 0.0, 0.0)),
    "nonblender": (3, False, False, True, (0.0, 0.0, 0.0)),
    "6dof": (3, True, True, True, (0.0, 0.0, 0.0)),
    "static": (3, True, False, False, (0.0, 0.0, 0.0)),
    "white": (3, True, False, True, (1.0, 1.0, 1.0)),
}


def _per_frame(gm, deform, cam, bg, six, t=None):
    """The parent's code path for one frame -> (color, depth, pair count). The count comes from the split-SH
    forward called on the same render inputs (render() does not return it); its image must be render()'s."""
    from deformgs.arguments import PipelineParams
    from deformgs.renderer import _GaussianInputs, render
    from diff_gaussian_rasterization import _RasterizeGaussiansSplitSH, GaussianRasterizationSettings
    import math
    n = gm.get_xyz.shape[0]
    with torch.no_grad():
        fid = cam.fid if t is None else torch.tensor([t], dtype=torch.float32, device="cuda")
        if deform is None:
            d = (0.0, 0.0, 0.0)
        else:
            d = deform.step(gm.get_xyz.detach(), fid.unsqueeze(0).expand(n, -1))
        pkg = render(cam, gm, PipelineParams(), bg, d[0], d[1], d[2], six)
        rows = None if deform is None else (d[0]._dgs_se3_raw if six else d[0]._base)
        m3, _, op, sc, ro = _GaussianInputs.apply(gm._xyz, gm._features_dc, gm._features_rest, gm._scaling, gm._rotation,
                                                  gm._opacity, rows, six and deform is not None, False)
        rs = GaussianRasterizationSettings(
            image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=gm.active_sh_degree, campos=cam.camera_center,
            prefiltered=False, debug=False)

        class Ctx:  # the attributes the autograd function's forward sets
            def save_for_backward(self, *a):
                pass

            def mark_non_differentiable(self, *a):
                pass

            def set_materialize_grads(self, v):
                pass

        ctx = Ctx()
        color2, _, _, _ = _RasterizeGaussiansSplitSH.forward(ctx, m3, None, None, gm._features_dc, gm._features_rest, op,
                                                            sc, ro, rs)
        ctx.raster.free()
        assert torch.equal(color2, pkg["render"])
    return pkg["render"], pkg["depth"], ctx.num_rendered


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gm, deform, cams, bg, six, reference colour (F,3,H,W), depth (F,1,H,W), pair counts) per variant, computed
    once and left unchanged."""
    sh, blender, six, has_net, bgc = VARIANTS[name]
    gm = S.gaussians(sh_degree=sh)
    deform = S.network(is_blender=blender, is_6dof=six) if has_net else None
    cams = S.cameras()
    bg = torch.tensor(bgc, dtype=torch.float32, device="cuda")
    ref = [_per_frame(gm, deform, c, bg, six) for c in cams]
    color = torch.stack([r[0] for r in ref])
    depth = torch.stack([r[1] for r in ref])
    return gm, deform, cams, bg, six, color, depth, [r[2] for r in ref]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_parity_bitwise(name):
    from deformgs.render_frames import render_frames
    gm, deform, cams, bg, six, color, depth, nr = _case(name)
    print("per-frame pair counts", nr)
    # some tile list spans several 256-entry batches
    assert max(nr) > 256 * 35
    out = render_frames(cams, gm, deform, bg, is_6dof=six, outputs=("color", "depth"))
    print("render_frames pair counts", out["num_rendered"].tolist(), "redone", out["redone"])
    assert out["num_rendered"].tolist() == nr
    assert torch.equal(out["color"], color)
    assert torch.equal(out["depth"], depth)


def test_times_override_view_fid():
    from deformgs.render_frames import render_frames
    gm, deform, cams, bg, six, _, _, _ = _case("sh3")
    times = [0.9 - 0.1 * k for k in range(S.F)]
    out = render_frames(cams, gm, deform, bg, times=times, outputs=("color",))
    for k in (0, S.F - 1):
        ref, _, nr = _per_frame(gm, deform, cams[k], bg, False, t=times[k])
        assert torch.equal(out["color"][k], ref)
        assert int(out["num_rendered"][k]) == nr


def test_overflow_redo():
    from deformgs import _lib
    from deformgs.render_frames import render_frames
    lib = _lib.load()
    gm, deform, cams, bg, six, color, depth, nr = _case("sh3")
    dev = torch.cuda.current_device()
    before = lib.dgs_debug_pair_cap(dev)
    try:
        # (the call feeds its counts to the learned capacity only after its wait: every frame is binned for 64)
        lib.dgs_debug_set_pair_cap(dev, 64)
        out = render_frames(cams, gm, deform, bg, outputs=("color", "depth", "depth8"))
    finally:
        lib.dgs_debug_set_pair_cap(dev, before)
    assert out["redone"] == S.F
    assert out["num_rendered"].tolist() == nr
    assert torch.equal(out["color"], color)
    assert torch.equal(out["depth"], depth)
    assert torch.equal(out["depth8"], _depth8(depth))


def test_sort_binning_path():
    """The duplicate + tile-key radix sort binning (dgs_debug_set_binning(1); taken by images past the rect
    binning's tile / cell limits): per-frame counts through the copy to the frame's host word, speculative
    frames and redone ones. The tile lists are those of the rect binning, so the reference is unchanged."""
    import os
    from deformgs import _lib
    from deformgs.render_frames import render_frames
    lib = _lib.load()
    gm, deform, cams, bg, six, color, depth, nr = _case("sh3")
    dev = torch.cuda.current_device()
    before = lib.dgs_debug_pair_cap(dev)
    default = 1 if os.environ.get("DGS_BINNING") == "sort" else 0
    try:
        lib.dgs_debug_set_binning(1)
        a = render_frames(cams, gm, deform, bg, outputs=("color", "depth"))
        lib.dgs_debug_set_pair_cap(dev, 64)
        b = render_frames(cams, gm, deform, bg, outputs=("color", "depth"))
        lib.dgs_debug_set_pair_cap(dev, 0)  # no learned capacity: the first frame waits for its own count
        c = render_frames(cams, gm, deform, bg, outputs=("color", "depth"))
    finally:
        lib.dgs_debug_set_binning(default)
        lib.dgs_debug_set_pair_cap(dev, before)
    assert b["redone"] == S.F and c["redone"] == 0
    for o in (a, b, c):
        assert o["num_rendered"].tolist() == nr
        assert torch.equal(o["color"], color) and torch.equal(o["depth"], depth)


@pytest.mark.parametrize("tile_sort", [1, 0])
@pytest.mark.parametrize("binning", ["rect", "sort"])
def test_shared_stages_both_callers(binning, tile_sort):
    """The frame-setup stages the training forward and render_frames share (geometry / rect carve, global depth
    order, pair count), on the paths the default binning does not reach: sort binning, and rect binning over the
    global depth order (tile sort off). 300 Gaussians (two 256-thread blocks, the second ragged) on a 48 x 40
    image (3 x 3 tiles, ragged right and bottom), two (camera, time) frames; both callers run under the same
    toggles, so the comparison is bitwise."""
    import os
    from deformgs import _lib
    from deformgs.render_frames import render_frames
    lib = _lib.load()
    gm, deform = S.gaussians(n=300), S.network()
    cams = S.cameras(2, width=48, height=40)
    bg = torch.zeros(3, device="cuda")
    default = 1 if os.environ.get("DGS_BINNING") == "sort" else 0
    ts_before = lib.dgs_debug_get_tile_sort()
    try:
        lib.dgs_debug_set_binning(1 if binning == "sort" else 0)
        lib.dgs_debug_set_tile_sort(tile_sort)
        ref = [_per_frame(gm, deform, c, bg, False) for c in cams]
        out = render_frames(cams, gm, deform, bg, outputs=("color", "depth"))
    finally:
        lib.dgs_debug_set_binning(default)
        lib.dgs_debug_set_tile_sort(ts_before)
    nr = [r[2] for r in ref]
    print("pair counts: per-frame", nr, "render_frames", out["num_rendered"].tolist(), "redone", out["redone"])
    assert min(nr) > 0
    assert out["num_rendered"].tolist() == nr
    assert torch.equal(out["color"], torch.stack([r[0] for r in ref]))
    assert torch.equal(out["depth"], torch.stack([r[1] for r in ref]))


def test_one_host_wait():
    from deformgs import _lib
    from deformgs.render_frames import render_frames
    lib = _lib.load()
    gm, deform, cams, bg, six, color, _, _ = _case("sh3")
    render_frames(cams, gm, deform, bg)  # learns the capacity
    w0, w1 = ctypes.c_longlong(0), ctypes.c_longlong(0)
    lib.dgs_debug_count_wait_ns(ctypes.byref(w0))
    out = render_frames(cams, gm, deform, bg)
    lib.dgs_debug_count_wait_ns(ctypes.byref(w1))
    print("host waits of one 6-frame call:", w1.value - w0.value)
    assert out["redone"] == 0
    assert w1.value - w0.value <= 1
    assert torch.equal(out["color"], color)


def _rgb8(color):
    return (255 * color.clamp(0, 1)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _depth8(depth):
    d = torch.stack([x / (x.amax() + 1e-5) for x in depth])
    return (255 * d.clamp(0, 1)).to(torch.uint8)[:, 0].contiguous()


def test_derived_outputs():
    from deformgs.cameras import orbit_camera
    from deformgs.render_frames import render_frames
    from deformgs.synthetic import DNERF_FOV
    gm, deform, cams, _, six, _, _, _ = _case("sh3")
    # one more view from far away, so that pixels exist which no Gaussian reaches
    cams = cams + [orbit_camera(0.3, 0.2, 9.0, DNERF_FOV, S.W, S.H, fid=0.5, data_device="cuda")]
    white = torch.ones(3, device="cuda")
    black = torch.zeros(3, device="cuda")
    every = ("color", "depth", "alpha", "rgb8", "depth8")
    ow = render_frames(cams, gm, deform, white, outputs=every)
    ob = render_frames(cams, gm, deform, black, outputs=every)
    for o in (ow, ob):
        assert torch.equal(o["rgb8"], _rgb8(o["color"]))
        assert torch.equal(o["depth8"], _depth8(o["depth"]))
    assert torch.equal(ow["alpha"], ob["alpha"]) and torch.equal(ow["depth"], ob["depth"])
    err = ((ow["color"] - ob["color"]) - (1.0 - ob["alpha"])).abs().max().item()
    print("max |white - black - (1 - alpha)|:", err)
    assert err <= 2e-6
    empty = ob["depth"][-1, 0] == 0  # a contributing Gaussian adds depth > 0.2 * alpha * T > 0
    assert empty.any()
    assert (ob["alpha"][-1, 0][empty] == 0).all()
    # odd image width: the byte-store variants of rgb8 / depth8
    odd = S.cameras(2, width=99, height=70)
    oo = render_frames(odd, gm, deform, white, outputs=every)
    assert torch.equal(oo["rgb8"], _rgb8(oo["color"])) and torch.equal(oo["depth8"], _depth8(oo["depth"]))
    only8 = render_frames(odd, gm, deform, white, outputs=("rgb8", "depth8"))
    assert torch.equal(only8["rgb8"], oo["rgb8"]) and torch.equal(only8["depth8"], oo["depth8"])


def test_edges():
    from deformgs.cameras import orbit_camera
    from deformgs.render_frames import render_frames
    from deformgs.synthetic import DNERF_FOV
    gm, deform, cams, bg, six, color, depth, nr = _case("sh3")
    # F = 0
    o = render_frames([], gm, deform, bg, outputs=("color", "rgb8"))
    assert o["color"].shape[0] == 0 and o["rgb8"].shape[0] == 0 and o["num_rendered"].numel() == 0 and o["redone"] == 0
    # P = 0: every frame is the background
    empty = S.gaussians(n=0)
    bgc = torch.tensor([0.25, 0.5, 0.75], device="cuda")
    o = render_frames(cams[:2], empty, deform, bgc, outputs=("color", "depth", "alpha", "rgb8", "depth8"))
    assert torch.equal(o["color"], bgc.view(1, 3, 1, 1).expand(2, 3, S.H, S.W))
    assert not o["depth"].any() and not o["alpha"].any() and not o["depth8"].any()
    assert torch.equal(o["rgb8"], _rgb8(o["color"])) and o["num_rendered"].tolist() == [0, 0]
    # a camera facing away: every Gaussian culled
    away = orbit_camera(0.0, 0.0, 4.0, DNERF_FOV, S.W, S.H, fid=0.5, data_device="cuda")
    flip = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0], device="cuda"))  # half a turn about the camera's y axis
    away.world_view_transform = (away.world_view_transform @ flip).contiguous()
    away.full_proj_transform = (away.world_view_transform @ away.projection_matrix).contiguous()
    o = render_frames([away], gm, deform, bgc, outputs=("color", "alpha"))
    assert o["num_rendered"].tolist() == [0]
    assert torch.equal(o["color"], bgc.view(1, 3, 1, 1).expand(1, 3, S.H, S.W)) and not o["alpha"].any()
    # a 16 x 16 image (one tile)
    small = S.cameras(2, width=16, height=16)
    o = render_frames(small, gm, deform, bg, outputs=("color", "depth"))
    for k, c in enumerate(small):
        rc, rd, rn = _per_frame(gm, deform, c, bg, False)
        assert torch.equal(o["color"][k], rc) and torch.equal(o["depth"][k], rd) and int(o["num_rendered"][k]) == rn
    # chunk = 1 equals chunk = None
    a = render_frames(cams, gm, deform, bg, outputs=("color", "depth", "rgb8", "depth8"), chunk=1)
    assert torch.equal(a["color"], color) and torch.equal(a["depth"], depth) and a["num_rendered"].tolist() == nr
    b = render_frames(cams, gm, deform, bg, outputs=("rgb8", "depth8"))
    assert torch.equal(a["rgb8"], b["rgb8"]) and torch.equal(a["depth8"], b["depth8"])


def test_training_path_untouched(monkeypatch):
    """A forward_backward step gives the same loss and gradients, bitwise in the deterministic mode, whether or
    not a render_frames call ran on the model before it."""
    from deformgs.arguments import PipelineParams
    from deformgs.render_frames import render_frames
    from deformgs.renderer import set_deterministic
    from deformgs.train_step import forward_backward
    monkeypatch.setenv("DGS_DETERMINISTIC", "1")
    prev = set_deterministic(True)
    try:
        cams = S.cameras()
        bg = torch.zeros(3, device="cuda")
        gt = torch.rand(3, S.H, S.W, generator=torch.Generator().manual_seed(3)).cuda()

        def step(with_render):
            gm = S.gaussians()
            deform = S.network()
            if with_render:
                render_frames(cams, gm, deform, bg, outputs=("color", "rgb8", "depth8"))
            loss, _ = forward_backward(gm, deform, cams[1], gt, PipelineParams(), bg)
            ps = [gm._xyz, gm._features_dc, gm._features_rest, gm._scaling, gm._rotation, gm._opacity]
            ps += list(deform.deform.parameters())
            return loss.detach().clone(), [p.grad.detach().clone() for p in ps]

        l0, g0 = step(False)
        l1, g1 = step(True)
        assert torch.equal(l0, l1)
        assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    finally:
        set_deterministic(prev)


def _args(gm, cams, bg, outs):
    """A valid static-Gaussian argument block for ctypes-level calls; returns (args, keepalive)."""
    import math
    from deformgs import _lib
    n = gm._xyz.shape[0]
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")  # noqa: E731
    keep = [e(n, 3), e(n, 3), e(n, 4), e(n, 1)]
    a = _lib.RenderFramesArgs()
    a.P = n
    a.xyz, a.f_dc, a.f_rest = gm._xyz.data_ptr(), gm._features_dc.data_ptr(), gm._features_rest.data_ptr()
    a.scaling, a.rotation, a.opacity = gm._scaling.data_ptr(), gm._rotation.data_ptr(), gm._opacity.data_ptr()
    a.means3D, a.scales, a.rotations, a.opacities = (k.data_ptr() for k in keep)
    a.H, a.W, a.sh_degree, a.scale_modifier, a.bg = S.H, S.W, 3, 1.0, bg.data_ptr()
    frames = (_lib.Frame * len(cams))()
    for f, c in enumerate(cams):
        frames[f].viewmatrix, frames[f].projmatrix = c.world_view_transform.data_ptr(), c.full_proj_transform.data_ptr()
        frames[f].campos = c.camera_center.data_ptr()
        frames[f].tanfovx, frames[f].tanfovy = math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5)
    a.F, a.frames = len(cams), frames
    for k, v in outs.items():
        setattr(a, k, v.data_ptr())
    return a, keep + [frames]


def test_errors():
    from deformgs import _lib
    from deformgs.render_frames import render_frames
    lib = _lib.load()
    gm, deform, cams, bg, six, color, _, _ = _case("sh3")
    stream = _lib.stream_ptr(torch.device("cuda"))
    img = torch.empty(2, 3, S.H, S.W, device="cuda")

    def call(a):
        rc = lib.dgs_render_frames(ctypes.byref(a), None, stream)
        return rc, lib.dgs_last_error().decode()

    a, keep = _args(gm, cams[:2], bg, {"out_color": img})
    assert call(a)[0] == 0  # the block itself is valid
    torch.cuda.synchronize()
    assert torch.equal(img, _case("static")[5][:2])
    a, keep = _args(gm, cams[:2], bg, {})
    rc, msg = call(a)
    assert rc == -1 and "output" in msg
    a, keep = _args(gm, cams[:2], bg, {"out_color": img})
    a.f_rest = gm._features_rest.data_ptr() + 4
    rc, msg = call(a)
    assert rc == -1 and "aligned" in msg
    a, keep = _args(gm, cams[:2], bg, {"out_color": img})
    a.sh_degree = 4
    rc, msg = call(a)
    assert rc == -1 and "SH degree" in msg
    # the non-blender network's kernels read a column of P times: t_full is required
    a, keep = _args(gm, cams[:2], bg, {"out_color": img})
    from deformgs.deform_network import FLAG_UNIFORM_T
    flags = 0
    packed = torch.zeros(lib.dgs_deform_packed_floats(flags | FLAG_UNIFORM_T), device="cuda")
    t = torch.zeros(2, device="cuda")
    mlp_out = torch.empty(S.N, lib.dgs_deform_outputs(flags), device="cuda")
    a.deform, a.mlp_flags, a.mlp_packed, a.t, a.mlp_out = 1, flags, packed.data_ptr(), t.data_ptr(), mlp_out.data_ptr()
    rc, msg = call(a)
    assert rc == -1 and "t_full" in msg
    # Python: a non-contiguous parameter tensor is refused, not rendered some other way
    bad = S.gaussians()
    bad._scaling = torch.nn.Parameter(torch.empty(3, S.N, device="cuda").t())
    assert not bad._scaling.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        render_frames(cams, bad, deform, bg)
    with pytest.raises(ValueError, match="outputs"):
        render_frames(cams, gm, deform, bg, outputs=("normals",))
