"""render_frames(): N (camera, time) pairs in, N frames out, through dgs_render_frames (csrc/render.hip).

The forward-only counterpart of render_baseline.py's loops (render_set, interpolate_time / _view / _all /
_poses / _view_original: per frame deform.step(xyz, fid) + render(), render_baseline.py:57-66). One C call
per chunk of frames: the network's inference forward, the render-input glue and the forward-only
rasterizer of every frame are enqueued back to back on torch's current stream, with one host wait per
call instead of one per frame, no autograd context and no backward state. `color` and `depth` are
bitwise those of deform.step + render() under no_grad.
"""
import ctypes
import math

import torch

from . import _lib

OUTPUTS = ("color", "depth", "alpha", "rgb8", "depth8")
_CHUNK_BYTES = 1 << 30  # one chunk's outputs stay under 1 GiB


def _refuse(why):
    raise ValueError(f"render_frames: {why} (the fused render path cannot take this configuration; "
                     "use deform.step + render() per frame)")


def _network(deform):
    """The _DeformBase network of a DeformModel wrapper (or the network itself), None for static Gaussians."""
    if deform is None:
        return None
    from .deform_network import _DeformBase
    net = getattr(deform, "deform", deform)
    if not isinstance(net, _DeformBase):
        _refuse("the deformation model is not a fused DeformNetwork")
    if not net._rotscale:
        _refuse("the network variant without rotation / scaling heads returns deltas the fused input glue does not take")
    return net


def default_chunk(H, W, outputs):
    per = {"color": 12, "depth": 4, "alpha": 4, "rgb8": 3, "depth8": 1}
    return max(1, _CHUNK_BYTES // max(1, H * W * sum(per[o] for o in outputs)))


@torch.no_grad()
def render_frames(views, gaussians, deform, background, times=None, is_6dof=False, scaling_modifier=1.0,
                  outputs=("color",), chunk=None):
    """-> dict of stacked tensors: any of color (F,3,H,W), depth (F,1,H,W), alpha (F,1,H,W) = 1 - final
    transmittance, rgb8 (F,H,W,3) uint8 = the reference's to8b of the colour, depth8 (F,H,W) uint8 = depth /
    (its frame maximum + 1e-5) quantised the same way; plus num_rendered (F,) int32 (CPU: every frame's
    tile-pair count) and redone (int: frames re-rendered because their pair count exceeded the learned
    capacity). views: Camera / MiniCam objects of one image size; times (F floats or a tensor) overrides
    view.fid per frame; deform=None renders the static Gaussians. chunk bounds the frames per C call."""
    from diff_gaussian_rasterization import split_sh_ok
    from .renderer import _FUSED, _HONOR_OVERRIDE, _SPLIT_SH, _fused_ok
    outputs = tuple(outputs)
    if not outputs or any(o not in OUTPUTS for o in outputs):
        raise ValueError(f"render_frames: outputs must be a non-empty subset of {OUTPUTS}, got {outputs}")
    pc = gaussians
    if not _fused_ok(pc):
        _refuse("the Gaussian parameters must be contiguous fp32 device tensors with the reference's activations")
    if not (split_sh_ok(pc._features_dc, pc._features_rest)):
        _refuse("features_dc / features_rest must be (P,1,3) / (P,15,3), contiguous and 16-byte aligned")
    if not (_FUSED["on"] and _SPLIT_SH) or _HONOR_OVERRIDE["on"]:
        _refuse("the fused render inputs / split-SH rasterizer are switched off")
    net = _network(deform)
    if net is not None and bool(is_6dof) != bool(net.is_6dof):
        _refuse("is_6dof does not match the network's head")
    views = list(views)
    F = len(views)
    dev = pc._xyz.device
    lib = _lib.load()
    P = pc._xyz.shape[0]
    if F:
        H, W = int(views[0].image_height), int(views[0].image_width)
        if any(int(v.image_height) != H or int(v.image_width) != W for v in views):
            _refuse("every view of one call must have the same image size")
    else:
        H = W = 0
    if times is None:
        t = (torch.cat([v.fid.reshape(1).to(dev, torch.float32) for v in views]) if F
             else torch.empty((0,), dtype=torch.float32, device=dev))
    else:
        t = torch.as_tensor(times, dtype=torch.float32).reshape(-1).to(dev)
        if t.numel() != F:
            raise ValueError(f"render_frames: {t.numel()} times for {F} views")
    e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)  # noqa: E731
    out = {}
    if "color" in outputs:
        out["color"] = e(F, 3, H, W)
    if "depth" in outputs:
        out["depth"] = e(F, 1, H, W)
    if "alpha" in outputs:
        out["alpha"] = e(F, 1, H, W)
    if "rgb8" in outputs:
        out["rgb8"] = u8(F, H, W, 3)
    if "depth8" in outputs:
        out["depth8"] = u8(F, H, W)
    nr = (ctypes.c_int * max(F, 1))()
    redone_total = 0
    if F:
        a = _lib.RenderFramesArgs()
        a.P = P
        a.xyz, a.f_dc, a.f_rest = pc._xyz.data_ptr(), pc._features_dc.data_ptr(), pc._features_rest.data_ptr()
        a.scaling, a.rotation, a.opacity = pc._scaling.data_ptr(), pc._rotation.data_ptr(), pc._opacity.data_ptr()
        stream = _lib.stream_ptr(dev)
        keep = []
        if net is not None:
            from .deform_network import FLAG_EXACT_FP32, FLAG_UNIFORM_T
            flags = net.flags | (FLAG_EXACT_FP32 if net.exact_fp32 else 0)
            # packed once per call (the layout of the flags the frames run with), not per frame
            packed = e(lib.dgs_deform_packed_floats(flags | FLAG_UNIFORM_T))
            params = [p.detach().contiguous() for p in net.kernel_params()]
            _lib.check(lib.dgs_deform_pack(flags | FLAG_UNIFORM_T, _lib.ptr_array(params), _lib.ptr(packed), stream),
                       "deform_pack")
            mlp_out, t_full = e(max(P, 1), lib.dgs_deform_outputs(flags)), e(max(P, 1))
            keep += [packed, params, mlp_out, t_full]
            a.deform, a.mlp_flags, a.mlp_packed = 1, flags, packed.data_ptr()
            a.mlp_out, a.t_full = mlp_out.data_ptr(), t_full.data_ptr()
        scratch = [e(max(P, 1), 3), e(max(P, 1), 3), e(max(P, 1), 4), e(max(P, 1), 1)]
        a.means3D, a.scales, a.rotations, a.opacities = (s.data_ptr() for s in scratch)
        a.H, a.W, a.sh_degree, a.scale_modifier = H, W, int(pc.active_sh_degree), float(scaling_modifier)
        bg = background.to(dev, torch.float32).contiguous()
        a.bg = bg.data_ptr()
        frames = (_lib.Frame * F)()
        for f, v in enumerate(views):
            mats = [m if (m.is_contiguous() and m.dtype == torch.float32 and m.device == dev)
                    else m.to(dev, torch.float32).contiguous()
                    for m in (v.world_view_transform, v.full_proj_transform, v.camera_center)]
            keep.append(mats)
            fr = frames[f]
            fr.viewmatrix, fr.projmatrix, fr.campos = (m.data_ptr() for m in mats)
            fr.tanfovx, fr.tanfovy = math.tan(v.FoVx * 0.5), math.tan(v.FoVy * 0.5)
        n = int(chunk) if chunk else default_chunk(H, W, outputs)
        if n < 1:
            raise ValueError("render_frames: chunk must be >= 1")
        for f0 in range(0, F, n):
            nf = min(n, F - f0)
            a.F = nf
            a.frames = ctypes.cast(ctypes.byref(frames, f0 * ctypes.sizeof(_lib.Frame)), ctypes.POINTER(_lib.Frame))
            a.t = t.data_ptr() + 4 * f0
            for name in OUTPUTS:
                setattr(a, "out_" + name, out[name][f0:].data_ptr() if name in out else None)
            a.num_rendered = ctypes.cast(ctypes.byref(nr, 4 * f0), ctypes.POINTER(ctypes.c_int))
            redone = ctypes.c_int(0)
            _lib.check(lib.dgs_render_frames(ctypes.byref(a), ctypes.byref(redone), stream), "render_frames")
            redone_total += redone.value
        # the scratch / camera tensors go back to torch's caching allocator, which hands them out again in
        # the order of this same stream
        del keep
    out["num_rendered"] = torch.tensor(list(nr)[:F], dtype=torch.int32)
    out["redone"] = redone_total
    return out
