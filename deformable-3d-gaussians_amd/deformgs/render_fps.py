"""Inference FPS loop of render_baseline.render_set (render_baseline.py:57-74): per view, deform.step
+ render() between two device synchronisations, FPS = 1 / mean(t[skip:]). No image I/O (the
reference's first loop, which writes PNGs, is not timed there either).

batched=True times the same views through render_frames (one dgs_render_frames call: every frame enqueued
back to back, one host wait per call) between one device synchronisation before the call and one after:
FPS = frames / elapsed, the first `skip` frames rendered in an untimed warm-up call."""
import time

import numpy as np
import torch

from .renderer import render


@torch.no_grad()
def measure_fps(views, gaussians, pipeline, background, deform, is_6dof=False, skip=5, repeat=1, batched=False):
    if batched:
        from .render_frames import render_frames
        if any(getattr(pipeline, k, False) for k in ("compute_cov3D_python", "convert_SHs_python", "debug")):
            raise ValueError("measure_fps(batched=True): render_frames takes the fused render path only "
                             "(no compute_cov3D_python / convert_SHs_python / debug pipeline switches)")
        views = list(views) * repeat
        if skip:
            render_frames(views[:skip], gaussians, deform, background, is_6dof=is_6dof)
        timed = views[skip:]
        torch.cuda.synchronize()
        t0 = time.time()
        render_frames(timed, gaussians, deform, background, is_6dof=is_6dof)
        torch.cuda.synchronize()
        return len(timed) / (time.time() - t0), len(timed)
    t_list = []
    for _ in range(repeat):
        for view in views:
            xyz = gaussians.get_xyz
            time_input = view.fid.unsqueeze(0).expand(xyz.shape[0], -1)
            torch.cuda.synchronize()
            t0 = time.time()
            d_xyz, d_rotation, d_scaling = deform.step(xyz.detach(), time_input)
            render(view, gaussians, pipeline, background, d_xyz, d_rotation, d_scaling, is_6dof)
            torch.cuda.synchronize()
            t_list.append(time.time() - t0)
    t = np.array(t_list[skip:])
    return 1.0 / t.mean(), len(t)
