#!/usr/bin/env python3
"""Inference FPS, per-frame path against render_frames, in one session (profiles/render_frames_fps.jsonl).

The README's configurations (synthetic scenes sized like the D-NeRF table of the reference's README:
15 733 / 55 622 / 78 624 Gaussians at 400x400, plus synth-100k at 800x800; blender network with the heads
at 1/100 scale, 30 views). Per configuration the two paths alternate, three runs each, after one untimed
run of each: measure_fps(...) is the per-frame loop (deform.step + render() between two device
synchronisations per view, FPS = 1 / mean of the per-view times after the first 5), measure_fps(...,
batched=True) one render_frames call over the same views (frames / elapsed, first 5 in a warm-up call).
One JSON line per run: {"commit", "config", "gaussians", "res", "path", "run", "fps", "frames"}; then per
configuration a line with the rasterizer kernel-class times of one render_frames call (timing hooks).

    python tools/render_fps_ab.py --commit $(git rev-parse --short HEAD) --out profiles/render_frames_fps.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))

import torch  # noqa: E402

CONFIGS = [("hell", 15733, 400), ("bouncing", 55622, 400), ("trex", 78624, 400), ("synth-100k", 100000, 800)]
CLASSES = ("mlp_fwd", "inputs_fwd", "preprocess_img", "count", "scan", "place", "tile_sort", "blend_img", "depth8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from deformgs import _lib
    from deformgs.arguments import PipelineParams
    from deformgs.deform_model import DeformModelBaseline
    from deformgs.gaussian_model import GaussianModel
    from deformgs.render_fps import measure_fps
    from deformgs.render_frames import render_frames
    from deformgs.synthetic import synth_camera, synth_gaussians
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name, n, res in CONFIGS:
        g = synth_gaussians(n, seed=0, device=dev)
        gm = GaussianModel(3)
        gm.from_tensors(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
        torch.manual_seed(0)
        deform = DeformModelBaseline(is_blender=True, is_6dof=False, device=dev)
        with torch.no_grad():
            for head in (deform.deform.gaussian_warp, deform.deform.gaussian_rotation, deform.deform.gaussian_scaling):
                head.weight.mul_(0.01)
                head.bias.mul_(0.01)
        views = [synth_camera(res, res, index=k, fid=k / args.views, device=dev) for k in range(args.views)]
        bg = torch.zeros(3, device=dev)
        pipe = PipelineParams()
        base = {"commit": args.commit, "config": name, "gaussians": n, "res": res}
        for run in range(-1, args.runs):  # run -1: untimed warm-up of both paths
            for path in ("per_frame", "batched"):
                fps, nt = measure_fps(views, gm, pipe, bg, deform, batched=(path == "batched"))
                if run >= 0:
                    emit({**base, "path": path, "run": run, "fps": round(fps, 1), "frames": nt})
        lib.dgs_timing_reset()
        lib.dgs_timing_enable(1)
        render_frames(views, gm, deform, bg)
        torch.cuda.synchronize()
        lib.dgs_timing_enable(0)
        cls = {}
        for c in CLASSES:
            k = ctypes.c_int(0)
            ms = lib.dgs_timing_query(c.encode(), ctypes.byref(k))
            if k.value:
                cls[c] = round(1e3 * ms / k.value, 1)
        emit({**base, "path": "batched", "kernel_class_us_per_frame": cls})


if __name__ == "__main__":
    main()
