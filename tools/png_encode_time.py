#!/usr/bin/env python3
"""PNG writing time and size: --frames RGB frames at --res^2, the rgb8 output of render_frames on the synthetic
scene (--gaussians Gaussians, the deformation heads at 1/100 scale as tools/fps.py), to PNG bytes in host memory.

Legs, medians of --rounds rounds, alternating within a round, each between two device synchronisations:
  host_zlib   today's path: frames.cpu().numpy(), then deformgs.png.encode_png per frame
  device      one deformgs.png_gpu.encode_frames call (filter, deflate and pack kernels, the copy of the
              compressed bytes, the chunk framing and CRC on the host)
Every device file is decoded and compared with its frame before the timing. --profile runs the device leg alone
(three calls) for a kernel trace of the run. Prints one JSON line per leg and a summary line (time ratio, total
bytes of both writers); --out appends them to a file (profiles/png_encode_time.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))

from deformgs import png, png_gpu  # noqa: E402


def render(n_frames, res, n_gaussians, dev):
    from deformgs.deform_model import DeformModelBaseline
    from deformgs.gaussian_model import GaussianModel
    from deformgs.render_frames import render_frames
    from deformgs.synthetic import synth_camera, synth_gaussians
    g = synth_gaussians(n_gaussians, seed=0, device=dev)
    gm = GaussianModel(3)
    gm.from_tensors(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
    torch.manual_seed(0)
    deform = DeformModelBaseline(is_blender=True, is_6dof=False, device=dev)
    with torch.no_grad():
        for head in (deform.deform.gaussian_warp, deform.deform.gaussian_rotation, deform.deform.gaussian_scaling):
            head.weight.mul_(0.01)
            head.bias.mul_(0.01)
    views = [synth_camera(res, res, index=k, fid=k / max(n_frames - 1, 1), device=dev) for k in range(n_frames)]
    return render_frames(views, gm, deform, torch.zeros(3, device=dev), outputs=("rgb8",))["rgb8"]


def host_leg(frames):
    a = frames.cpu().numpy()
    return [png.encode_png(a[i]) for i in range(a.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "png_encode_time.py measures the GPU path: it needs a GPU"
    dev = torch.device("cuda", 0)
    frames = render(args.frames, args.res, args.gaussians, dev)
    torch.cuda.synchronize()
    if args.profile:
        for _ in range(3):
            png_gpu.encode_frames(frames)
        torch.cuda.synchronize()
        return
    files = png_gpu.encode_frames(frames)  # warm-up, and the check
    want = frames.cpu().numpy()
    for i, data in enumerate(files):
        assert np.array_equal(png.decode_png(data), want[i]), f"frame {i} does not decode to its input"
    t = {"host_zlib": [], "device": []}
    old = None
    for _ in range(args.rounds):
        for key, fn in (("host_zlib", host_leg), ("device", png_gpu.encode_frames)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(frames)
            torch.cuda.synchronize()
            t[key].append(time.perf_counter() - t0)
            if key == "host_zlib":
                old = res
    lines = [{"leg": k, "frames": args.frames, "res": args.res, "seconds_median": statistics.median(v), "seconds": v}
             for k, v in t.items()]
    med = {d["leg"]: d["seconds_median"] for d in lines}
    new_bytes, old_bytes = sum(len(f) for f in files), sum(len(f) for f in old)
    lines.append({"summary": "encode_frames vs .cpu().numpy() + encode_png per frame", "frames": args.frames,
                  "res": args.res, "gaussians": args.gaussians, "host_ms_per_frame": 1e3 * med["host_zlib"] / args.frames,
                  "device_ms_per_frame": 1e3 * med["device"] / args.frames, "speedup": med["host_zlib"] / med["device"],
                  "host_bytes": old_bytes, "device_bytes": new_bytes, "size_ratio": new_bytes / old_bytes,
                  "raw_bytes": int(want.nbytes), "device_name": torch.cuda.get_device_name(0)})
    for d in lines:
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
