#!/usr/bin/env python3
"""JPEG writing time and size: --frames RGB frames at --res^2, the rgb8 output of render_frames on the synthetic
scene (--gaussians Gaussians, the deformation heads at 1/100 scale as tools/fps.py), to JPEG files in host memory at
--quality and --subsampling: what render_cli --video mjpeg spends per chunk before the container.

Legs, medians of --rounds rounds, alternating within a round, each between two device synchronisations:
  device      one deformgs.jpeg_gpu.encode_frames call (transform, entropy twice, scan; the copy of the compressed
              bytes and the framing on the host)
  png_gpu     one deformgs.png_gpu.encode_frames call on the same frames, for scale
  host_pil    frames.cpu().numpy(), then PIL's Image.save(format="JPEG", optimize=False) per frame: only where PIL
              is installed; otherwise the absolute times of the other two legs are all there is
The first device file is decoded by the device decoder (deformgs.ingest) and every one by PIL where installed, and
where PIL is installed its decoded pixels must equal those of PIL's own file. --profile runs the device leg alone
(three calls) for a kernel trace. Prints one JSON line per leg and a summary line; --out appends them to a file
(profiles/jpeg_encode_time.jsonl)."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deformgs import ingest, jpeg_gpu, png_gpu  # noqa: E402
from png_encode_time import render  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None

_PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", default="4:2:0", choices=list(_PIL_SUBSAMPLING))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_encode_time.py measures the GPU path: it needs a GPU"
    dev = torch.device("cuda", 0)
    frames = render(args.frames, args.res, args.gaussians, dev)
    torch.cuda.synchronize()

    def device_leg(f):
        return jpeg_gpu.encode_frames(f, quality=args.quality, subsampling=args.subsampling)

    def host_leg(f):
        a, out = f.cpu().numpy(), []
        for i in range(a.shape[0]):
            b = io.BytesIO()
            Image.fromarray(a[i]).save(b, format="JPEG", quality=args.quality, optimize=False,
                                       subsampling=_PIL_SUBSAMPLING[args.subsampling])
            out.append(b.getvalue())
        return out

    if args.profile:
        for _ in range(3):
            device_leg(frames)
        torch.cuda.synchronize()
        return
    files = device_leg(frames)  # warm-up, and the check
    png_gpu.encode_frames(frames)
    got0 = ingest.ingest_images(files[:1], False, device=dev, return_uint8=True)[1][0].cpu().numpy()
    assert got0.shape == tuple(frames.shape[1:])
    err = np.abs(got0.astype(np.int32) - frames[0].cpu().numpy().astype(np.int32))
    pil_equal = None
    if Image is not None:
        theirs = host_leg(frames)
        pil_equal = all(np.array_equal(np.asarray(Image.open(io.BytesIO(a))), np.asarray(Image.open(io.BytesIO(b))))
                        for a, b in zip(files, theirs))
        assert pil_equal, "a device file does not decode to the pixels of PIL's own file"
    legs = [("device", device_leg), ("png_gpu", png_gpu.encode_frames)] + ([("host_pil", host_leg)] if Image else [])
    t = {k: [] for k, _ in legs}
    sizes = {}
    for _ in range(args.rounds):
        for key, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(frames)
            torch.cuda.synchronize()
            t[key].append(time.perf_counter() - t0)
            sizes[key] = sum(len(f) for f in res)
    lines = [{"leg": k, "frames": args.frames, "res": args.res, "seconds_median": statistics.median(v), "seconds": v,
              "bytes": sizes[k]} for k, v in t.items()]
    med = {d["leg"]: d["seconds_median"] for d in lines}
    summary = {"summary": "jpeg_gpu.encode_frames" + (" vs .cpu().numpy() + PIL save per frame" if Image else
                                                       " (PIL is not installed: absolute times only)"),
               "frames": args.frames, "res": args.res, "gaussians": args.gaussians, "quality": args.quality,
               "subsampling": args.subsampling, "device_ms_per_frame": 1e3 * med["device"] / args.frames,
               "png_gpu_ms_per_frame": 1e3 * med["png_gpu"] / args.frames, "device_bytes": sizes["device"],
               "png_gpu_bytes": sizes["png_gpu"], "raw_bytes": int(frames.numel()),
               "frame0_max_abs_error": int(err.max()), "frame0_mean_abs_error": float(err.mean()),
               "decodes_as_pils_file": pil_equal, "device_name": torch.cuda.get_device_name(0)}
    if Image:
        summary.update(host_pil_ms_per_frame=1e3 * med["host_pil"] / args.frames, speedup=med["host_pil"] / med["device"],
                       host_pil_bytes=sizes["host_pil"])
    lines.append(summary)
    for d in lines:
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
