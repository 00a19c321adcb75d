"""Scoring time of a rendered test set: --frames frame pairs at --res^2 (30 at 800^2: a D-NeRF test split), on the device.

Timed, medians of --rounds rounds, the legs alternating within a round, each leg --reps times per round (a host
clock around work that ends in a host read of the scores):
  per_view        the loop deformgs.metrics.evaluate() runs: float(fused_ssim(r, g)) and float(psnr(r, g)) per view
  batched         one deformgs.image_metrics call for PSNR + SSIM over the same list of frames, one host read
  ms_ssim         one image_metrics call for MS-SSIM alone, one host read
The frames are a seeded smooth pattern + noise (gt) and gt + smaller noise (render); the legs' scores are compared
before anything is timed. Prints one JSON line per leg and a summary; --out appends them to a file
(profiles/image_metrics_time.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))

from deformgs.image_metrics import image_metrics  # noqa: E402
from deformgs.loss import psnr  # noqa: E402
from deformgs.metrics import fused_ssim  # noqa: E402


def make_frames(n, res, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(res, device=dev, dtype=torch.float32),
                            torch.arange(res, device=dev, dtype=torch.float32), indexing="ij")
    renders, gts = [], []
    for i in range(n):
        smooth = torch.stack([0.5 + 0.3 * torch.sin(0.02 * (c + 1) * xx + 0.1 * i) * torch.cos(0.015 * (c + 2) * yy)
                              for c in range(3)])
        gt = (smooth + 0.08 * torch.randn(smooth.shape, device=dev, generator=gen)).clamp(0, 1)
        renders.append((gt + 0.02 * torch.randn(smooth.shape, device=dev, generator=gen)).clamp(0, 1).unsqueeze(0))
        gts.append(gt.unsqueeze(0))
    return renders, gts


def per_view(renders, gts):
    ssims = [float(fused_ssim(r, g)) for r, g in zip(renders, gts)]
    psnrs = [float(psnr(r, g)) for r, g in zip(renders, gts)]
    return ssims, psnrs


def batched(renders, gts):
    m = image_metrics(renders, gts, ("psnr", "ssim"))
    return m["ssim"].tolist(), m["psnr"].tolist()


def ms_only(renders, gts):
    return image_metrics(renders, gts, ("ms_ssim",))["ms_ssim"].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "image_metrics_time.py measures the GPU path: it needs a GPU"
    dev = torch.device("cuda", 0)
    renders, gts = make_frames(args.frames, args.res, dev)
    legs = {"per_view": per_view, "batched": batched, "ms_ssim": ms_only}
    first = {k: fn(renders, gts) for k, fn in legs.items()}  # warm-up of every timed shape
    d_ssim = max(abs(a - b) for a, b in zip(first["per_view"][0], first["batched"][0]))
    d_psnr = max(abs(a - b) for a, b in zip(first["per_view"][1], first["batched"][1]))
    assert d_ssim < 1e-6 and d_psnr < 1e-4, (d_ssim, d_psnr)
    t = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn(renders, gts)
            t[k].append((time.perf_counter() - t0) / args.reps)
    lines = [{"leg": k, "frames": args.frames, "res": args.res, "seconds_median": statistics.median(v), "seconds": v,
              "reps_per_round": args.reps} for k, v in t.items()]
    med = {d["leg"]: d["seconds_median"] for d in lines}
    lines.append({"summary": "PSNR + SSIM of a test set: per-view loop vs one image_metrics call; MS-SSIM alone",
                  "frames": args.frames, "res": args.res, "per_view_ms": 1e3 * med["per_view"],
                  "batched_ms": 1e3 * med["batched"], "ms_ssim_ms": 1e3 * med["ms_ssim"],
                  "per_view_over_batched": med["per_view"] / med["batched"],
                  "max_abs_diff": {"ssim": d_ssim, "psnr_db": d_psnr},
                  "mean_ms_ssim": sum(first["ms_ssim"]) / len(first["ms_ssim"]),
                  "device": torch.cuda.get_device_name(0)})
    for d in lines:
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
