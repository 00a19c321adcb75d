"""LPIPS-VGG scoring time of a rendered test set: --frames frame pairs at --res^2 (30 at 800^2: a D-NeRF test split).

Timed, medians of --rounds rounds, the legs alternating within a round (a host clock around a call that ends in a
host read of the scores):
  hip      deformgs.lpips.lpips: csrc/lpips.hip, fp32 MFMA convolutions, default scratch budget
  torch    the same definition in fp32 torch on the GPU (conv2d / max_pool2d under no_grad), in chunks of
           --torch_chunk pairs so that its activations fit as well
Random weights (the definition's cost does not depend on them); the legs' scores are compared before anything is
timed. Also reports the convolution FLOPs (2 * 9 * Cin * Cout per output pixel, both images of every pair) over the
whole hip call's time as a fraction of the 157.3 TFLOP/s fp32 matrix peak; the call also runs the pools and the
tail, so the convolution kernels alone sit a little higher. Prints one JSON line per leg and a summary; --out
appends them to a file (profiles/lpips_time.jsonl).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as tnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))

from deformgs.lpips import CONV_CIN, CONV_COUT, TAP_CHANNELS, lpips, weights_from_tensors  # noqa: E402

TAP_AFTER = (1, 3, 6, 9, 12)
PEAK_FP32_MATRIX = 157.3e12


def random_weights(dev):
    gen = torch.Generator().manual_seed(0)
    ws = [torch.randn((co, ci, 3, 3), generator=gen) * math.sqrt(2.0 / (9 * ci)) for ci, co in zip(CONV_CIN, CONV_COUT)]
    bs = [torch.randn((co,), generator=gen) * 0.1 for co in CONV_COUT]
    lins = [torch.rand((1, c, 1, 1), generator=gen) * (2.0 / c) for c in TAP_CHANNELS]
    return [w.to(dev) for w in ws], [b.to(dev) for b in bs], [l.to(dev) for l in lins]


def make_frames(n, res, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(res, device=dev, dtype=torch.float32),
                            torch.arange(res, device=dev, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([0.5 + 0.3 * torch.sin(0.02 * (c + 1) * xx) * torch.cos(0.015 * (c + 2) * yy) for c in range(3)])
    gts = (smooth + 0.08 * torch.randn((n, 3, res, res), device=dev, generator=gen)).clamp(0, 1)
    renders = (gts + 0.02 * torch.randn((n, 3, res, res), device=dev, generator=gen)).clamp(0, 1)
    return renders, gts


def torch_lpips(renders, gts, ws, bs, lins, chunk):
    shift = torch.tensor([-0.030, -0.088, -0.188], device=renders.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=renders.device).view(1, 3, 1, 1)
    out = []
    with torch.no_grad():
        for i in range(0, renders.shape[0], chunk):
            n = min(chunk, renders.shape[0] - i)
            v = (torch.cat([renders[i:i + n], gts[i:i + n]]) - shift) / scale
            total, k = 0.0, 0
            for j, (w, b) in enumerate(zip(ws, bs)):
                v = torch.relu_(tnf.conv2d(v, w, b, padding=1))
                if j in TAP_AFTER:
                    u = v / (v.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                    total = total + ((u[:n] - u[n:]).pow(2) * lins[k]).sum(1).mean((1, 2))
                    del u
                    k += 1
                    if k < 5:
                        v = tnf.max_pool2d(v, 2, 2)
            out.append(total)
    return torch.cat(out).tolist()


def conv_flops(frames, res):
    flops, h, w = 0, res, res
    for j, (ci, co) in enumerate(zip(CONV_CIN, CONV_COUT)):
        flops += 2 * 9 * ci * co * h * w
        if j in TAP_AFTER[:-1]:
            h, w = h // 2, w // 2
    return 2 * frames * flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch_chunk", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_time.py measures the GPU path: it needs a GPU"
    dev = torch.device("cuda", 0)
    ws, bs, lins = random_weights(dev)
    weights = weights_from_tensors(ws, bs, lins, dev)
    renders, gts = make_frames(args.frames, args.res, dev)
    legs = {"hip": lambda: lpips(renders, gts, weights).tolist(),
            "torch": lambda: torch_lpips(renders, gts, ws, bs, lins, args.torch_chunk)}
    first = {k: fn() for k, fn in legs.items()}  # warm-up of every timed shape
    diff = max(abs(a - b) for a, b in zip(first["hip"], first["torch"]))
    assert diff < 1e-4 * max(first["torch"]), (diff, first["hip"][:3], first["torch"][:3])
    t = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    lines = [{"leg": k, "frames": args.frames, "res": args.res, "seconds_median": statistics.median(v), "seconds": v}
             for k, v in t.items()]
    med = {d["leg"]: d["seconds_median"] for d in lines}
    flops = conv_flops(args.frames, args.res)
    lines.append({"summary": "LPIPS-VGG of a test set: csrc/lpips.hip vs fp32 torch on the same GPU, random weights",
                  "frames": args.frames, "res": args.res, "hip_ms": 1e3 * med["hip"], "torch_ms": 1e3 * med["torch"],
                  "torch_over_hip": med["torch"] / med["hip"], "conv_tflop": flops / 1e12,
                  "hip_conv_tflops": flops / med["hip"] / 1e12,
                  "hip_fraction_of_fp32_matrix_peak": flops / med["hip"] / PEAK_FP32_MATRIX,
                  "torch_fraction_of_fp32_matrix_peak": flops / med["torch"] / PEAK_FP32_MATRIX,
                  "max_abs_diff": diff, "mean_lpips": sum(first["hip"]) / len(first["hip"]),
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
