#!/usr/bin/env python3
"""Image writing time and size, --codec png or jpeg: --frames RGB frames at --res^2, the rgb8 output of render_frames on
the synthetic scene (--gaussians Gaussians, the deformation heads at 1/100 scale as tools/fps.py), to files in host
memory. Legs, medians of --rounds rounds, alternating within a round, each between two device synchronisations:

--codec png
  host_zlib   frames.cpu().numpy(), then deformgs.png.encode_png per frame
  device      one deformgs.png_gpu.encode_frames call (filter, deflate and pack kernels, the copy of the
              compressed bytes, the chunk framing and CRC on the host)
  Every device file is decoded and compared with its frame before the timing.

--codec jpeg (at --quality and --subsampling: what render_cli --video mjpeg spends per chunk before the container)
  device      one deformgs.jpeg_gpu.encode_frames call (transform, entropy twice, scan; the copy of the compressed
              bytes and the framing on the host)
  png_gpu     one deformgs.png_gpu.encode_frames call on the same frames, for scale
  host_pil    frames.cpu().numpy(), then PIL's Image.save(format="JPEG", optimize=False) per frame: only where PIL
              is installed; otherwise the absolute times of the other two legs are all there is
  The first device file is decoded by the device decoder (deformgs.ingest) and every one by PIL where installed, and
  where PIL is installed its decoded pixels must equal those of PIL's own file.

--profile runs the device leg alone (three calls) for a kernel trace. Prints one JSON line per leg and a summary
line; --out appends them to a file (profiles/png_encode_time.jsonl, profiles/jpeg_encode_time.jsonl)."""
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

from deformgs import ingest, jpeg_gpu, png, png_gpu  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None

_PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


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


def png_codec(args, frames):
    """-> (legs, check, summary): the timed legs in their order within a round; check(the device leg's files) -> the
    fields it adds to the summary line; summary(median seconds, bytes, per leg) -> the codec's summary fields."""
    def host_leg(f):
        a = f.cpu().numpy()
        return [png.encode_png(a[i]) for i in range(a.shape[0])]

    def check(files):
        want = frames.cpu().numpy()
        for i, data in enumerate(files):
            assert np.array_equal(png.decode_png(data), want[i]), f"frame {i} does not decode to its input"
        return {}

    def summary(med, sizes):
        return {"summary": "encode_frames vs .cpu().numpy() + encode_png per frame",
                "host_ms_per_frame": 1e3 * med["host_zlib"] / args.frames,
                "device_ms_per_frame": 1e3 * med["device"] / args.frames, "speedup": med["host_zlib"] / med["device"],
                "host_bytes": sizes["host_zlib"], "device_bytes": sizes["device"],
                "size_ratio": sizes["device"] / sizes["host_zlib"]}

    return [("host_zlib", host_leg), ("device", png_gpu.encode_frames)], check, summary


def jpeg_codec(args, frames):
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

    def check(files):
        got0 = ingest.ingest_images(files[:1], False, device=frames.device, return_uint8=True)[1][0].cpu().numpy()
        assert got0.shape == tuple(frames.shape[1:])
        err = np.abs(got0.astype(np.int32) - frames[0].cpu().numpy().astype(np.int32))
        pil_equal = None
        if Image is not None:
            pil_equal = all(np.array_equal(np.asarray(Image.open(io.BytesIO(a))), np.asarray(Image.open(io.BytesIO(b))))
                            for a, b in zip(files, host_leg(frames)))
            assert pil_equal, "a device file does not decode to the pixels of PIL's own file"
        return {"frame0_max_abs_error": int(err.max()), "frame0_mean_abs_error": float(err.mean()),
                "decodes_as_pils_file": pil_equal}

    def summary(med, sizes):
        d = {"summary": "jpeg_gpu.encode_frames" + (" vs .cpu().numpy() + PIL save per frame" if Image else
                                                    " (PIL is not installed: absolute times only)"),
             "quality": args.quality, "subsampling": args.subsampling,
             "device_ms_per_frame": 1e3 * med["device"] / args.frames,
             "png_gpu_ms_per_frame": 1e3 * med["png_gpu"] / args.frames, "device_bytes": sizes["device"],
             "png_gpu_bytes": sizes["png_gpu"]}
        if Image:
            d.update(host_pil_ms_per_frame=1e3 * med["host_pil"] / args.frames, speedup=med["host_pil"] / med["device"],
                     host_pil_bytes=sizes["host_pil"])
        return d

    legs = [("device", device_leg), ("png_gpu", png_gpu.encode_frames)] + ([("host_pil", host_leg)] if Image else [])
    return legs, check, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codec", required=True, choices=("png", "jpeg"))
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--quality", type=int, default=90, help="jpeg")
    ap.add_argument("--subsampling", default="4:2:0", choices=list(_PIL_SUBSAMPLING), help="jpeg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encode_time.py measures the GPU path: it needs a GPU"
    dev = torch.device("cuda", 0)
    frames = render(args.frames, args.res, args.gaussians, dev)
    torch.cuda.synchronize()
    legs, check, summary = (png_codec if args.codec == "png" else jpeg_codec)(args, frames)
    if args.profile:
        for _ in range(3):
            dict(legs)["device"](frames)
        torch.cuda.synchronize()
        return
    warm = {k: fn(frames) for k, fn in legs if not k.startswith("host_")}  # the device legs: warm-up, and the check
    checked = check(warm["device"])
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
    lines.append({**summary({d["leg"]: d["seconds_median"] for d in lines}, sizes), **checked, "frames": args.frames,
                  "res": args.res, "gaussians": args.gaussians, "raw_bytes": int(frames.numel()),
                  "device_name": torch.cuda.get_device_name(0)})
    for d in lines:
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
