"""Dataset image ingest timing: 150 RGBA PNGs at 800x800 (a D-NeRF scene's worth), built in memory; with
--rgb --size 480 270, 150 RGB PNGs of a NeRF-DS capture's size (no alpha: no composite).

The images are rendered-looking frames (tests/png_fixtures.disc_image; --distinct of them, repeated), encoded
with adaptive per-row filters (the libpng heuristic), so Paeth and Average rows dominate as in real renders.
Timed, medians of --rounds rounds, the legs alternating within a round:
  (a) host inflate + validation, at most 16 threads (deformgs.ingest.front_end_all, the front end of ingest_images)
  (b) upload + HIP ingest to the float images at 800^2 and at 400^2 (ends in a device synchronise)
  (c) the numpy path on 5 of the images, scaled to the full count
  (d) where PIL is importable: the reference's pipeline per image: Image.open().convert("RGBA"), the float64
      composite, resize, / 255 (scene/dataset_readers.py:242-255, utils/general_utils.py:23-29), at 400^2;
      with --rgb the Nerfies reader's: np.array(Image.open()), Image.fromarray, resize, / 255
      (scene/dataset_readers.py:453-454)
With --jpeg [--size W H]: 150 baseline JPEGs (quality 90, 4:2:0, the same frames; written with PIL, or read from
--files DIR where PIL is absent), the legs: (a) host marker parse + Huffman decode into one buffer, at most 16
threads (deformgs.ingest.jpeg_decode_host); (b) upload + HIP IDCT / upsampling / colour + resize + float at full
and half size; (d) where PIL is importable, the reference's Colmap pipeline per image: Image.open, resize, / 255
(scene/dataset_readers.py:134, utils/general_utils.py:23-29). No numpy leg: deformgs/jpeg.py is for small images.
"full" and "half" are the file's size and half of it per axis (integer division).
Prints one JSON line per leg and a summary line; --out appends them to a file (profiles/ingest_time.jsonl).
"""
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
for p in (os.path.join(ROOT, "deformable-3d-gaussians_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from png_fixtures import adaptive_types, disc_image, encode_png_filtered  # noqa: E402

from deformgs import ingest  # noqa: E402


def build_images(n, width, height, distinct, rgb=False):
    frames = []
    hist = np.zeros(5, np.int64)
    for k in range(distinct):
        img = disc_image(width, height, k / distinct, n_discs=6, seed=1)
        if rgb:
            img = np.ascontiguousarray(img[:, :, :3])
        types = adaptive_types(img)
        hist += np.bincount(types, minlength=5)
        frames.append(encode_png_filtered(img, types))
    return [frames[i % distinct] for i in range(n)], hist


def reference_pipeline(data, size, rgb=False):
    from PIL import Image
    if rgb:
        image = Image.fromarray(np.array(Image.open(io.BytesIO(data))).astype(np.uint8))
        return torch.from_numpy(np.array(image.resize(size))) / 255.0
    im_data = np.array(Image.open(io.BytesIO(data)).convert("RGBA"))
    bg = np.array([0, 0, 0])
    norm_data = im_data / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + bg * (1 - norm_data[:, :, 3:4])
    image = Image.fromarray((arr * 255.0).astype(np.uint8), "RGB")
    return torch.from_numpy(np.array(image.resize(size))) / 255.0


def build_jpegs(n, width, height, distinct, files_dir=""):
    if files_dir:
        names = sorted(f for f in os.listdir(files_dir) if f.lower().endswith((".jpg", ".jpeg")))
        frames = []
        for f in names[:distinct]:
            with open(os.path.join(files_dir, f), "rb") as fh:
                frames.append(fh.read())
    else:
        from PIL import Image
        frames = []
        for k in range(distinct):
            buf = io.BytesIO()
            img = np.ascontiguousarray(disc_image(width, height, k / distinct, n_discs=6, seed=1)[:, :, :3])
            Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2)
            frames.append(buf.getvalue())
    return [frames[i % len(frames)] for i in range(n)]


def jpeg_main(args):
    dev = torch.device("cuda", 0)
    n = args.images
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    if not have_pil and not args.files:
        raise SystemExit("ingest_time.py --jpeg writes its images with PIL; without PIL give --files DIR of baseline JPEGs")
    W, H = args.size or (args.res, args.res)
    jpgs = build_jpegs(n, W, H, args.distinct, args.files)
    files = [(d, ingest.jpeg_header_native(d)) for d in jpgs]
    info = files[0][1]
    W, H, hs, vs = info.width, info.height, info.hs, info.vs
    full, half = (W, H), (W // 2, H // 2)

    def device_leg(coef, qt, size):
        return ingest.resize_float_device(ingest.jpeg_device(coef, qt, W, H, hs, vs, dev), size)[0]

    coef, qt = ingest.jpeg_decode_host(files)
    for size in (full, half):  # warm-up of every timed shape
        f = device_leg(coef[:8], qt[:8], size)
        torch.cuda.synchronize()
    if have_pil:
        want = reference_pipeline(jpgs[0], half, rgb=True).permute(2, 0, 1)
        assert torch.equal(f[0].cpu(), want), "HIP JPEG ingest differs from PIL on this machine"
    t = {k: [] for k in ("host_decode", "hip_full", "hip_half", "pil_half")}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        coef, qt = ingest.jpeg_decode_host(files)
        t["host_decode"].append(time.perf_counter() - t0)
        for key, size in (("hip_full", full), ("hip_half", half)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = device_leg(coef, qt, size)
            torch.cuda.synchronize()
            t[key].append(time.perf_counter() - t0)
            del f
        if have_pil:
            t0 = time.perf_counter()
            for d in jpgs:
                reference_pipeline(d, half, rgb=True)
            t["pil_half"].append(time.perf_counter() - t0)
    res = W if W == H else [W, H]
    lines = [{"leg": k, "format": "jpeg", "images": n, "res": res, "sampling": [hs, vs], "seconds_median": statistics.median(v),
              "seconds": v} for k, v in t.items() if v]
    med = {d["leg"]: d["seconds_median"] for d in lines}
    lines.append({"summary": "host_decode + hip_half vs pil_half", "format": "jpeg", "images": n, "res": res,
                  "sampling": [hs, vs], "hip_total_s": med["host_decode"] + med["hip_half"], "pil_s": med.get("pil_half"),
                  "pil": "absent on this machine: this project's figures only" if not have_pil else "present",
                  "device": torch.cuda.get_device_name(0), "file_bytes": sum(len(d) for d in jpgs),
                  "coefficient_bytes": int(coef.nbytes)})
    for d in lines:
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=150)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("W", "H"), help="a non-square size instead of --res")
    ap.add_argument("--rgb", action="store_true", help="RGB images (colour type 2), as real captures are")
    ap.add_argument("--jpeg", action="store_true", help="baseline JPEG files (4:2:0, quality 90), as a Colmap capture's")
    ap.add_argument("--files", default="", help="--jpeg: a directory of equally sized baseline JPEGs instead of PIL-written ones")
    ap.add_argument("--distinct", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_time.py measures the GPU path: it needs a GPU"
    if args.jpeg:
        return jpeg_main(args)
    dev = torch.device("cuda", 0)
    n = args.images
    W, H = args.size or (args.res, args.res)
    ch = 3 if args.rgb else 4
    full, half = (W, H), (W // 2, H // 2)
    pngs, hist = build_images(n, W, H, args.distinct, args.rgb)
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    raws = [m[4] for m in ingest.front_end_all(pngs, True)]
    # warm-up of every timed shape; the small result is also checked against the numpy path
    for size in (full, half):
        f, _ = ingest.ingest_group_device(raws[:8], W, H, ch, False, size, dev)
        torch.cuda.synchronize()
    want = ingest.ingest_group_numpy(raws[:1], W, H, ch, False, half)[0]
    assert np.array_equal(f[:1].cpu().numpy(), want), "HIP ingest differs from the numpy path"
    t = {k: [] for k in ("inflate", "hip_full", "hip_half", "numpy_half", "pil_half")}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        ingest.front_end_all(pngs, True)
        t["inflate"].append(time.perf_counter() - t0)
        for key, size in (("hip_full", full), ("hip_half", half)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f, _ = ingest.ingest_group_device(raws, W, H, ch, False, size, dev)
            torch.cuda.synchronize()
            t[key].append(time.perf_counter() - t0)
            del f
        t0 = time.perf_counter()
        ingest.ingest_group_numpy(raws[:5], W, H, ch, False, half)
        t["numpy_half"].append((time.perf_counter() - t0) * n / 5)
        if have_pil:
            t0 = time.perf_counter()
            for d in pngs:
                reference_pipeline(d, half, args.rgb)
            t["pil_half"].append(time.perf_counter() - t0)
    lines = []
    for k, v in t.items():
        if v:
            lines.append({"leg": k, "images": n, "res": W if W == H else [W, H], "channels": ch,
                          "seconds_median": statistics.median(v), "seconds": v})
    med = {d["leg"]: d["seconds_median"] for d in lines}
    lines.append({"summary": "inflate + hip_half vs pil_half", "images": n, "res": W if W == H else [W, H], "channels": ch,
                  "hip_total_s": med["inflate"] + med["hip_half"],
                  "pil_s": med.get("pil_half"), "filter_rows": {str(i): int(c) for i, c in enumerate(hist)},
                  "device": torch.cuda.get_device_name(0), "filtered_bytes": sum(len(r) for r in raws)})
    for d in lines:
        print(json.dumps(d), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
