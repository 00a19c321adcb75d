"""Writes tests/golden/dataset_ingest.npz and tests/golden/dnerf_tiny/ (run by hand where a checkout of the
reference and PIL exist; the tests only read the results):

    python tests/golden/make_golden_dataset.py --reference /path/to/Deformable-3D-Gaussians

dataset_ingest.npz
  rgba_<W>x<H>, rgb_<W>x<H>           seeded random bytes
  comp_<bg>_<W>x<H>                   the RGBA arrays composited over black / white, in numpy float64 by the
                                      expression of scene/dataset_readers.py:249-255:
                                      arr = (c/255.0)*(a/255.0) + bg*(1 - a/255.0); arr*255.0 truncated to 8 bits
  resized_<bg>_<W>x<H>_<w>x<h>        float32 (3, h, w): the reference's own PILtoTorch
                                      (utils/general_utils.py:23-29, imported from the checkout) on the
                                      composited image, at the target size
  resized_rgb_<W>x<H>_<w>x<h>         the same on the RGB arrays (no composite)

The composite half is pinned by the written formula, not by a run of the reference: its
readCamerasFromTransforms cannot produce the fixture with a current PIL, where it raises in
Image.fromarray(<int8 array>, "RGB"). The resize half is a run of the reference's function.

dnerf_tiny/: transforms_train.json (6 frames), transforms_test.json (2 frames) and eight 32x32 RGBA PNGs of a
few soft-edged discs that move with `time` (tests/png_fixtures.disc_image), written with per-row filter types
cycling 0..4.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from png_fixtures import disc_image, encode_png_filtered  # noqa: E402

# (W, H) -> (w, h); the last two entries: one axis unchanged, no resize
RESIZE_CASES = [((19, 13), (10, 6)), ((32, 32), (16, 16)), ((24, 40), (12, 20)), ((33, 17), (8, 4)),
                ((16, 16), (16, 8)), ((19, 13), (19, 13))]
RGB_CASES = [((19, 13), (10, 6)), ((19, 13), (19, 13))]


def composite(rgba, white):
    bg = np.array([1, 1, 1]) if white else np.array([0, 0, 0])
    norm_data = rgba / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + bg * (1 - norm_data[:, :, 3:4])
    return (arr * 255.0).astype(np.int64).astype(np.uint8)


def orbit_c2w(azimuth, elevation, radius):
    cpos = np.array([radius * np.cos(elevation) * np.sin(azimuth), -radius * np.cos(elevation) * np.cos(azimuth),
                     radius * np.sin(elevation)])
    fwd = -cpos / np.linalg.norm(cpos)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, -fwd, cpos
    return c2w


def write_dnerf_tiny(root):
    k = 0
    for name, n in (("train", 6), ("test", 2)):
        os.makedirs(os.path.join(root, name), exist_ok=True)
        frames = []
        for i in range(n):
            t = i / (n - 1) if name == "train" else (i + 0.5) / n
            az = 2 * np.pi * (k / 8.0)
            el = 0.3 + 0.1 * np.sin(1.7 * k)
            img = disc_image(32, 32, t)
            with open(os.path.join(root, name, f"r_{i:03d}.png"), "wb") as f:
                f.write(encode_png_filtered(img, [(y + k) % 5 for y in range(32)], level=9))
            frames.append({"file_path": f"./{name}/r_{i:03d}", "rotation": 0.0, "time": float(t),
                           "transform_matrix": orbit_c2w(az, el, 4.0).tolist()})
            k += 1
        with open(os.path.join(root, f"transforms_{name}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of preacherwhite/Deformable-3D-Gaussians")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from PIL import Image
    from utils.general_utils import PILtoTorch  # the reference's own function
    rng = np.random.default_rng(20240607)
    out = {}
    for (W, H), _ in RESIZE_CASES:
        key = f"{W}x{H}"
        if f"rgba_{key}" not in out:
            out[f"rgba_{key}"] = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            # alpha 0 and 255 are the common values of real renders: make sure both occur
            out[f"rgba_{key}"][0, 0, 3], out[f"rgba_{key}"][-1, -1, 3] = 0, 255
            for bg, white in (("black", False), ("white", True)):
                out[f"comp_{bg}_{key}"] = composite(out[f"rgba_{key}"], white)
    for (W, H), (w, h) in RESIZE_CASES:
        for bg in ("black", "white"):
            img = Image.fromarray(out[f"comp_{bg}_{W}x{H}"], "RGB")
            out[f"resized_{bg}_{W}x{H}_{w}x{h}"] = PILtoTorch(img, (w, h)).numpy()
    out["rgb_19x13"] = rng.integers(0, 256, (13, 19, 3), dtype=np.uint8)
    for (W, H), (w, h) in RGB_CASES:
        img = Image.fromarray(out[f"rgb_{W}x{H}"], "RGB")
        out[f"resized_rgb_{W}x{H}_{w}x{h}"] = PILtoTorch(img, (w, h)).numpy()
    np.savez_compressed(os.path.join(HERE, "dataset_ingest.npz"), **out)
    write_dnerf_tiny(os.path.join(HERE, "dnerf_tiny"))
    print("wrote", len(out), "arrays and dnerf_tiny/")


if __name__ == "__main__":
    main()
