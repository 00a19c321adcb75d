#!/usr/bin/env python3
"""Writes tests/golden/jpeg_encode.npz: what PIL (Pillow 12.2.0 with libjpeg-turbo 3.1.4) makes of the encoder
tests' source images. Run by hand where Pillow is installed; no test imports it.

Per case `<W>x<H>_<content>` the source RGB array (`src_...`), and per (case, sampling, quality) PIL's
Image.save(format="JPEG", quality=q, subsampling=s, optimize=False) as
  `<W>x<H>_<content>_<444|422|420>_q<q>_coef`  the quantised coefficients of PIL's file, read with
                                              deformgs.jpeg.parse_header / decode_coefficients
  `..._pix`                                   np.asarray(Image.open(that file))
and per quality `qt_q<q>`: the luma and chroma quantisation tables of PIL's files, natural order.
`groups`: `<W>x<H>_<sampling>_q<q>`, each with every content of `contents_<W>x<H>` (one encoder call in the GPU test).

Contents: uniform noise (the longest codes, many 0xFF bytes to stuff), constant grey and constant (255, 0, 0)
(EOB-only blocks), a smooth gradient, an 8x8-periodic grey pattern of the highest DCT frequency alone (coefficient
63 and its neighbours: ZRL runs and blocks that end without EOB), the same frequency as a square wave of full swing
(at quality 100 its coefficient 63 is in category 10, the longest AC code + value), 8x8 blocks of black and white in
turn (DC differences of category 11 at quality 100), and at 100x72 a frame of soft discs on black
(tests/png_fixtures.disc_image composited, standing for a rendered frame)."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from deformgs import jpeg  # noqa: E402
from png_fixtures import disc_image  # noqa: E402

SAMPLINGS = {"444": 0, "422": 1, "420": 2}
QUALITIES = (25, 75, 90, 100)
# (W, H): samplings. 8x80 and 24x150 have ten MCU rows: the restart counter wraps past RST7
SIZES = {(1, 1): ("444", "422", "420"), (8, 8): ("444", "422", "420"), (16, 16): ("444", "422", "420"),
         (17, 9): ("444", "422", "420"), (33, 31): ("444", "422", "420"), (8, 80): ("444",), (24, 150): ("420",)}
CONTENTS = ("noise", "grey", "red", "gradient", "hf", "square", "blocks")


def content(kind, w, h, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "grey":
        return np.full((h, w, 3), 128, np.uint8)
    if kind == "red":
        return np.full((h, w, 3), (255, 0, 0), np.uint8)
    if kind == "gradient":
        d = max(w + h - 2, 1)
        return np.stack([255 * xx // max(w - 1, 1), 255 * yy // max(h - 1, 1), 255 - 255 * (xx + yy) // d], -1).astype(np.uint8)
    if kind == "hf":
        c = np.cos((2 * (np.arange(8)) + 1) * 7 * np.pi / 16)
        v = np.clip(np.rint(128 + 110 * np.outer(c, c)), 0, 255).astype(np.uint8)
        return np.repeat(v[yy % 8, xx % 8][:, :, None], 3, axis=2)
    if kind == "square":
        c = np.sign(np.cos((2 * (np.arange(8)) + 1) * 7 * np.pi / 16))
        v = (128 + 127 * np.outer(c, c)).astype(np.uint8)
        return np.repeat(v[yy % 8, xx % 8][:, :, None], 3, axis=2)
    if kind == "blocks":
        return np.repeat((255 * ((xx // 8 + yy // 8) & 1)).astype(np.uint8)[:, :, None], 3, axis=2)
    raise ValueError(kind)


def blobs(w, h):
    d = disc_image(w, h, 0.3, n_discs=6, seed=5)
    rgb, a = d[:, :, :3].astype(np.int32), d[:, :, 3:4].astype(np.int32)
    return ((rgb * a + 127) // 255).astype(np.uint8)


def main():
    out, groups = {}, []
    sources = {}
    for k, ((w, h), samplings) in enumerate(SIZES.items()):
        names = []
        for j, kind in enumerate(CONTENTS):
            sources[f"{w}x{h}_{kind}"] = content(kind, w, h, 100 * k + j)
            names.append(kind)
        out[f"contents_{w}x{h}"] = np.array(names)
        groups += [(w, h, s, q) for s in samplings for q in QUALITIES]
    sources["100x72_blobs"] = blobs(100, 72)
    out["contents_100x72"] = np.array(["blobs"])
    groups += [(100, 72, "444", 90), (100, 72, "420", 90)]
    for name, rgb in sources.items():
        out[f"src_{name}"] = rgb
    for w, h, s, q in groups:
        for kind in out[f"contents_{w}x{h}"]:
            rgb = sources[f"{w}x{h}_{kind}"]
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, format="JPEG", quality=q, subsampling=SAMPLINGS[s], optimize=False)
            data = b.getvalue()
            hd = jpeg.parse_header(data)
            assert (hd.width, hd.height) == (w, h) and (hd.hs, hd.vs) == {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[s]
            assert np.array_equal(hd.qt[1], hd.qt[2])
            qt = hd.qt[:2].copy()
            assert np.array_equal(out.setdefault(f"qt_q{q}", qt), qt)
            key = f"{w}x{h}_{kind}_{s}_q{q}"
            out[f"{key}_coef"] = jpeg.decode_coefficients(data, hd)
            out[f"{key}_pix"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    out["groups"] = np.array([f"{w}x{h}_{s}_q{q}" for w, h, s, q in groups])
    path = os.path.join(HERE, "jpeg_encode.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(groups)} groups, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
