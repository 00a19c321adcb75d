"""PNG streams with chosen filter types, and the procedural test images (helpers of tests/test_dataset.py,
tests/test_gpu_ingest.py, tests/golden/make_golden_dataset.py and tools/ingest_time.py).

The forward filters read only the original pixels (left, up, upper-left), so they are whole-image numpy."""
import struct
import zlib

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"
_CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}


def filtered_variants(px):
    """px: uint8 (H, W, C) -> uint8 (5, H, W*C): every row filtered with type 0..4 (mod 256)."""
    h, w, c = px.shape
    x = px.astype(np.int32)
    a = np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, 1:] = x[:-1, :-1]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    return np.stack([((x - q) & 255).astype(np.uint8).reshape(h, w * c) for q in preds])


def filter_scanlines(px, types):
    """px: uint8 (H, W, C); types: H filter types -> the filtered scanlines (H rows of 1 + W*C bytes)."""
    px = np.asarray(px, np.uint8)
    if px.ndim == 2:
        px = px[:, :, None]
    types = np.asarray(types, np.uint8)
    v = filtered_variants(px)
    rows = v[np.minimum(types, 4), np.arange(px.shape[0])]
    return np.concatenate([types[:, None], rows], axis=1).tobytes()


def adaptive_types(px):
    """The encoder heuristic of libpng: per row the type with the least sum of absolute (signed) bytes."""
    v = filtered_variants(np.asarray(px, np.uint8)).astype(np.int32)
    cost = np.where(v < 128, v, 256 - v).sum(axis=2)
    return np.argmin(cost, axis=0).astype(np.uint8)


def png_from_scanlines(w, h, channels, raw, depth=8, interlace=0, level=6):
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    ihdr = struct.pack(">IIBBBBB", w, h, depth, _CTYPE[channels], 0, 0, interlace)
    return _SIG + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b"")


def encode_png_filtered(px, types, level=6):
    """uint8 (H, W, C) with C in 1..4 (or (H, W)) and one filter type per row -> PNG bytes."""
    px = np.asarray(px, np.uint8)
    if px.ndim == 2:
        px = px[:, :, None]
    h, w, c = px.shape
    return png_from_scanlines(w, h, c, filter_scanlines(px, types), level=level)


def disc_image(w, h, t, n_discs=4, seed=0):
    """A rendered-looking RGBA frame: a few coloured, soft-edged, shaded discs that move with time t in
    [0, 1]; alpha falls to 0 outside them. -> uint8 (h, w, 4)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = (xx + 0.5) / w, (yy + 0.5) / h
    rgb = np.zeros((h, w, 3))
    alpha = np.zeros((h, w))
    for _ in range(n_discs):
        cx, cy, r = rng.uniform(0.25, 0.75), rng.uniform(0.25, 0.75), rng.uniform(0.12, 0.25)
        ax, ay, ph = rng.uniform(0.05, 0.2), rng.uniform(0.05, 0.2), rng.uniform(0, 2 * np.pi)
        col = rng.uniform(0.2, 1.0, 3)
        px, py = cx + ax * np.sin(2 * np.pi * t + ph), cy + ay * np.cos(2 * np.pi * t + ph)
        d = np.sqrt((u - px) ** 2 + (v - py) ** 2)
        cover = np.clip((r - d) / (0.25 * r), 0.0, 1.0)  # soft edge over a quarter of the radius
        shade = 0.55 + 0.45 * np.clip(1.0 - d / r, 0.0, 1.0) + 0.05 * np.sin(40 * u + 31 * v)
        rgb = rgb * (1 - cover[..., None]) + cover[..., None] * np.clip(col * shade[..., None], 0, 1)
        alpha = alpha * (1 - cover) + cover
    out = np.concatenate([rgb * (alpha[..., None] > 0), alpha[..., None]], axis=2)
    return (out * 255.0 + 0.5).astype(np.uint8)
