"""A PNG writer and reader on the standard library alone (zlib + struct), 8 bits per channel, non-interlaced:
the writer RGB and grey, the reader also RGBA and grey + alpha (the D-NeRF images are RGBA). The render
script writes renders/ depth/ gt/ with it and the metrics script reads them back (the reference uses
torchvision.utils.save_image and PIL, render_baseline.py:44-55 / metrics.py:25-37; neither is assumed here).
inflate_png stops before the unfiltering: deformgs/ingest.py does that on the device."""
import struct
import zlib

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def encode_png(img, level=6):
    """img: uint8 array (H, W, 3) -> RGB, or (H, W) -> grey. Filter type 0 on every row."""
    a = np.ascontiguousarray(np.asarray(img))
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_png takes a uint8 (H, W, 3) or (H, W) array, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = a.reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return _SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, level)) + _chunk(b"IEND", b"")


def write_png(path, img, level=6):
    with open(path, "wb") as f:
        f.write(encode_png(img, level))


_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}  # colour type -> channels at 8 bits


def inflate_png(data):
    """-> (W, H, channels, filtered_scanlines): the chunk parse, header check and zlib inflate of decode_png
    without the unfiltering (H rows of one filter byte + W * channels bytes), for the device path of
    deformgs/ingest.py. Raises ValueError on anything decode_png does not read."""
    if data[:8] != _SIG:
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError("PNG without IHDR")
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or ctype not in _CHANNELS or interlace != 0:
        raise ValueError(f"unsupported PNG (bit depth {depth}, colour type {ctype}, interlace {interlace}): "
                         "8-bit RGB, RGBA, grey or grey + alpha, non-interlaced only")
    bpp = _CHANNELS[ctype]
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"PNG data does not inflate: {e}") from None
    if len(raw) != h * (w * bpp + 1):
        raise ValueError("PNG data length does not match its header")
    return w, h, bpp, raw


def unfilter(raw, w, h, bpp):
    """Filtered scanlines (h rows of 1 + w*bpp bytes) -> uint8 (h, w, bpp): the five PNG filter types mod 256,
    row 0 over a zero previous row, pixel 0 with zero left and upper-left neighbours. Average and Paeth are
    recurrences along the row that also read the row above, so the image is swept by anti-diagonals
    (pixel x of row r at step r + x: its left, upper and upper-left neighbours are done) with every row of a
    diagonal handled at once, the schedule of the HIP kernel (csrc/ingest.hip)."""
    lines = np.frombuffer(raw, np.uint8, h * (w * bpp + 1)).reshape(h, w * bpp + 1)
    ft = lines[:, 0].astype(np.int32)
    if ft.size and int(ft.max()) > 4:
        raise ValueError(f"PNG filter type {int(ft.max())}")
    x_in = lines[:, 1:].reshape(h, w, bpp).astype(np.int32)
    if not np.any(ft >= 3):  # no recurrence on the row above's left neighbour: whole rows at a time
        out = np.zeros((h, w, bpp), np.int32)
        prev = np.zeros((w, bpp), np.int32)
        for y in range(h):
            if ft[y] == 0:
                cur = x_in[y]
            elif ft[y] == 2:
                cur = (x_in[y] + prev) & 255
            else:  # Sub: a running sum per channel
                cur = np.cumsum(x_in[y], axis=0) & 255
            out[y] = cur
            prev = cur
        return out.astype(np.uint8)
    o = np.zeros((h + 1, w + 1, bpp), np.int32)  # one zero row above and one zero column to the left
    for d in range(h + w - 1):
        r = np.arange(max(0, d - w + 1), min(h - 1, d) + 1)
        x = d - r
        a, b, c = o[r + 1, x], o[r, x + 1], o[r, x]
        f = ft[r][:, None]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        pred = np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, np.where(f == 4, paeth, 0))))
        o[r + 1, x + 1] = (x_in[r, x] + pred) & 255
    return o[1:, 1:].astype(np.uint8)


def filter_rows(img):
    """uint8 (H, W, 3) or (H, W) -> the filtered scanlines (H rows of one filter byte + W * channels bytes) with
    libpng's adaptive choice: per row the type (None, Sub, Up, Average, Paeth) whose residuals, read as signed
    bytes, have the least sum of absolute values, ties toward the lower type. Row 0 over a zero previous row,
    pixel 0 with zero left and upper-left neighbours, as unfilter assumes. Every output byte reads original pixels
    only: the numpy restatement of k_png_filter (csrc/png_encode.hip)."""
    a = np.ascontiguousarray(np.asarray(img))
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"filter_rows takes a uint8 (H, W, 3) or (H, W) array, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    x = a.reshape(h, w, -1).astype(np.int32)
    left, up, ul = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    left[:, 1:] = x[:, :-1]
    up[1:] = x[:-1]
    ul[1:, 1:] = x[:-1, :-1]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    res = np.stack([(x - q).reshape(h, -1) & 255 for q in (np.zeros_like(x), left, up, (left + up) >> 1, paeth)])
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)
    types = np.argmin(cost, axis=0)  # the first of equal minima: the lower type
    rows = res[types, np.arange(h)].astype(np.uint8)
    return np.concatenate([types.astype(np.uint8)[:, None], rows], axis=1).tobytes()


def decode_png(data):
    """-> uint8 array (H, W, 3) RGB, (H, W) grey, (H, W, 4) RGBA or (H, W, 2) grey + alpha. 8 bits per
    channel, the five filter types, no interlace."""
    w, h, bpp, raw = inflate_png(data)
    out = unfilter(raw, w, h, bpp)
    return out[:, :, 0] if bpp == 1 else out


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())
