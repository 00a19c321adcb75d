"""A PNG writer and reader on the standard library alone (zlib + struct): 8-bit RGB and 8-bit grey,
non-interlaced. The render script writes renders/ depth/ gt/ with it and the metrics script reads them
back (the reference uses torchvision.utils.save_image and PIL, render_baseline.py:44-55 / metrics.py:25-37;
neither is assumed here)."""
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


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def decode_png(data):
    """-> uint8 array (H, W, 3) or (H, W). 8-bit RGB / grey, the five filter types, no interlace."""
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
    if depth != 8 or ctype not in (0, 2) or interlace != 0:
        raise ValueError(f"unsupported PNG (bit depth {depth}, colour type {ctype}, interlace {interlace}): "
                         "8-bit RGB or grey, non-interlaced only")
    bpp = 3 if ctype == 2 else 1
    stride = w * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (stride + 1):
        raise ValueError("PNG data length does not match its header")
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:  # Sub: a running sum per channel
            cur = (np.cumsum(line.reshape(w, bpp), axis=0) & 255).reshape(-1)
        elif ft in (3, 4):  # Average / Paeth depend on the pixel to the left: sequential
            cur = np.zeros(stride, np.int32)
            ln, pv = line.tolist(), prev.tolist()
            c = [0] * stride
            for i in range(stride):
                a = c[i - bpp] if i >= bpp else 0
                b = pv[i]
                if ft == 3:
                    c[i] = (ln[i] + ((a + b) >> 1)) & 255
                else:
                    cc = pv[i - bpp] if i >= bpp else 0
                    c[i] = (ln[i] + _paeth(a, b, cc)) & 255
            cur = np.array(c, np.int32)
        else:
            raise ValueError(f"PNG filter type {ft}")
        out[y] = cur.astype(np.uint8)
        prev = cur
    return out.reshape(h, w, 3) if bpp == 3 else out.reshape(h, w)


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())
