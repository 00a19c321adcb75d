"""Dataset image ingest: PNG and baseline JPEG files -> the float (N, 3, h, w) images the cameras hold
(Camera.original_image).

What the reference does per image with PIL and numpy (scene/dataset_readers.py:242-255, utils/camera_utils.py:44,
utils/general_utils.py:23-29), restated in integer arithmetic so that it is bit-exact without PIL:

  1. unfilter the PNG scanlines (the five filter types, mod 256);
  2. RGBA only: composite over the background, arr = (c/255.0)*(a/255.0) + bg*(1 - a/255.0) in float64,
     arr*255.0 truncated to 8 bits — here a 256 x 256 byte table built with exactly that expression;
  3. when the target size differs: PIL's Image.resize default (bicubic a = -0.5, support 2*max(scale, 1),
     antialiased), horizontal pass then vertical pass, each rounding to uint8, weights normalised in double and
     converted to 22-bit fixed point, accumulator from 2^21, clip8(acc >> 22) (Pillow's Resample.c, 8bpc);
  4. float32 = byte / 255.0, channels first.

On a GPU device the host only parses chunks and inflates (zlib releases the GIL: a pool of at most 16 threads);
the filtered scanlines of all images of one (W, H, channels) go up in one copy and steps 1-4 are HIP kernels
(csrc/ingest.hip) on the current stream. On the CPU the same steps run in numpy: the oracle of the GPU tests
and the path for CPU-only use (a CPU device asked for explicitly, never a silent fallback).

A JPEG file (recognised by its signature, not its name) replaces steps 1-2 by libjpeg-turbo's default decode,
which is what the reference gets from Image.open: the host parses markers and Huffman-decodes to quantised
coefficients (csrc/jpeg_decode.h through ctypes, which releases the GIL: the same pool of threads, writing into
one host buffer per group), the coefficients and the per-image quantisation tables go up in one copy each, and
dequantisation, the 8x8 inverse DCT, chroma upsampling and YCbCr -> RGB are HIP kernels (csrc/jpeg.hip); steps
3-4 follow unchanged. On the CPU deformgs/jpeg.py does all of it in Python and numpy. There is no alpha, so
white_background has no effect. Images are grouped by (format, W, H, channels or chroma sampling).
"""
import ctypes
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import jpeg
from .png import inflate_png, unfilter

MAX_INFLATE_THREADS = 16
PRECISION_BITS = 32 - 8 - 2  # Pillow's fixed-point weights for 8-bit channels


def composite_table(white_background):
    """(256, 256) uint8 [colour, alpha]: dataset_readers.py:246-255 for every byte pair, in float64."""
    c = np.arange(256, dtype=np.float64)[:, None]
    a = np.arange(256, dtype=np.float64)[None, :]
    bg = 1.0 if white_background else 0.0
    arr = (c / 255.0) * (a / 255.0) + bg * (1 - a / 255.0)
    return (arr * 255.0).astype(np.int64).astype(np.uint8)


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_tables(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter over the whole axis:
    -> bounds (n_out, 2) int32 = first input index, tap count; coef (n_out, ksize) int32."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = np.array([_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)], np.float64)
        ww = 0.0
        for v in k:  # Pillow's running double sum, in its order
            ww += v
        if ww != 0.0:
            k = k / ww
        bounds[i] = (xmin, xmax)
        coef[i, :xmax] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
                          for v in k]
    return bounds, coef


def resample_numpy(img, axis, n_out, tables=None):
    """One resize pass of a uint8 array along `axis` (the integer arithmetic of k_resample)."""
    n_in = img.shape[axis]
    bounds, coef = tables or resample_tables(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for i in range(n_out):
        x0, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coef[i, :n].astype(np.int64), src[x0:x0 + n], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_numpy(rgb8, size):
    """uint8 (..., H, W, 3) -> (..., h, w, 3), size = (w, h): horizontal pass, then vertical; a pass whose
    axis keeps its size is skipped (as PIL does)."""
    w, h = size
    if rgb8.shape[-2] != w:
        rgb8 = resample_numpy(rgb8, rgb8.ndim - 2, w)
    if rgb8.shape[-3] != h:
        rgb8 = resample_numpy(rgb8, rgb8.ndim - 3, h)
    return rgb8


def composite_numpy(pixels, white_background):
    """uint8 (..., 4) RGBA -> (..., 3) over the background; (..., 3) passes through."""
    if pixels.shape[-1] == 3:
        return pixels
    lut = composite_table(white_background)
    return lut[pixels[..., :3], pixels[..., 3:4]]


def validate_scanlines(raw, w, h, channels):
    """The checks the device path relies on: the stream length and every filter byte (<= 4)."""
    stride = 1 + w * channels
    if len(raw) != h * stride:
        raise ValueError("PNG data length does not match its header")
    ft = np.frombuffer(raw, np.uint8).reshape(h, stride)[:, 0]
    if ft.size and int(ft.max()) > 4:
        raise ValueError(f"PNG filter type {int(ft.max())}")


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, "rb") as f:
        return f.read()


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def image_header(head):
    """The first 26 bytes of a file (more do no harm) -> (format, width, height, colour type). "png": the IHDR's
    size, or None where the bytes are short of it or hold no IHDR there, and its colour type byte (None when
    short). "jpeg": None for the rest, its size lies behind its markers (jpeg.jpeg_size). Neither signature:
    format None. The callers word their own refusals."""
    if head[:8] == PNG_SIGNATURE:
        ihdr = len(head) >= 24 and head[12:16] == b"IHDR"
        return ("png", int.from_bytes(head[16:20], "big") if ihdr else None,
                int.from_bytes(head[20:24], "big") if ihdr else None, head[25] if len(head) >= 26 else None)
    return "jpeg" if head[:2] == b"\xff\xd8" else None, None, None, None


def _pool_map(fn, items, threads):
    n = max(1, min(int(threads), MAX_INFLATE_THREADS, len(items)))
    if n == 1:
        return [fn(it) for it in items]
    with ThreadPoolExecutor(max_workers=n) as pool:
        return list(pool.map(fn, items))


def front_end_all(items, native_jpeg, threads=MAX_INFLATE_THREADS):
    """-> [(format, W, H, channels or (hs, vs), payload)] in input order. PNG: payload = the validated filtered
    scanlines. JPEG: only the header is read here; payload = (file bytes, header), the header
    being a _lib.JpegInfo (native_jpeg: the C++ front end) or a jpeg.JpegHeader (the Python one)."""
    def one(item):
        data = _read(item)
        fmt = image_header(data)[0]
        if fmt is None:
            raise ValueError("ingest_images takes PNG or JPEG files (neither signature found)")
        if fmt == "png":
            w, h, ch, raw = inflate_png(data)
            if ch not in (3, 4):
                raise ValueError(f"ingest_images takes RGB or RGBA images, got {ch} channel(s)")
            validate_scanlines(raw, w, h, ch)
            return "png", w, h, ch, raw
        hd = jpeg_header_native(data) if native_jpeg else jpeg.parse_header(data)
        return "jpeg", hd.width, hd.height, (hd.hs, hd.vs), (data, hd)
    return _pool_map(one, items, threads)


def jpeg_header_native(data):
    """dgs_jpeg_header (csrc/jpeg_decode.h) -> _lib.JpegInfo; ValueError with the front end's reason."""
    from . import _lib
    info = _lib.JpegInfo()
    err = ctypes.create_string_buffer(256)
    if _lib.load().dgs_jpeg_header(data, len(data), ctypes.byref(info), err, len(err)) != 0:
        raise ValueError(err.value.decode(errors="replace"))
    return info


def jpeg_blocks(info):
    """8x8 blocks of the three components together (padded to whole MCUs)."""
    return sum(int(info.blocks_w[c]) * int(info.blocks_h[c]) for c in range(3))


def jpeg_coefficients_native(data, info=None, out=None):
    """dgs_jpeg_coefficients -> int16 (blocks, 64), natural order, component-major (into `out` when given)."""
    from . import _lib
    info = info or jpeg_header_native(data)
    if out is None:
        out = np.empty((jpeg_blocks(info), 64), np.int16)
    err = ctypes.create_string_buffer(256)
    if _lib.load().dgs_jpeg_coefficients(data, len(data), ctypes.byref(info), out.ctypes.data_as(ctypes.c_void_p),
                                         out.size, err, len(err)) != 0:
        raise ValueError(err.value.decode(errors="replace"))
    return out


def jpeg_decode_host(files, threads=MAX_INFLATE_THREADS):
    """files: [(bytes, _lib.JpegInfo)] of one (W, H, sampling) -> int16 (B, blocks, 64) coefficients in one host
    buffer, filled by at most 16 threads, and the uint16 (B, 3, 64) quantisation tables."""
    n = jpeg_blocks(files[0][1])
    coef = np.empty((len(files), n, 64), np.int16)
    qt = np.stack([np.ctypeslib.as_array(info.qt).reshape(3, 64) for _, info in files]).astype(np.uint16)
    _pool_map(lambda k: jpeg_coefficients_native(files[k][0], files[k][1], coef[k]), list(range(len(files))), threads)
    return coef, qt


def jpeg_device(coef, qt, W, H, hs, vs, device):
    """Host coefficients (B, blocks, 64) and tables (B, 3, 64) -> device uint8 (B, H, W, 3): one upload each,
    then dgs_ingest_jpeg on the current stream."""
    from . import _lib
    B, n = coef.shape[0], coef.shape[1]
    cd = torch.from_numpy(coef).to(device)
    qd = torch.from_numpy(qt.view(np.int16)).to(device)  # torch has no uint16 arithmetic; the bits are what goes up
    scratch = torch.empty(B * n * 64, dtype=torch.uint8, device=device)
    rgb8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=device)
    _lib.check(_lib.load().dgs_ingest_jpeg(B, W, H, hs, vs, _lib.ptr(cd), _lib.ptr(qd), _lib.ptr(rgb8), _lib.ptr(scratch),
                                           _lib.stream_ptr(rgb8.device)), "ingest_jpeg")
    return rgb8


def unfilter_device(scan, B, W, H, channels, lut=None):
    """scan: device uint8 tensor of B x H x (1 + W*channels) validated scanlines -> (B, H, W, channels) bytes,
    or (B, H, W, 3) composited with the device table `lut` (channels 4 only)."""
    from . import _lib
    _lib.require_cuda(scan, lut)
    if scan.dtype != torch.uint8 or scan.numel() != B * H * (1 + W * channels):
        raise ValueError("unfilter_device: scanline buffer does not match (B, W, H, channels)")
    out = torch.empty((B, H, W, 3 if lut is not None else channels), dtype=torch.uint8, device=scan.device)
    _lib.check(_lib.load().dgs_ingest_unfilter(B, W, H, channels, _lib.ptr(scan), _lib.ptr(lut), _lib.ptr(out),
                                               _lib.stream_ptr(scan.device)), "ingest_unfilter")
    return out


def _resample_device(img, axis, n_out):
    """img: device uint8 (B, H, W, 3); one pass along axis 1 (vertical) or 2 (horizontal)."""
    from . import _lib
    B, H, W, C = img.shape
    n_in = img.shape[axis]
    bounds, coef = resample_tables(n_in, n_out)
    bd = torch.from_numpy(bounds).to(img.device)
    cd = torch.from_numpy(coef).to(img.device)
    outer, inner = (B * H, C) if axis == 2 else (B, W * C)
    shape = (B, H, n_out, C) if axis == 2 else (B, n_out, W, C)
    out = torch.empty(shape, dtype=torch.uint8, device=img.device)
    _lib.check(_lib.load().dgs_ingest_resample(outer, n_in, n_out, inner, _lib.ptr(img), _lib.ptr(bd), _lib.ptr(cd),
                                               coef.shape[1], _lib.ptr(out), _lib.stream_ptr(img.device)),
               "ingest_resample")
    return out


def _to_float_device(rgb8, out):
    from . import _lib
    B, H, W, _ = rgb8.shape
    _lib.check(_lib.load().dgs_ingest_to_float(B, H, W, _lib.ptr(rgb8), _lib.ptr(out), _lib.stream_ptr(rgb8.device)),
               "ingest_to_float")


def _target(size, W, H):
    if size is None:
        return W, H
    w, h = size(W, H) if callable(size) else size
    if int(w) < 1 or int(h) < 1:
        raise ValueError(f"ingest_images: target size {(w, h)}")
    return int(w), int(h)


def resize_float_device(rgb8, size, out=None):
    """Steps 3-4 on the device, the tail of every group: uint8 (B, H, W, 3) -> horizontal pass, vertical pass (a
    pass whose axis keeps its size is skipped) -> float, on the current stream. -> (float (B, 3, h, w), uint8
    (B, h, w, 3)). `out`: a (B, 3, h, w) float view to fill."""
    w, h = size
    if w != rgb8.shape[2]:
        rgb8 = _resample_device(rgb8, 2, w)
    if h != rgb8.shape[1]:
        rgb8 = _resample_device(rgb8, 1, h)
    if out is None:
        out = torch.empty((rgb8.shape[0], 3, h, w), dtype=torch.float32, device=rgb8.device)
    _to_float_device(rgb8, out)
    return out, rgb8


def resize_float_numpy(px, size):
    """Steps 3-4 in numpy: uint8 (B, H, W, 3) -> (float32 (B, 3, h, w), uint8 (B, h, w, 3)) arrays."""
    rgb8 = np.ascontiguousarray(resize_numpy(px, size))
    return np.ascontiguousarray(rgb8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0), rgb8


def ingest_group_device(raws, W, H, channels, white_background, size, device, out=None, lut=None):
    """One (W, H, channels) group on the device: one upload, then unfilter (+ composite) -> resize -> float on
    the current stream. -> (float (B, 3, h, w), uint8 (B, h, w, 3)). `out`: a (B, 3, h, w) float view to fill.
    `lut`: the composite table already on the device; without one an RGBA group uploads its own."""
    host = torch.from_numpy(np.frombuffer(b"".join(raws), np.uint8).copy())
    scan = host.to(device)
    if channels == 4 and lut is None:
        lut = torch.from_numpy(composite_table(white_background).reshape(-1).copy()).to(device)
    return resize_float_device(unfilter_device(scan, len(raws), W, H, channels, lut if channels == 4 else None), size, out)


def ingest_jpeg_group_device(files, W, H, sampling, size, device, out=None, threads=MAX_INFLATE_THREADS):
    """One (W, H, sampling) group of JPEG files [(bytes, _lib.JpegInfo)] on the device: threaded Huffman
    decode into one host buffer, two uploads, IDCT + upsampling + colour, then resize -> float as for PNG.
    -> (float (B, 3, h, w), uint8 (B, h, w, 3))."""
    coef, qt = jpeg_decode_host(files, threads)
    return resize_float_device(jpeg_device(coef, qt, W, H, sampling[0], sampling[1], device), size, out)


def ingest_jpeg_group_numpy(files, size):
    """The same in Python and numpy (deformgs/jpeg.py). files: [(bytes, jpeg.JpegHeader)]."""
    px = np.stack([jpeg.upsample_color(jpeg.idct_planes(jpeg.decode_coefficients(d, hd), hd), hd) for d, hd in files])
    return resize_float_numpy(px, size)


def ingest_group_numpy(raws, W, H, channels, white_background, size):
    """The same steps in numpy. -> (float32 (B, 3, h, w), uint8 (B, h, w, 3)) arrays."""
    px = np.stack([unfilter(r, W, H, channels) for r in raws])
    return resize_float_numpy(composite_numpy(px, white_background), size)


def ingest_images(images, white_background, size=None, device="cuda", return_uint8=False, threads=MAX_INFLATE_THREADS):
    """images: PNG (8-bit RGB or RGBA) or baseline JPEG files as bytes or paths, told apart by their signature.
    size: None (keep), (w, h), or a function (W, H) -> (w, h) of the file's size (the -r rule). -> float32
    (N, 3, h, w) on `device`, in input order (with return_uint8 also the uint8 (N, h, w, 3) image). Images are
    grouped by (format, W, H, channels or chroma sampling), one launch sequence per group; all groups must reach
    one target size. white_background has no effect on images without alpha (RGB PNG, JPEG). Raises ValueError
    on malformed or unsupported files."""
    dev = torch.device(device)
    images = list(images)
    metas = front_end_all(images, dev.type == "cuda", threads)
    groups = {}
    for i, (fmt, W, H, kind, _) in enumerate(metas):
        groups.setdefault((fmt, W, H, kind), []).append(i)
    targets = {_target(size, W, H) for (_, W, H, _) in groups}
    if len(targets) > 1:
        raise ValueError(f"ingest_images: the images reach different sizes {sorted(targets)}; pass size=(w, h)")
    if not images:
        empty = torch.empty((0, 3, 0, 0), dtype=torch.float32, device=dev)
        return (empty, torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=dev)) if return_uint8 else empty
    w, h = next(iter(targets))
    out = torch.empty((len(images), 3, h, w), dtype=torch.float32, device=dev)
    out8 = torch.empty((len(images), h, w, 3), dtype=torch.uint8, device=dev) if return_uint8 else None
    for (fmt, W, H, ch), idx in groups.items():
        raws = [metas[i][4] for i in idx]
        whole = len(groups) == 1  # then the group's result is the output itself
        if dev.type == "cuda":
            if fmt == "jpeg":
                f, u = ingest_jpeg_group_device(raws, W, H, ch, (w, h), dev, out if whole else None, threads)
            else:
                f, u = ingest_group_device(raws, W, H, ch, white_background, (w, h), dev, out if whole else None)
        else:
            if fmt == "jpeg":
                f, u = ingest_jpeg_group_numpy(raws, (w, h))
            else:
                f, u = ingest_group_numpy(raws, W, H, ch, white_background, (w, h))
            f, u = torch.from_numpy(f), torch.from_numpy(u)
        if not (whole and dev.type == "cuda"):
            out[idx] = f.to(dev)
        if out8 is not None:
            out8[idx] = u.to(dev)
    return (out, out8) if return_uint8 else out
