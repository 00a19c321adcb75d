"""Baseline JPEG writing with the transform and the entropy coder on the device (csrc/jpeg_encode.hip behind
dgs_jpeg_encode): a batch of uint8 RGB frames that are already on the GPU (rgb8 of render_frames) becomes one complete
JFIF file per frame, and only the compressed bytes cross to the host. The files are what libjpeg-turbo's default
compressor (PIL's Image.save(format="JPEG", quality=q, subsampling=s, optimize=False)) computes: the same quantised
coefficients, so the same decoded pixels; the Annex K Huffman tables; framed with a restart interval of one MCU row,
which is what lets the rows be coded in parallel. deformgs/jpeg.py reads them, as does any baseline decoder.

The host part is the framing alone: SOI, APP0 (JFIF 1.01, density 1:1), two DQT, SOF0, four DHT, DRI, SOS before the
device bytes and EOI behind them. Progressive, optimised-Huffman, arithmetic-coded and grayscale output are not
written."""
import struct

import numpy as np
import torch

from . import _encode, _lib
from .jpeg import ZIGZAG

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
MAX_DIM = 65535  # the SOF0 field

# ITU-T T.81 Annex K.1 (natural order): what jpeg_set_quality scales
_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def _ac_symbols(first_rows):
    """The 162 symbols of an Annex K.3 AC table: its head (the codes of up to 15 bits, in code order), then every
    other run/size symbol in ascending order (the 16-bit codes)."""
    head = bytes.fromhex(first_rows)
    rest = bytes(s for s in range(256) if 1 <= (s & 15) <= 10 and s not in head)
    return head + rest


# ITU-T T.81 Annex K.3, as DHT bodies: table class / id, codes per length 1..16, symbols. csrc/jpeg_encode.hip codes
# with the same four.
_DHT = (
    bytes([0x00, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12)),
    bytes([0x10, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]) + _ac_symbols(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f0243362728209"),
    bytes([0x01, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]) + bytes(range(12)),
    bytes([0x11, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]) + _ac_symbols(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f1"),
)
assert all(len(t) == 17 + sum(t[1:17]) for t in _DHT)


def quant_tables(quality):
    """jpeg_set_quality(quality, force_baseline): -> uint16 (2, 64) luma and chroma tables, natural order."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"encode_frames: quality must be an int in 1..100, got {quality!r}")
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (_STD_LUMA, _STD_CHROMA)],
                    np.uint16)


def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def jfif_header(width, height, hs, vs, qt):
    """Everything before the entropy-coded data."""
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for i in range(2):
        parts.append(_segment(0xDB, bytes([i]) + qt[i][ZIGZAG].astype(np.uint8).tobytes()))
    parts.append(_segment(0xC0, struct.pack(">BHHB", 8, height, width, 3)
                          + bytes((1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1))))
    parts.extend(_segment(0xC4, t) for t in _DHT)
    parts.append(_segment(0xDD, struct.pack(">H", -(-width // (8 * hs)))))  # one MCU row per restart interval
    parts.append(_segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(parts)


def _check(frames, subsampling):
    _encode.check_frames(frames)
    if frames.ndim == 3:
        raise ValueError(f"encode_frames takes (F, H, W, 3) RGB frames; grey (F, H, W) frames {tuple(frames.shape)} are "
                         "not written as JPEG (grayscale JPEG is unsupported, as in deformgs.jpeg)")
    if frames.ndim != 4 or frames.shape[3] != 3 or min(frames.shape) < 1:
        raise ValueError(f"encode_frames takes (F, H, W, 3) RGB frames, got {tuple(frames.shape)}")
    if max(frames.shape[1:3]) > MAX_DIM:
        raise ValueError(f"encode_frames: frames of {frames.shape[2]}x{frames.shape[1]} are beyond JPEG ({MAX_DIM} a side)")
    if subsampling not in SAMPLING:
        raise ValueError(f"encode_frames: subsampling must be one of {', '.join(SAMPLING)}, got {subsampling!r}")


def encode_streams(frames, quality=90, subsampling="4:2:0", capacity=None, out=None):
    """-> (packed, offsets, lengths, flags): the entropy-coded data of the frames back to back in one device uint8
    tensor of `capacity` bytes (default F (H W 3/2 + 1024)), where each starts and how long it is (device int64; the
    true lengths whatever the capacity), and per frame whether it did not fit and was left out (device int32). out:
    the tensor to write into (at least `capacity` bytes; default: a new one). No host synchronisation."""
    _check(frames, subsampling)
    qt = np.ascontiguousarray(quant_tables(quality))
    hs, vs = SAMPLING[subsampling]
    frames = frames.contiguous()
    F, H, W = frames.shape[:3]
    lib = _lib.load()
    scratch_bytes = lib.dgs_jpeg_encode_scratch_bytes(F, H, W, hs, vs)
    if not scratch_bytes:
        raise ValueError(f"encode_frames: frames of {W}x{H} are beyond the encoder")
    dev = frames.device
    if capacity is None:
        capacity = out.numel() if out is not None else F * (H * W * 3 // 2 + 1024)
    capacity = int(capacity)
    if out is not None and not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.uint8
                                and out.ndim == 1 and out.is_contiguous() and 0 <= capacity <= out.numel()):
        raise ValueError("encode_streams: out must be a contiguous 1-D uint8 tensor on the frames' device with at "
                         "least `capacity` bytes")
    if capacity < 0:
        raise ValueError(f"encode_streams: capacity {capacity}")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
        where = torch.empty((2, F), dtype=torch.int64, device=dev)
        flags = torch.empty(F, dtype=torch.int32, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.dgs_jpeg_encode(F, H, W, hs, vs, _lib.ptr(frames), qt.ctypes.data, _lib.ptr(out), capacity,
                                       _lib.ptr(where[0]), _lib.ptr(where[1]), _lib.ptr(flags), _lib.ptr(scratch),
                                       _lib.stream_ptr(dev)), "dgs_jpeg_encode")
    return out, where[0], where[1], flags


def encode_frames(frames, quality=90, subsampling="4:2:0", capacity=None):
    """frames: device uint8 (F, H, W, 3) RGB -> [F JFIF files as bytes]. Two copies to the host: the 2 F offsets and
    lengths, then the packed compressed bytes; no raw frame. Where the frames did not all fit the capacity (noise at
    a high quality), the call is repeated once with the exact total it has just read."""
    out, offsets, lengths, _ = encode_streams(frames, quality, subsampling, capacity)
    spans, total = _encode.fetch_spans(offsets, lengths)
    if total > (out.numel() if capacity is None else capacity):
        out, offsets, lengths, _ = encode_streams(frames, quality, subsampling, total)
        spans, again = _encode.fetch_spans(offsets, lengths)
        assert again == total
    packed = _encode.fetch_bytes(out, total)
    F, H, W = frames.shape[:3]
    head = jfif_header(W, H, *SAMPLING[subsampling], quant_tables(quality))
    return [b"".join((head, packed[o:o + n], b"\xff\xd9")) for o, n in spans]


def write_frames(paths, frames, quality=90, subsampling="4:2:0"):
    """Writes frame i to paths[i]."""
    _encode.write_files(paths, encode_frames(frames, quality, subsampling))
