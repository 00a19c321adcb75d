"""PNG writing with the filtering and the deflate on the device (csrc/png_encode.hip behind dgs_png_encode): a batch
of uint8 frames that are already on the GPU (rgb8 / depth8 of render_frames, an 8-bit ground truth) becomes one
complete PNG file per frame, and only the compressed bytes cross to the host. The files are standard 8-bit,
non-interlaced RGB or grey PNGs with adaptive row filters and one IDAT chunk; deformgs/png.py reads them.

The host part is the framing alone: signature, IHDR, the IDAT length and CRC (zlib.crc32) and IEND."""
import struct
import zlib

import torch

from . import _encode, _lib
from .png import _SIG, _chunk


def _check(frames):
    _encode.check_frames(frames, " (deformgs.png.encode_png is the host writer)")
    if not (frames.ndim == 3 or (frames.ndim == 4 and frames.shape[3] == 3)) or min(frames.shape) < 1:
        raise ValueError(f"encode_frames takes (F, H, W, 3) RGB or (F, H, W) grey frames, got {tuple(frames.shape)}")


def encode_streams(frames):
    """-> (packed, offsets, lengths): the zlib streams of the frames back to back in one device uint8 tensor, and
    where each starts and how long it is (device int64). No host synchronisation."""
    _check(frames)
    frames = frames.contiguous()
    F, H, W = frames.shape[:3]
    C = 3 if frames.ndim == 4 else 1
    lib = _lib.load()
    cap, scratch_bytes = lib.dgs_png_out_capacity(F, H, W, C), lib.dgs_png_encode_scratch_bytes(F, H, W, C)
    if not cap or not scratch_bytes:
        raise ValueError(f"encode_frames: frames of {W}x{H} are beyond the encoder (65536 a side)")
    dev = frames.device
    with torch.cuda.device(dev):
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        where = torch.empty((2, F), dtype=torch.int64, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.dgs_png_encode(F, H, W, C, _lib.ptr(frames), _lib.ptr(out), _lib.ptr(where[0]), _lib.ptr(where[1]),
                                      _lib.ptr(scratch), _lib.stream_ptr(dev)), "dgs_png_encode")
    return out, where[0], where[1]


def encode_frames(frames):
    """frames: device uint8 (F, H, W, 3) RGB or (F, H, W) grey -> [F PNG files as bytes]. Two copies to the host:
    the 2 F offsets and lengths, then the packed compressed bytes; no raw frame."""
    out, offsets, lengths = encode_streams(frames)
    F, H, W = frames.shape[:3]
    spans, total = _encode.fetch_spans(offsets, lengths)
    packed = _encode.fetch_bytes(out, total)
    ihdr = _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if frames.ndim == 4 else 0, 0, 0, 0))
    iend = _chunk(b"IEND", b"")
    files = []
    for o, n in spans:
        body = packed[o:o + n]
        files.append(b"".join((_SIG, ihdr, struct.pack(">I", n), b"IDAT", body,
                               struct.pack(">I", zlib.crc32(body, zlib.crc32(b"IDAT")) & 0xffffffff), iend)))
    return files


def write_frames(paths, frames):
    """Writes frame i to paths[i]."""
    _encode.write_files(paths, encode_frames(frames))
