"""Motion-JPEG in an AVI container, on the standard library alone: every frame is one complete baseline JPEG file
(deformgs/jpeg_gpu.py writes them), the container a few hundred bytes of RIFF around them. The video that
render_cli --video mjpeg writes in place of the reference's imageio MP4 (H.264 needs an encoder library; MJPEG does
not). ffmpeg-based players, VLC and mpv read the format.

Layout (AVI 1.0, no OpenDML: the file stays below 2^31 bytes or is refused):

  RIFF 'AVI '
    LIST 'hdrl'   avih (AVIF_HASINDEX, microseconds per frame, frame count, largest chunk, size)
      LIST 'strl' strh ('vids' / 'MJPG', scale 1, rate fps)  strf (BITMAPINFOHEADER, 'MJPG', 24 bits)
    LIST 'movi'   one '00dc' chunk per frame, padded to even length
    idx1          one keyframe entry per frame, offsets relative to the 'movi' fourcc
"""
import struct

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
MAX_FILE = (1 << 31) - 1
_HDRL = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))  # 'hdrl', avih, LIST strl with strh and strf


def file_size(lengths):
    """The size of the AVI file that holds JPEG frames of these byte lengths."""
    lengths = list(lengths)
    movi = 4 + sum(8 + n + (n & 1) for n in lengths)
    return 12 + (8 + _HDRL) + (8 + movi) + (8 + 16 * len(lengths))


def _check(lengths, width, height, fps):
    if not lengths:
        raise ValueError("write_avi: no frames")
    if isinstance(fps, bool) or int(fps) != fps or not 1 <= fps <= 1000:
        raise ValueError(f"write_avi: fps must be a whole number in 1..1000 (scale 1, rate fps), got {fps!r}")
    if not (1 <= width <= 65535 and 1 <= height <= 65535) or 3 * width * height >= 1 << 32:
        raise ValueError(f"write_avi: frame size {width}x{height}")
    size = file_size(lengths)
    if size > MAX_FILE:
        raise ValueError(f"write_avi: the file would take {size} bytes, beyond the 2^31 - 1 of AVI 1.0 (OpenDML is not "
                         "written): fewer frames, a lower quality, or several files")
    return size


def write_avi(path, jpegs, width, height, fps):
    """jpegs: the frames as complete JPEG files (bytes), all of width x height. -> the file's size."""
    jpegs = [bytes(j) for j in jpegs]
    lengths = [len(j) for j in jpegs]
    size = _check(lengths, int(width), int(height), fps)  # before anything is written
    width, height, fps, n = int(width), int(height), int(fps), len(jpegs)
    largest = max(lengths)
    avih = struct.pack("<14I", round(1e6 / fps), 0, 0, AVIF_HASINDEX, n, 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIiI4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, n, largest, -1, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", 3 * width * height, 0, 0, 0, 0)
    strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)
    assert len(hdrl) == _HDRL
    movi, index, pos = [b"movi"], [], 4
    for j in jpegs:
        index.append(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, pos, len(j)))
        c = _chunk(b"00dc", j)
        movi.append(c)
        pos += len(c)
    body = b"".join([b"AVI ", _chunk(b"LIST", hdrl), _chunk(b"LIST", b"".join(movi)), _chunk(b"idx1", b"".join(index))])
    assert 8 + len(body) == size
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)))
        f.write(body)
    return size


def _chunk(tag, data):
    return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _fail(msg):
    raise ValueError(f"AVI: {msg}")


def _chunks(data, start, end):
    """The chunks of data[start:end] as (tag, payload offset, payload size)."""
    pos, out = start, []
    while pos < end:
        if pos + 8 > end:
            _fail(f"truncated chunk header at byte {pos}")
        tag, n = struct.unpack_from("<4sI", data, pos)
        if pos + 8 + n > end:
            _fail(f"chunk {tag!r} at byte {pos} runs past its parent")
        out.append((tag, pos + 8, n))
        pos += 8 + n + (n & 1)
    if pos != end and pos != end + 1:
        _fail("chunks do not fill their parent")
    return out


def read_avi(path):
    """-> (info, [the frames as JPEG bytes, unpadded]); info: width, height, fps, frames, microsec_per_frame,
    suggested_buffer, flags. Walks the chunks and checks idx1 against the '00dc' chunks it finds."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        _fail("not a RIFF AVI file")
    riff = struct.unpack_from("<I", data, 4)[0]
    if 8 + riff != len(data):
        _fail(f"RIFF size {riff} does not match the file length {len(data)}")
    info, frames, where, index, movi_at = {}, [], [], None, None
    for tag, off, n in _chunks(data, 12, len(data)):
        kind = data[off:off + 4] if tag == b"LIST" else None
        if kind == b"hdrl":
            for t2, o2, n2 in _chunks(data, off + 4, off + n):
                if t2 == b"avih":
                    v = struct.unpack_from("<14I", data, o2)
                    info.update(microsec_per_frame=v[0], flags=v[3], frames=v[4], streams=v[6], suggested_buffer=v[7],
                                width=v[8], height=v[9])
                elif t2 == b"LIST" and data[o2:o2 + 4] == b"strl":
                    for t3, o3, n3 in _chunks(data, o2 + 4, o2 + n2):
                        if t3 == b"strh":
                            s = struct.unpack_from("<4s4sIHHIIIIIIiI4H", data, o3)
                            info.update(stream_type=s[0], handler=s[1], scale=s[6], rate=s[7], length=s[9])
                        elif t3 == b"strf":
                            b = struct.unpack_from("<IiiHH4sIiiII", data, o3)
                            info.update(bi_width=b[1], bi_height=b[2], bit_count=b[4], compression=b[5], size_image=b[6])
        elif kind == b"movi":
            movi_at = off
            for t2, o2, n2 in _chunks(data, off + 4, off + n):
                if t2 != b"00dc":
                    _fail(f"unexpected chunk {t2!r} in movi")
                frames.append(data[o2:o2 + n2])
                where.append((o2 - 8 - off, n2))
        elif tag == b"idx1":
            index = [struct.unpack_from("<4sIII", data, off + 16 * k) for k in range(n // 16)]
    if movi_at is None or "rate" not in info or "width" not in info or "compression" not in info:
        _fail("missing hdrl or movi")
    if info["stream_type"] != b"vids" or info["handler"] != b"MJPG" or info["compression"] != b"MJPG":
        _fail("not a Motion-JPEG video stream")
    if index is None or len(index) != len(frames):
        _fail("idx1 is missing or does not list every frame")
    for k, (tag, flags, o, n) in enumerate(index):
        if tag != b"00dc" or (o, n) != where[k] or not flags & AVIIF_KEYFRAME:
            _fail(f"idx1 entry {k} does not point at its frame")
    if info["frames"] != len(frames) or info["length"] != len(frames):
        _fail("the frame counts of the headers do not match the movi list")
    info["fps"] = info["rate"] / info["scale"]
    return info, frames
