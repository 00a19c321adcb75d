"""CPU: the MJPEG-AVI container (deformgs/mjpeg.py) with JPEG files from the encoder's numpy restatement: the round
trip, the alignment of every chunk, idx1, the RIFF / LIST sizes, padding of odd-length frames and the size refusal."""
import os
import struct

import numpy as np
import pytest

import jpeg_encode_ref as ref
from deformgs import jpeg, mjpeg

W, H = 17, 9


@pytest.fixture(scope="module")
def jpegs():
    rng = np.random.default_rng(3)
    files = [ref.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), q, s)
             for q, s in ((90, "4:2:0"), (75, "4:4:4"), (25, "4:2:2"), (100, "4:2:0"), (90, "4:2:0"))]
    # lengths of both parities, whatever the coder gave: a JPEG decoder stops at EOI, so a trailing byte is harmless
    if all(len(f) % 2 == len(files[0]) % 2 for f in files):
        files[1] += b"\0"
    assert {len(f) % 2 for f in files} == {0, 1}
    return files


def _walk(data, start, end, depth=0):
    """Every chunk as (depth, tag, header offset, size); LISTs are entered."""
    pos, out = start, []
    while pos < end:
        tag, n = struct.unpack_from("<4sI", data, pos)
        out.append((depth, tag, pos, n))
        if tag == b"LIST":
            out += _walk(data, pos + 12, pos + 8 + n, depth + 1)
        pos += 8 + n + (n & 1)
    assert pos == end, (tag, pos, end)
    return out


@pytest.mark.parametrize("fps", [30, 60])
def test_round_trip(tmp_path, jpegs, fps):
    path = str(tmp_path / "v.avi")
    size = mjpeg.write_avi(path, jpegs, W, H, fps)
    assert size == os.path.getsize(path) == mjpeg.file_size([len(j) for j in jpegs])
    info, frames = mjpeg.read_avi(path)
    assert frames == jpegs  # unpadded, the odd-length ones too
    assert (info["width"], info["height"], info["fps"], info["frames"]) == (W, H, fps, len(jpegs))
    assert info["microsec_per_frame"] == round(1e6 / fps) and info["flags"] & mjpeg.AVIF_HASINDEX
    assert info["suggested_buffer"] == max(len(j) for j in jpegs)
    assert (info["bi_width"], info["bi_height"], info["bit_count"], info["size_image"]) == (W, H, 24, 3 * W * H)
    assert (info["scale"], info["rate"], info["streams"]) == (1, fps, 1)
    for f in frames:
        assert jpeg.decode_jpeg(f).shape == (H, W, 3)


def test_structure(tmp_path, jpegs):
    path = str(tmp_path / "v.avi")
    mjpeg.write_avi(path, jpegs, W, H, 30)
    with open(path, "rb") as f:
        data = f.read()
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    chunks = _walk(data, 12, len(data))  # asserts that every LIST's chunks add up to its size
    assert [(d, t) for d, t, _, _ in chunks if t != b"00dc"] == [
        (0, b"LIST"), (1, b"avih"), (1, b"LIST"), (2, b"strh"), (2, b"strf"), (0, b"LIST"), (0, b"idx1")]
    assert all(pos % 2 == 0 for _, _, pos, _ in chunks)
    movi = [pos for d, t, pos, _ in chunks if t == b"LIST" and data[pos + 8:pos + 12] == b"movi"][0] + 8
    frames = [(pos, n) for _, t, pos, n in chunks if t == b"00dc"]
    assert [n for _, n in frames] == [len(j) for j in jpegs]
    (idx_pos, idx_n), = [(pos, n) for _, t, pos, n in chunks if t == b"idx1"]
    assert idx_n == 16 * len(jpegs)
    for k, (pos, n) in enumerate(frames):
        tag, flags, off, size = struct.unpack_from("<4sIII", data, idx_pos + 8 + 16 * k)
        assert (tag, flags, off, size) == (b"00dc", mjpeg.AVIIF_KEYFRAME, pos - movi, n)
        assert data[movi + off:movi + off + 4] == b"00dc" and data[movi + off + 8:movi + off + 8 + size] == jpegs[k]
        if n & 1:
            assert data[pos + 8 + n] == 0  # the pad byte, not counted in the chunk size


def test_size_refusal_before_anything_is_written(tmp_path, monkeypatch):
    big = (1 << 31) // 4
    assert mjpeg.file_size([big] * 4) > mjpeg.MAX_FILE
    assert mjpeg.file_size([10, 11]) == 12 + 8 + mjpeg._HDRL + 8 + 4 + (8 + 10) + (8 + 12) + 8 + 32
    with pytest.raises(ValueError, match="2\\^31"):
        mjpeg._check([big] * 4, W, H, 30)
    # through write_avi itself, with the limit lowered instead of 2 GiB of frames
    monkeypatch.setattr(mjpeg, "MAX_FILE", 1000)
    path = str(tmp_path / "big.avi")
    with pytest.raises(ValueError, match="2\\^31"):
        mjpeg.write_avi(path, [b"\xff\xd8" + bytes(600) + b"\xff\xd9"] * 2, W, H, 30)
    assert not os.path.exists(path)


def test_refused_arguments(tmp_path):
    path = str(tmp_path / "x.avi")
    for kwargs in (dict(jpegs=[], width=W, height=H, fps=30), dict(jpegs=[b"x"], width=0, height=H, fps=30),
                   dict(jpegs=[b"x"], width=W, height=H, fps=29.97), dict(jpegs=[b"x"], width=W, height=H, fps=0)):
        with pytest.raises(ValueError):
            mjpeg.write_avi(path, **kwargs)
    assert not os.path.exists(path)


def test_reader_refuses_a_damaged_index(tmp_path, jpegs):
    path = str(tmp_path / "v.avi")
    mjpeg.write_avi(path, jpegs, W, H, 30)
    with open(path, "rb") as f:
        data = bytearray(f.read())
    at = data.rindex(b"idx1") + 8 + 8  # the offset field of the first entry
    data[at] ^= 2
    with open(path, "wb") as f:
        f.write(data)
    with pytest.raises(ValueError, match="idx1"):
        mjpeg.read_avi(path)
    with open(path, "wb") as f:
        f.write(data[:-3])
    with pytest.raises(ValueError):
        mjpeg.read_avi(path)
