"""GPU: the device PNG encoder (csrc/png_encode.hip behind deformgs.png_gpu.encode_frames). Every file must decode
(deformgs.png.decode_png: zlib's inflater + the numpy unfilter) to the input bitwise, and its inflated IDAT must
equal deformgs.png.filter_rows(input) bitwise: the row filter kernel against its numpy restatement, the deflate and
pack kernels against zlib. Shapes around the 32 KiB segment size, the stored fallback, degenerate Huffman
alphabets, batches, reproducibility, the size conditions and the refused inputs."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from conftest import gpu_available
from png_fixtures import disc_image

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

_GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ingest.npz"))
SEG = 32768  # PNG_SEG of csrc/png_encode.hip
FRAMING = 8 + 25 + 12 + 12 + 2 + 4  # signature, IHDR, IDAT and IEND framing, zlib header, Adler-32


def _idat(data):
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            out.append(data[pos + 8:pos + 8 + n])
        assert zlib.crc32(data[pos + 4:pos + 8 + n]) & 0xffffffff == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        pos += 12 + n
    assert pos == len(data) and len(out) == 1
    return out[0]


def _encode(frames):
    from deformgs import png_gpu
    return png_gpu.encode_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda())


def _check(files, frames):
    from deformgs import png
    assert len(files) == len(frames)
    for data, img in zip(files, frames):
        assert isinstance(data, bytes)
        assert zlib.decompress(_idat(data)) == png.filter_rows(img)
        got = png.decode_png(data)
        assert got.shape == img.shape and np.array_equal(got, img)


def _blobs(h, w, t, white=False):
    d = disc_image(w, h, t, n_discs=5, seed=3)
    rgb, a = d[:, :, :3].astype(np.int32), d[:, :, 3:4].astype(np.int32)
    bg = 255 if white else 0
    return ((rgb * a + bg * (255 - a) + 127) // 255).astype(np.uint8)


def _rng(seed):
    return np.random.default_rng(seed)


def _runs_image():
    """Grey rows of runs of exactly 2, 3 and 259 equal bytes (and 1, 4, 258, 260), alternating with rows of other
    values so that no filter merges them: the filtered rows keep runs of those lengths."""
    lengths = (2, 3, 259, 1, 4, 258, 1, 260, 2, 3)
    w = sum(lengths)
    img = np.zeros((12, w), np.uint8)
    for y in range(12):
        v, x = 40 + 17 * y, 0
        for k, n in enumerate(lengths):
            img[y, x:x + n] = (v + 91 * k * (1 + y % 3)) & 255
            x += n
    return img


SHAPE_CASES = {
    "1x1_rgb": _rng(1).integers(0, 256, (1, 1, 3), dtype=np.uint8),
    "1x1_grey": _rng(2).integers(0, 256, (1, 1), dtype=np.uint8),
    "1x7_rgb": _rng(3).integers(0, 256, (1, 7, 3), dtype=np.uint8),
    "7x1_rgb": _rng(4).integers(0, 256, (7, 1, 3), dtype=np.uint8),
    "7x1_grey": _rng(5).integers(0, 256, (7, 1), dtype=np.uint8),
    "67x173_rgb_blobs": _blobs(67, 173, 0.2),  # 34 840 bytes of scanlines: the segment boundary falls in row 63
    "250x300_grey": np.ascontiguousarray(_blobs(250, 300, 0.6)[:, :, 1]),
    "256x256_rgb_blobs": _blobs(256, 256, 0.4),
    "256x256_rgb_blobs_white": _blobs(256, 256, 0.4, white=True),
}


@pytest.mark.parametrize("name", sorted(SHAPE_CASES))
def test_shapes(name):
    img = SHAPE_CASES[name]
    _check(_encode(img[None]), img[None])


@pytest.mark.parametrize("name", [str(c) for c in _GOLD["cases"]])
def test_decoded_photographs(name):
    img = _GOLD[f"{name}_rgb"]
    _check(_encode(img[None]), img[None])


def test_constant_frame_long_runs_across_segments():
    """Up-filtered rows are one filter byte and 768 zeros: runs longer than 258; 196 864 bytes = 7 segments, whose
    boundaries fall inside runs. Under 2 % of the raw scanlines: a 258-byte match costs at most 13 bits and a
    segment's header <= 172 bytes per 32 KiB."""
    img = np.full((256, 256, 3), 77, np.uint8)
    files = _encode(img[None])
    _check(files, img[None])
    assert len(_idat(files[0])) < 0.02 * 256 * (1 + 256 * 3)
    grey = np.full((300, 700), 200, np.uint8)  # 210 300 bytes, rows of 701: boundaries mid-run at other phases
    _check(_encode(grey[None]), grey[None])


def test_runs_of_exactly_2_3_and_259():
    from deformgs import png
    img = _runs_image()
    lines = np.frombuffer(png.filter_rows(img), np.uint8)
    edges = np.flatnonzero(np.diff(lines) != 0)
    runs = set(np.diff(np.concatenate([[-1], edges, [lines.size - 1]])).tolist())
    assert {2, 3, 259} <= runs, sorted(runs)
    _check(_encode(img[None]), img[None])


def test_noise_takes_the_stored_fallback():
    img = _rng(21).integers(0, 256, (120, 160, 3), dtype=np.uint8)
    files = _encode(img[None])
    _check(files, img[None])
    raw = 120 * (1 + 160 * 3)
    nseg = -(-raw // SEG)
    assert len(files[0]) <= raw + 5 * nseg + FRAMING
    body = _idat(files[0])
    assert (body[2] & 7) == 0  # the first block is stored (BTYPE 00) and not the final one
    assert struct.unpack("<HH", body[3:7]) == (SEG, SEG ^ 0xFFFF)


def test_noise_segment_among_constant_ones():
    """256x200 RGB, 601 bytes a row: rows 55..108 (bytes 33 055 .. 65 508) are noise, so segment 1 (32 768 .. 65 535)
    is all literals but its last bytes, and the others are all matches."""
    img = np.full((256, 200, 3), 30, np.uint8)
    img[55:109] = _rng(22).integers(0, 256, (54, 200, 3), dtype=np.uint8)
    _check(_encode(img[None]), img[None])


def test_segment_without_any_match():
    """A segment in which every byte differs from its neighbours has no length and no distance symbol: the block
    still declares one distance code. One grey row of 16 000 pixels (one segment) that climbs by steps of 2, 3 or
    4, never the same step twice running: the Sub residuals are those steps and the filter byte 1 equals none of
    them. An alphabet of three codes at 2 bits at the most, so the dynamic block is taken, not the stored one:
    the file stays under a third of the scanline bytes."""
    from deformgs import png
    r = _rng(23)
    state = np.concatenate([[0], r.integers(1, 3, 15999).cumsum()]) % 3
    img = ((2 + state).cumsum() % 256).astype(np.uint8)[None, :]
    lines = np.frombuffer(png.filter_rows(img), np.uint8)
    assert lines[0] == 1 and not np.any(lines[1:] == lines[:-1])
    files = _encode(img[None])
    _check(files, img[None])
    assert len(files[0]) < 16001 // 3


def test_single_symbol_segment():
    """Black grey frames: filter None, the stream is zeros throughout (the filter byte too), one run. 1x258 is the
    literal 0 and one match of 258: exactly one literal/length symbol of each kind besides end-of-block; 1x259 adds
    a second literal; 64x1024 is two segments of one run each."""
    for shape in ((1, 258), (1, 259), (1, 4000), (64, 1024)):
        img = np.zeros(shape, np.uint8)
        _check(_encode(img[None]), img[None])


# The inputs of test_streams_equal_the_recorded_ones, the smallest that reach each path of the encoder: one pixel; a
# column; two segments with the boundary inside a row (twice, so that one shape has a batch); the stored fallback;
# alphabets of one literal and one length symbol; runs of 2, 3, 258, 259 and 260; segments of one run each.
PIN_CASES = {
    "1x1_rgb": SHAPE_CASES["1x1_rgb"],
    "1x1_grey": SHAPE_CASES["1x1_grey"],
    "7x1_grey": SHAPE_CASES["7x1_grey"],
    "67x173_rgb_blobs": SHAPE_CASES["67x173_rgb_blobs"],
    "67x173_rgb_blobs_white": _blobs(67, 173, 0.9, white=True),
    "40x50_rgb_noise": _rng(41).integers(0, 256, (40, 50, 3), dtype=np.uint8),
    "1x258_zeros": np.zeros((1, 258), np.uint8),
    "1x259_zeros": np.zeros((1, 259), np.uint8),
    "runs": _runs_image(),
    "64x1024_zeros": np.zeros((64, 1024), np.uint8),
}
PIN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode_streams.npz")


def pin_streams(frames):
    """png_gpu.encode_streams on the host: (the packed bytes up to the last stream's end, offsets, lengths)."""
    from deformgs import png_gpu
    packed, offsets, lengths = png_gpu.encode_streams(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    offsets, lengths = offsets.cpu().numpy(), lengths.cpu().numpy()
    return packed[:int(offsets[-1] + lengths[-1])].cpu().numpy(), offsets, lengths


def test_streams_equal_the_recorded_ones():
    """The zlib streams, byte for byte, against those the encoder of the recorded parent revision wrote for the
    same inputs (tests/golden/make_golden_png_encode.py): a change that is meant to leave the bytes alone is held to
    it. Then every shape with more than one case as one batch: its frames' streams are the recorded ones, back to
    back."""
    gold = np.load(PIN_PATH)
    assert sorted(str(c) for c in gold["cases"]) == sorted(PIN_CASES)
    by_shape = {}
    for name, img in PIN_CASES.items():
        packed, offsets, lengths = pin_streams(img[None])
        assert offsets.dtype == lengths.dtype == np.int64
        assert offsets.tolist() == gold[f"{name}_offsets"].tolist() == [0], name
        assert lengths.tolist() == gold[f"{name}_lengths"].tolist(), name
        assert packed.tobytes() == gold[f"{name}_packed"].tobytes(), name
        by_shape.setdefault(img.shape, []).append(name)
    batches = [names for names in by_shape.values() if len(names) > 1]
    assert batches
    for names in batches:
        packed, offsets, lengths = pin_streams(np.stack([PIN_CASES[n] for n in names]))
        want = [gold[f"{n}_packed"].tobytes() for n in names]
        assert lengths.tolist() == [len(w) for w in want], names
        assert offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist(), names
        assert packed.tobytes() == b"".join(want), names


def test_batch_of_five_and_reproducible():
    frames = np.stack([_blobs(67, 173, 0.1), _blobs(67, 173, 0.9, white=True),
                       _rng(31).integers(0, 256, (67, 173, 3), dtype=np.uint8), np.full((67, 173, 3), 9, np.uint8),
                       _blobs(67, 173, 0.5)])
    files = _encode(frames)
    _check(files, frames)
    assert files == _encode(frames)
    for i in range(5):
        assert _encode(frames[i:i + 1])[0] == files[i], i
    grey = np.ascontiguousarray(frames[:, :, :, 0])
    _check(_encode(grey), grey)


@pytest.mark.parametrize("name", ["256x256_rgb_blobs", "256x256_rgb_blobs_white", "67x173_rgb_blobs"])
def test_smooth_rgb_frames_are_no_larger_than_todays_writer(name):
    from deformgs import png
    img = SHAPE_CASES[name]
    new, old = len(_encode(img[None])[0]), len(png.encode_png(img))
    print(f"{name}: device encoder {new} bytes, encode_png {old} bytes")
    assert new <= old


def test_write_frames(tmp_path):
    from deformgs import png, png_gpu
    frames = np.stack([_blobs(20, 30, 0.2), _blobs(20, 30, 0.7)])
    paths = [str(tmp_path / f"{i}.png") for i in range(2)]
    png_gpu.write_frames(paths, torch.from_numpy(frames).cuda())
    for p, img in zip(paths, frames):
        assert np.array_equal(png.read_png(p), img)


def test_refused_inputs():
    from deformgs import png_gpu
    dev = torch.device("cuda")
    with pytest.raises(ValueError):
        png_gpu.encode_frames(torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        png_gpu.encode_frames(torch.zeros((1, 4, 4, 3), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        png_gpu.encode_frames(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        png_gpu.encode_frames(torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        png_gpu.write_frames(["a.png"], torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=dev))
