"""GPU: the device JPEG encoder (csrc/jpeg_encode.hip behind deformgs.jpeg_gpu) against the numpy restatement
(tests/jpeg_encode_ref.py, itself pinned to PIL by tests/test_jpeg_encode_ref.py): every file byte for byte, a batch
against its frames one by one, the round trip through the device decoder to PIL's pixels, the output capacity, the
refused inputs and reproducibility."""
import numpy as np
import pytest
import torch

from conftest import gpu_available
from jpeg_encode_cases import GROUPS, golden, group, ref_file, source

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


def _stack(name):
    size, sampling, quality, contents = group(name)
    frames = np.stack([source(size, kind) for kind in contents])
    return torch.from_numpy(frames).cuda(), sampling, quality, contents


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = [i for i in range(n) if a[i] != b[i]][:1]
    return (len(a), len(b), d[0] if d else n)


@pytest.mark.parametrize("name", GROUPS)
def test_files_equal_the_restatement_and_round_trip(name):
    """One call for all the contents of a size (different lengths: offsets, lengths, independence of frames), then
    each frame alone; the files through the device decoder give PIL's decode of PIL's file."""
    from deformgs import ingest, jpeg_gpu
    frames, sampling, quality, contents = _stack(name)
    files = jpeg_gpu.encode_frames(frames, quality=quality, subsampling=sampling)
    assert len(files) == len(contents)
    for i, kind in enumerate(contents):
        want = ref_file(name, kind)
        assert isinstance(files[i], bytes)
        assert files[i] == want, (kind, _first_difference(files[i], want))
        alone = jpeg_gpu.encode_frames(frames[i:i + 1], quality=quality, subsampling=sampling)
        assert alone == [want], (kind, "alone")
    _, u = ingest.ingest_images(files, False, device="cuda", return_uint8=True)
    got = u.cpu().numpy()
    for i, kind in enumerate(contents):
        assert np.array_equal(got[i], golden(name, kind, "pix")), kind


def test_capacity_too_small_flags_the_frames_and_writes_nothing_past_it():
    """33x31 at quality 100, 4:4:4: the noise frame is the first and by far the longest. With room for less than
    it, every frame is flagged and nothing at all is written; with room for the first two frames, those two are
    there and the rest is flagged. The lengths are the true ones both times; the bytes behind the capacity keep
    their fill. encode_frames given the same small capacity repeats the call and returns the right files."""
    from deformgs import jpeg_gpu
    name = "33x31_444_q100"
    frames, sampling, quality, contents = _stack(name)
    assert contents[0] == "noise"
    full, offsets, lengths, flags = jpeg_gpu.encode_streams(frames, quality, sampling)
    offsets, lengths = offsets.cpu().numpy(), lengths.cpu().numpy()
    assert not flags.cpu().numpy().any()
    assert offsets[0] == 0 and np.array_equal(offsets[1:], np.cumsum(lengths)[:-1])
    total = int(offsets[-1] + lengths[-1])
    full = full[:total].cpu().numpy()
    guard = 256
    for fit in (0, 2):
        cap = int(lengths[0]) - 1 if fit == 0 else int(offsets[2]) + 3
        buf = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        out, o2, l2, f2 = jpeg_gpu.encode_streams(frames, quality, sampling, capacity=cap, out=buf)
        assert out is buf
        assert np.array_equal(o2.cpu().numpy(), offsets) and np.array_equal(l2.cpu().numpy(), lengths)
        assert f2.cpu().numpy().tolist() == [0] * fit + [1] * (len(contents) - fit)
        got = buf.cpu().numpy()
        written = int(offsets[fit]) if fit else 0
        assert np.array_equal(got[:written], full[:written])
        assert np.all(got[written:] == 0xA5), "bytes outside the frames that fit were written"
    files = jpeg_gpu.encode_frames(frames, quality, sampling, capacity=int(lengths[0]) - 1)
    assert files == [ref_file(name, kind) for kind in contents]


def test_default_capacity_is_exceeded_by_noise_and_retried():
    """Noise at quality 100 and 4:4:4 takes more than the 1.5 bytes a pixel + 1024 a frame of the first attempt once
    the frame is large enough: 96x96."""
    from deformgs import jpeg_gpu
    rgb = np.random.default_rng(7).integers(0, 256, (2, 96, 96, 3), dtype=np.uint8)
    frames = torch.from_numpy(rgb).cuda()
    _, offsets, lengths, flags = jpeg_gpu.encode_streams(frames, 100, "4:4:4")
    assert int(lengths.sum()) > 2 * (96 * 96 * 3 // 2 + 1024) and flags.cpu().numpy().tolist() == [1, 1]
    files = jpeg_gpu.encode_frames(frames, 100, "4:4:4")
    import jpeg_encode_ref as ref
    assert files == [ref.encode(rgb[i], 100, "4:4:4") for i in range(2)]


def test_more_than_one_round_of_blocks_in_a_segment():
    """200x40 at 4:2:0: 13 MCUs x 6 blocks = 78 blocks a row, under the 128 of one round; 520x24 at 4:4:4: 65 x 3 =
    195 blocks, two rounds with bits of an unfinished byte carried between them; 700x17 at 4:2:0: 44 x 6 = 264, three."""
    from deformgs import jpeg_gpu
    import jpeg_encode_ref as ref
    rng = np.random.default_rng(11)
    for (h, w), sampling, quality in (((40, 200), "4:2:0", 90), ((24, 520), "4:4:4", 100), ((17, 700), "4:2:0", 75)):
        rgb = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        rgb[1] = (np.arange(w)[None, :, None] * 3 + np.arange(h)[:, None, None] * 5) % 256
        files = jpeg_gpu.encode_frames(torch.from_numpy(rgb).cuda(), quality, sampling)
        for i in range(2):
            want = ref.encode(rgb[i], quality, sampling)
            assert files[i] == want, (h, w, i, _first_difference(files[i], want))


def test_two_calls_give_identical_bytes():
    from deformgs import jpeg_gpu
    frames, sampling, quality, _ = _stack("33x31_420_q90")
    assert jpeg_gpu.encode_frames(frames, quality, sampling) == jpeg_gpu.encode_frames(frames, quality, sampling)


def test_write_frames(tmp_path):
    from deformgs import jpeg, jpeg_gpu
    frames, sampling, quality, contents = _stack("17x9_422_q75")
    paths = [str(tmp_path / f"{i}.jpg") for i in range(len(contents))]
    jpeg_gpu.write_frames(paths, frames, quality=quality, subsampling=sampling)
    for p, kind in zip(paths, contents):
        assert np.array_equal(jpeg.read_jpeg(p), golden("17x9_422_q75", kind, "pix"))


def test_refused_inputs():
    from deformgs import jpeg_gpu
    dev = torch.device("cuda")
    ok = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="CPU tensor"):
        jpeg_gpu.encode_frames(ok.cpu())
    with pytest.raises(ValueError, match="uint8"):
        jpeg_gpu.encode_frames(ok.float())
    with pytest.raises(ValueError, match="grey"):
        jpeg_gpu.encode_frames(ok[..., 0])
    for q in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            jpeg_gpu.encode_frames(ok, quality=q)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg_gpu.encode_frames(ok, subsampling="4:1:1")
    with pytest.raises(ValueError, match="65535"):
        jpeg_gpu.encode_frames(torch.zeros((1, 1, 65536, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        jpeg_gpu.write_frames(["a.jpg"], torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=dev))


def test_c_entry_refuses_bad_arguments():
    from deformgs import _lib
    lib = _lib.load()
    assert lib.dgs_jpeg_encode_scratch_bytes(1, 8, 8, 2, 2) > 0
    for args in ((0, 8, 8, 2, 2), (1, 0, 8, 2, 2), (1, 8, 65536, 2, 2), (1, 8, 8, 1, 2), (1, 8, 8, 4, 1)):
        assert lib.dgs_jpeg_encode_scratch_bytes(*args) == 0, args
    dev = torch.device("cuda")
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros(4096, dtype=torch.uint8, device=dev)
    where = torch.zeros((2, 1), dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.zeros(4096 + 16, dtype=torch.uint8, device=dev)
    qt = np.ones((2, 64), np.uint16)

    def call(q=qt, s=scratch, hs=2):
        return lib.dgs_jpeg_encode(1, 8, 8, hs, 2, _lib.ptr(frames), q.ctypes.data, _lib.ptr(out), 4096, _lib.ptr(where[0]),
                                   _lib.ptr(where[1]), _lib.ptr(flags), _lib.ptr(s), _lib.stream_ptr(dev))
    assert call() == 0
    zero = qt.copy()
    zero[1, 63] = 0
    assert call(q=zero) == -1
    assert call(s=scratch[1:]) == -1
    assert call(hs=3) == -1
    torch.cuda.synchronize()
