"""GPU: the HIP image ingest (csrc/ingest.hip) against the numpy path, bit for bit: the unfilter kernel over
sizes that cross its 64-row bands and its 8-pixel look-ahead, every filter type, both pixel sizes and batches;
composite + resize against tests/golden/dataset_ingest.npz; and that exactly the output is written."""
import os

import numpy as np
import pytest
import torch

from conftest import gpu_available
from png_fixtures import encode_png_filtered, filter_scanlines

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

SIZES = [(1, 1), (1, 70), (37, 70), (64, 64), (130, 5), (257, 3)]  # W x H
KINDS = [0, 1, 2, 3, 4, "cycle", "random"]
RESIZE_CASES = [((19, 13), (10, 6)), ((32, 32), (16, 16)), ((24, 40), (12, 20)), ((33, 17), (8, 4)),
                ((16, 16), (16, 8)), ((19, 13), (19, 13))]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dataset_ingest.npz")))


def _types(kind, h, rng):
    if kind == "cycle":
        return [y % 5 for y in range(h)]
    if kind == "random":
        return rng.integers(0, 5, h).tolist()
    return [kind] * h


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bpp", [3, 4])
def test_unfilter_bitwise(size, bpp):
    """All filter kinds and both batch sizes of one (size, bpp) in one test: 14 launches."""
    from deformgs import ingest, png
    W, H = size
    rng = np.random.default_rng(W * 1000 + H * 10 + bpp)
    for kind in KINDS:
        for B in (1, 5):
            px = rng.integers(0, 256, (B, H, W, bpp), dtype=np.uint8)  # different content per image
            types = [_types(kind, H, rng) for _ in range(B)]
            raws = [filter_scanlines(px[i], types[i]) for i in range(B)]
            want = np.stack([png.unfilter(r, W, H, bpp) for r in raws])
            assert np.array_equal(want, px)  # the oracle itself round-trips
            scan = torch.from_numpy(np.frombuffer(b"".join(raws), np.uint8).copy()).cuda()
            got = ingest.unfilter_device(scan, B, W, H, bpp).cpu().numpy()
            assert got.shape == (B, H, W, bpp)
            assert np.array_equal(got, want), (kind, B, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
@pytest.mark.parametrize("white", [False, True])
def test_composite_resize_matches_fixture(fx, case, white):
    from deformgs import ingest
    (W, H), (w, h) = case
    bg = "white" if white else "black"
    rgba = fx[f"rgba_{W}x{H}"]
    items = [encode_png_filtered(rgba, [y % 5 for y in range(H)]), encode_png_filtered(rgba, [4] * H)]
    got, got8 = ingest.ingest_images(items, white, size=(w, h), device="cuda", return_uint8=True)
    want = fx[f"resized_{bg}_{W}x{H}_{w}x{h}"]
    assert got.shape == (2, 3, h, w) and got.dtype == torch.float32 and got.is_cuda
    for i in range(2):
        assert np.array_equal(got[i].cpu().numpy(), want)
    if (w, h) == (W, H):
        assert np.array_equal(got8[0].cpu().numpy(), fx[f"comp_{bg}_{W}x{H}"])
    cpu = ingest.ingest_images(items, white, size=(w, h), device="cpu")
    assert np.array_equal(cpu.numpy(), got.cpu().numpy())


@pytest.mark.parametrize("target", [(10, 6), (19, 13)])
def test_rgb_input_skips_composite(fx, target):
    from deformgs import ingest
    data = encode_png_filtered(fx["rgb_19x13"], [y % 5 for y in range(13)])
    for white in (False, True):
        got = ingest.ingest_images([data], white, size=target, device="cuda")
        assert np.array_equal(got[0].cpu().numpy(), fx[f"resized_rgb_19x13_{target[0]}x{target[1]}"])


def test_mixed_groups_on_device(fx):
    from deformgs import ingest
    a, b = fx["rgba_19x13"], fx["rgb_19x13"]
    items = [encode_png_filtered(a, [1] * 13), encode_png_filtered(b, [2] * 13), encode_png_filtered(a[::-1].copy(), [3] * 13)]
    got = ingest.ingest_images(items, True, size=(10, 6), device="cuda")
    want = ingest.ingest_images(items, True, size=(10, 6), device="cpu")
    assert np.array_equal(got.cpu().numpy(), want.numpy())


@pytest.mark.parametrize("target", [(10, 6), (19, 13)])
def test_isolation_exact_extent_written(fx, target):
    """The float output is a view into a sentinel-filled buffer: exactly B*3*h*w floats change and the guard
    after them stays; the byte stages (unfilter, both resize passes) are checked the same way."""
    from deformgs import _lib, ingest
    lib = _lib.load()
    w, h = target
    W, H, B, guard = 19, 13, 3, 4096
    rgba = fx["rgba_19x13"]
    raws = [filter_scanlines(np.roll(rgba, i, axis=1), [(y + i) % 5 for y in range(H)]) for i in range(B)]
    n = B * 3 * h * w
    buf = torch.full((n + guard,), -7.0, dtype=torch.float32, device="cuda")
    out = buf[:n].view(B, 3, h, w)
    f, _ = ingest.ingest_group_device(raws, W, H, 4, False, (w, h), torch.device("cuda"), out=out)
    assert f.data_ptr() == buf.data_ptr()
    res = buf.cpu().numpy()
    assert np.all(res[n:] == -7.0)
    assert np.all((res[:n] >= 0.0) & (res[:n] <= 1.0))
    want = ingest.ingest_group_numpy(raws, W, H, 4, False, (w, h))[0]
    assert np.array_equal(res[:n].reshape(B, 3, h, w), want)
    # byte stages, each into a guarded buffer through the C ABI
    stream = _lib.stream_ptr(torch.device("cuda"))
    scan = torch.from_numpy(np.frombuffer(b"".join(raws), np.uint8).copy()).cuda()
    lut = torch.from_numpy(ingest.composite_table(False).reshape(-1).copy()).cuda()
    nb = B * H * W * 3
    b8 = torch.full((nb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dgs_ingest_unfilter(B, W, H, 4, _lib.ptr(scan), _lib.ptr(lut), _lib.ptr(b8), stream), "unfilter")
    assert torch.all(b8[nb:] == 0xA5)
    comp = b8[:nb].view(B, H, W, 3)
    assert np.array_equal(comp[0].cpu().numpy(), fx["comp_black_19x13"])
    bounds, coef = ingest.resample_tables(W, 10)
    bd, cd = torch.from_numpy(bounds).cuda(), torch.from_numpy(coef).cuda()
    nh = B * H * 10 * 3
    h8 = torch.full((nh + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dgs_ingest_resample(B * H, W, 10, 3, _lib.ptr(comp), _lib.ptr(bd), _lib.ptr(cd), coef.shape[1],
                                       _lib.ptr(h8), stream), "resample")
    assert torch.all(h8[nh:] == 0xA5)
    assert np.array_equal(h8[:nh].view(B, H, 10, 3).cpu().numpy(), ingest.resample_numpy(comp.cpu().numpy(), 2, 10))


def test_bad_arguments_return_status():
    from deformgs import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    stream = _lib.stream_ptr(torch.device("cuda"))
    assert lib.dgs_ingest_unfilter(1, 2, 2, 5, _lib.ptr(t), None, _lib.ptr(t), stream) == -1
    assert lib.dgs_ingest_unfilter(1, 2, 2, 3, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), stream) == -1  # table needs bpp 4
    assert lib.dgs_ingest_unfilter(1, 9000, 1, 4, _lib.ptr(t), None, _lib.ptr(t), stream) == -3
    assert lib.dgs_ingest_resample(1, 4, 2, 3, _lib.ptr(t), None, None, 5, _lib.ptr(t), stream) == -1
    assert lib.dgs_ingest_to_float(1, 0, 4, _lib.ptr(t), _lib.ptr(t), stream) == -1
