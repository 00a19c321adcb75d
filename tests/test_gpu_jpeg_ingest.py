"""GPU: JPEG ingest on the device (csrc/jpeg.hip behind ingest_images) against tests/golden/jpeg_ingest.npz: PIL's
decode (libjpeg-turbo 3.1.4) and the reference's PILtoTorch, bitwise; the C++ front end's coefficients against
deformgs/jpeg.py's; batch indexing."""
import os

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

_GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ingest.npz"))
CASES = [str(c) for c in _GOLD["cases"]]
HALVED = [c for c in CASES if f"{c}_half" in _GOLD.files]


def _jpg(name):
    return _GOLD[f"{name}_jpg"].tobytes()


@pytest.mark.parametrize("case", CASES)
def test_device_ingest_equals_pil(case):
    from deformgs import ingest
    want = _GOLD[f"{case}_rgb"]
    f, u = ingest.ingest_images([_jpg(case)], False, device="cuda", return_uint8=True)
    assert f.is_cuda and u.is_cuda and u.dtype == torch.uint8 and f.dtype == torch.float32
    got = u[0].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (case, int((got != want).sum()))
    assert np.array_equal(f[0].cpu().numpy(), want.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))
    if case in HALVED:
        half = _GOLD[f"{case}_half"]
        for white in (False, True):
            h = ingest.ingest_images([_jpg(case)], white, size=(half.shape[2], half.shape[1]), device="cuda")
            assert h.cpu().numpy().tobytes() == half[None].tobytes()


def test_batch_of_four_qualities_in_one_group():
    from deformgs import ingest
    files = [_jpg(f"batch{k}_420") for k in range(4)]
    f, u = ingest.ingest_images(files, False, device="cuda", return_uint8=True)
    want = np.stack([_GOLD[f"batch{k}_420_rgb"] for k in range(4)])
    assert np.array_equal(u.cpu().numpy(), want)
    assert np.array_equal(f.cpu().numpy(), want.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    h = ingest.ingest_images(files, False, size=(22, 14), device="cuda")
    assert np.array_equal(h[2].cpu().numpy(), _GOLD["batch2_420_half"])
    cpu = ingest.ingest_images(files, False, size=(22, 14), device="cpu")
    assert torch.equal(h.cpu(), cpu)


@pytest.mark.parametrize("case", CASES)
def test_cpp_front_end_equals_the_python_one(case):
    from deformgs import ingest, jpeg
    data = _jpg(case)
    info = ingest.jpeg_header_native(data)
    hd = jpeg.parse_header(data)
    assert (info.width, info.height, info.hs, info.vs) == (hd.width, hd.height, hd.hs, hd.vs)
    assert [(info.blocks_w[c], info.blocks_h[c]) for c in range(3)] == hd.blocks
    assert np.array_equal(np.ctypeslib.as_array(info.qt).reshape(3, 64), hd.qt)
    got = ingest.jpeg_coefficients_native(data)
    want = jpeg.decode_coefficients(data)
    assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)


def test_cpp_front_end_refuses_what_the_python_one_refuses():
    from deformgs import ingest
    for name, reason in (("progressive", "progressive"), ("grayscale", "grayscale"), ("cmyk", "CMYK")):
        with pytest.raises(ValueError, match=f"{reason}.*unsupported"):
            ingest.ingest_images([_GOLD[f"refuse_{name}_jpg"].tobytes()], False, device="cuda")
    data = _jpg("d44x28_420")
    for cut in (2, 300, len(data) // 2, len(data) - 2):
        with pytest.raises(ValueError):
            ingest.ingest_images([data[:cut]], False, device="cuda")
    with pytest.raises(ValueError, match="EOI"):
        ingest.jpeg_coefficients_native(data[:-2])


def test_three_image_group_equals_three_single_calls():
    """Batch indexing: images 1 and 2 of a group start at a block count (3 x 2 MCUs: 36 blocks, not a multiple of
    the 32 blocks of a workgroup) into the coefficient buffer and the planes."""
    from deformgs import ingest
    files = [_jpg(n) for n in ("d33x19_420", "d33x19b_420", "d33x19c_420")]
    f, u = ingest.ingest_images(files, False, device="cuda", return_uint8=True)
    assert u.shape == (3, 19, 33, 3)
    for k, d in enumerate(files):
        f1, u1 = ingest.ingest_images([d], False, device="cuda", return_uint8=True)
        assert torch.equal(u[k], u1[0]) and torch.equal(f[k], f1[0])
    cpu = ingest.ingest_images(files, False, device="cpu", return_uint8=True)[1]
    assert torch.equal(u.cpu(), cpu)
    assert not torch.equal(u[0], u[1]) and not torch.equal(u[1], u[2])


def test_mixed_png_and_jpeg_on_the_device():
    from deformgs import ingest
    from png_fixtures import disc_image, encode_png_filtered
    rgba = disc_image(44, 28, 0.5)
    items = [_jpg("d44x28_420"), encode_png_filtered(rgba, [4] * 28), _jpg("d44x28_444"), _jpg("batch1_420")]
    f, u = ingest.ingest_images(items, True, device="cuda", return_uint8=True)
    c, cu = ingest.ingest_images(items, True, device="cpu", return_uint8=True)
    assert torch.equal(u.cpu(), cu) and torch.equal(f.cpu(), c)
    assert np.array_equal(u[3].cpu().numpy(), _GOLD["batch1_420_rgb"])
