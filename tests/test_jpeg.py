"""CPU: the pure-Python JPEG decoder (deformgs/jpeg.py) and the CPU path of ingest_images on JPEG files against
tests/golden/jpeg_ingest.npz: PIL's own decode (libjpeg-turbo 3.1.4) and the reference's PILtoTorch, recorded by
tests/golden/make_golden_colmap.py. Everything is compared bitwise: libjpeg's default decoder is integer
arithmetic. No PIL and no libdgs_hip.so here."""
import os

import numpy as np
import pytest

from deformgs import ingest, jpeg
from png_fixtures import disc_image, encode_png_filtered

_GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ingest.npz"))
CASES = [str(c) for c in _GOLD["cases"]]
HALVED = [c for c in CASES if f"{c}_half" in _GOLD.files]
REASONS = {"progressive": "progressive", "grayscale": "grayscale", "cmyk": "CMYK"}


def _jpg(name):
    return _GOLD[f"{name}_jpg"].tobytes()


def test_the_fixture_holds_the_cases_the_decoder_can_go_wrong_on():
    assert len(CASES) == 32 and len(HALVED) == 7 and sorted(_GOLD["refusals"]) == sorted(REASONS)
    sampling = {c: (jpeg.parse_header(_jpg(c)).hs, jpeg.parse_header(_jpg(c)).vs) for c in CASES}
    assert {sampling[f"d44x28_{s}"] for s in ("420", "422", "444")} == {(2, 2), (2, 1), (1, 1)}
    assert [jpeg.parse_header(_jpg(f"n{w}x3_420")).width for w in range(1, 7)] == list(range(1, 7))
    assert jpeg.parse_header(_jpg("rst_blocks1_420")).restart == 1 and jpeg.parse_header(_jpg("rst_rows1_420")).restart == 3
    assert len(_jpg("exif_420")) > 20000
    # saturating blocks: the quality-100 noise reaches both ends of the range
    assert _GOLD["noise_q100_444_rgb"].min() == 0 and _GOLD["noise_q100_444_rgb"].max() == 255
    assert str(_GOLD["libjpeg_turbo_version"]).startswith("3.1.4")


@pytest.mark.parametrize("case", CASES)
def test_decode_equals_pil(case):
    got = jpeg.decode_jpeg(_jpg(case))
    want = _GOLD[f"{case}_rgb"]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), (case, int((got != want).sum()))


def test_header_fields():
    hd = jpeg.parse_header(_jpg("d44x28_420"))
    assert (hd.width, hd.height, hd.hs, hd.vs) == (44, 28, 2, 2)
    assert hd.blocks == [(6, 4), (3, 2), (3, 2)] and hd.total_blocks == 36  # padded to 3 x 2 MCUs of 16 x 16
    assert hd.qt.shape == (3, 64) and hd.qt.dtype == np.uint16 and np.array_equal(hd.qt[1], hd.qt[2])
    assert not np.array_equal(hd.qt[0], hd.qt[1]) and hd.qt.min() >= 1
    assert jpeg.parse_header(_jpg("d44x28_422")).blocks == [(6, 4), (3, 4), (3, 4)]
    assert jpeg.parse_header(_jpg("d44x28_444")).blocks == [(6, 4)] * 3
    coef = jpeg.decode_coefficients(_jpg("d44x28_420"))
    assert coef.shape == (36, 64) and coef.dtype == np.int16


@pytest.mark.parametrize("case", CASES)
def test_cpu_ingest_at_native_size_equals_piltotorch(case):
    f, u = ingest.ingest_images([_jpg(case)], False, device="cpu", return_uint8=True)
    want = _GOLD[f"{case}_rgb"]
    assert np.array_equal(u[0].numpy(), want)
    # PILtoTorch at the file's size: the uint8 tensor / 255.0
    assert f.dtype.is_floating_point and np.array_equal(f[0].numpy(), want.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))


@pytest.mark.parametrize("case", HALVED)
def test_cpu_ingest_at_half_size_equals_piltotorch(case):
    want = _GOLD[f"{case}_half"]
    size = (want.shape[2], want.shape[1])
    for white in (False, True):  # no alpha: the background must not matter
        f = ingest.ingest_images([_jpg(case)], white, size=size, device="cpu")
        assert f.shape == (1,) + want.shape and f.numpy().tobytes() == want[None].tobytes()
    h = _GOLD[f"{case}_rgb"].shape
    f2 = ingest.ingest_images([_jpg(case)], False, size=lambda w, hh: (max(w // 2, 1), max(hh // 2, 1)), device="cpu")
    assert (h[1] // 2, h[0] // 2) == size and np.array_equal(f2.numpy(), want[None])


def test_batch_of_four_qualities_in_one_group():
    files = [_jpg(f"batch{k}_420") for k in range(4)]
    assert len({jpeg.parse_header(d).qt.tobytes() for d in files}) == 4  # four different tables
    f, u = ingest.ingest_images(files, False, device="cpu", return_uint8=True)
    assert np.array_equal(u.numpy(), np.stack([_GOLD[f"batch{k}_420_rgb"] for k in range(4)]))


@pytest.mark.parametrize("name", sorted(REASONS))
def test_refusals_name_their_reason(name):
    data = _GOLD[f"refuse_{name}_jpg"].tobytes()
    for fn in (jpeg.decode_jpeg, lambda d: ingest.ingest_images([d], False, device="cpu")):
        with pytest.raises(ValueError, match=f"{REASONS[name]}.*unsupported"):
            fn(data)


def _patched(data, find, replace):
    k = data.index(find)
    return data[:k] + replace + data[k + len(find):]


def test_other_refusals():
    base = _jpg("d44x28_420")
    sof = base[base.index(b"\xff\xc0"):][:19]
    assert sof[4] == 8 and sof[9] == 3
    with pytest.raises(ValueError, match="12-bit.*unsupported"):
        jpeg.decode_jpeg(_patched(base, sof, sof[:4] + b"\x0c" + sof[5:]))
    with pytest.raises(ValueError, match="arithmetic.*unsupported"):
        jpeg.decode_jpeg(_patched(base, sof, b"\xff\xc9" + sof[2:]))
    with pytest.raises(ValueError, match="lossless.*unsupported"):
        jpeg.decode_jpeg(_patched(base, sof, b"\xff\xc3" + sof[2:]))
    # luma 1x2 (4:4:0) and chroma 2x1: other sampling layouts
    with pytest.raises(ValueError, match="sampling layout 1x2, 1x1, 1x1 is unsupported"):
        jpeg.decode_jpeg(_patched(base, sof, sof[:11] + b"\x12" + sof[12:]))
    with pytest.raises(ValueError, match="sampling layout.*unsupported"):
        jpeg.decode_jpeg(_patched(base, sof, sof[:14] + b"\x21" + sof[15:]))
    # an Adobe marker with transform 0 and no JFIF marker: RGB stored directly
    k = base.index(b"\xff\xe0")
    n = int.from_bytes(base[k + 2:k + 4], "big")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    with pytest.raises(ValueError, match="Adobe transform 0.*unsupported"):
        jpeg.decode_jpeg(base[:k] + adobe + base[k + 2 + n:])
    ycc = jpeg.decode_jpeg(base[:k] + adobe[:-1] + b"\x01" + base[k + 2 + n:])  # transform 1: YCbCr, no JFIF marker
    assert np.array_equal(ycc, _GOLD["d44x28_420_rgb"])
    assert np.array_equal(jpeg.decode_jpeg(base[:k] + base[k + 2 + n:]), _GOLD["d44x28_420_rgb"])  # no marker at all
    # a scan of one component: a non-interleaved file
    sos = base[base.index(b"\xff\xda"):][:14]
    with pytest.raises(ValueError, match="non-interleaved.*unsupported"):
        jpeg.decode_jpeg(_patched(base, sos, b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"))
    with pytest.raises(ValueError, match="PNG or JPEG"):
        ingest.ingest_images([b"GIF89a" + bytes(32)], False, device="cpu")


@pytest.mark.parametrize("case", ["d44x28_420", "rst_blocks1_420", "opt_420", "n5x3_422"])
def test_truncated_files_raise(case):
    data = _jpg(case)
    for cut in range(len(data)):
        with pytest.raises(ValueError):
            jpeg.decode_jpeg(data[:cut])
    for cut in (2, len(data) // 2, len(data) - 2, len(data) - 1):  # the last: a missing EOI
        with pytest.raises(ValueError):
            ingest.ingest_images([data[:cut]], False, device="cpu")
    with pytest.raises(ValueError, match="EOI"):
        jpeg.decode_jpeg(data[:-2])


def test_corrupt_entropy_data_raises():
    data = _jpg("d44x28_420")
    hd = jpeg.parse_header(data)
    # the height halved in the frame header: entropy data is left over; doubled: it ends early
    sof = data.index(b"\xff\xc0")
    for h, what in ((12, "left over"), (60, "ends early")):
        bad = data[:sof + 5] + h.to_bytes(2, "big") + data[sof + 7:]
        with pytest.raises(ValueError, match=what):
            jpeg.decode_jpeg(bad)
    # a restart marker where none belongs
    mid = hd.scan_offset + 40
    with pytest.raises(ValueError):
        jpeg.decode_jpeg(data[:mid] + b"\xff\xd0" + data[mid:])
    # every Huffman code of the DC table removed but one: most codes of the data are bad now
    with pytest.raises(ValueError):
        jpeg.decode_jpeg(data[:hd.scan_offset] + b"\xff\x00" * 64 + data[hd.scan_offset:])


def test_mixed_png_and_jpeg_keep_input_order(tmp_path):
    rgb = np.ascontiguousarray(disc_image(44, 28, 0.4)[:, :, :3])
    rgba = disc_image(44, 28, 0.5)
    png3, png4 = encode_png_filtered(rgb, [y % 5 for y in range(28)]), encode_png_filtered(rgba, [4] * 28)
    items = [_jpg("d44x28_420"), png3, _jpg("d44x28_444"), png4, _jpg("batch1_420"), _jpg("d44x28_422")]
    f, u = ingest.ingest_images(items, True, device="cpu", return_uint8=True)
    assert f.shape == (6, 3, 28, 44)
    for k, name in ((0, "d44x28_420"), (2, "d44x28_444"), (4, "batch1_420"), (5, "d44x28_422")):
        assert np.array_equal(u[k].numpy(), _GOLD[f"{name}_rgb"])
    assert np.array_equal(u[1].numpy(), rgb)
    assert np.array_equal(u[3].numpy(), ingest.composite_numpy(rgba, True))
    assert np.array_equal(f.numpy(), u.numpy().transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    # the signature decides, not the name; and a halved mixed batch reaches one size
    p = tmp_path / "really_a_jpeg.png"
    p.write_bytes(_jpg("d44x28_420"))
    q = tmp_path / "really_a_png.jpg"
    q.write_bytes(png3)
    g = ingest.ingest_images([str(p), str(q)], False, size=(22, 14), device="cpu")
    assert np.array_equal(g[0].numpy(), _GOLD["d44x28_420_half"])
    assert np.array_equal(g[1].numpy(), ingest.ingest_images([png3], False, size=(22, 14), device="cpu")[0].numpy())
    with pytest.raises(ValueError, match="different sizes"):
        ingest.ingest_images([_jpg("d44x28_420"), _jpg("d17x17_420")], False, device="cpu")


def test_image_size_reads_the_frame_header(tmp_path):
    from deformgs import dataset
    p = tmp_path / "a.jpg"
    p.write_bytes(_jpg("d33x19_420"))
    assert dataset.jpeg_size(str(p)) == (33, 19) == dataset.image_size(str(p))
    e = tmp_path / "e.jpg"
    e.write_bytes(_jpg("exif_420"))  # EXIF orientation 6 is ignored, as Image.open ignores it
    assert dataset.image_size(str(e)) == (44, 28) and _GOLD["exif_420_rgb"].shape == (28, 44, 3)
    q = tmp_path / "b.png"
    q.write_bytes(encode_png_filtered(np.zeros((5, 7, 3), np.uint8), [0] * 5))
    assert dataset.image_size(str(q)) == (7, 5)
    bad = tmp_path / "c.jpg"
    bad.write_bytes(_GOLD["refuse_progressive_jpg"].tobytes())
    with pytest.raises(ValueError, match="c.jpg.*progressive"):
        dataset.jpeg_size(str(bad))
