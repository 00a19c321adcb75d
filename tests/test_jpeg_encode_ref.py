"""CPU: the numpy restatement of the JPEG encoder (tests/jpeg_encode_ref.py) against PIL / libjpeg-turbo
(tests/golden/jpeg_encode.npz): the quantisation tables and the quantised coefficients, dummy blocks included, are
PIL's exactly, and the restatement's file decodes (deformgs.jpeg, and PIL where installed) to PIL's pixels exactly."""
import io

import numpy as np
import pytest

import jpeg_encode_ref as ref
from jpeg_encode_cases import GOLD, GROUPS, golden, group, ref_file, source


@pytest.mark.parametrize("quality", [25, 75, 90, 100])
def test_quantisation_tables_are_pils(quality):
    assert np.array_equal(ref.quant_tables(quality), GOLD[f"qt_q{quality}"])


def test_quality_100_tables_are_all_ones_and_1_is_clamped():
    assert np.all(ref.quant_tables(100) == 1)
    assert ref.quant_tables(1).max() == 255


@pytest.mark.parametrize("name", GROUPS)
def test_coefficients_are_pils(name):
    size, sampling, quality, contents = group(name)
    qt = ref.quant_tables(quality)
    for kind in contents:
        want = golden(name, kind, "coef")
        got = ref.coefficients(source(size, kind), qt, *ref.SAMPLING[sampling])
        assert got.dtype == np.int16 and got.shape == want.shape, (kind, got.shape, want.shape)
        assert np.array_equal(got, want), (kind, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("name", GROUPS)
def test_file_decodes_to_pils_pixels(name):
    from deformgs import jpeg
    size, sampling, quality, contents = group(name)
    for kind in contents:
        data = ref_file(name, kind)
        hd = jpeg.parse_header(data)
        assert hd.restart == hd.mcus_w and (hd.hs, hd.vs) == ref.SAMPLING[sampling]
        assert np.array_equal(jpeg.decode_coefficients(data, hd), golden(name, kind, "coef")), kind
        assert np.array_equal(jpeg.decode_jpeg(data), golden(name, kind, "pix")), kind


def test_restart_counter_wraps_past_rst7():
    for name in ("8x80_444_q75", "24x150_420_q75"):
        data = ref_file(name, "gradient")
        marks = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
        assert marks == [0xD0 + (k & 7) for k in range(9)]


def test_hf_pattern_has_zrl_runs_and_blocks_without_eob():
    """Coefficient 63 alone (besides the DC): three ZRL, then run 14 into the last position, and no EOB."""
    coef = golden("16x16_444_q90", "hf", "coef")
    luma = coef[:4]
    assert np.all(luma[:, 63] != 0) and np.all(luma[:, 1:63] == 0)


def test_quality_100_reaches_the_longest_categories_and_noise_stuffs():
    coef = golden("33x31_444_q100", "square", "coef").astype(np.int64)
    assert np.abs(coef[:, 1:]).max() >= 512  # AC category 10
    dc = golden("33x31_444_q100", "blocks", "coef").astype(np.int64)[:20, 0]
    assert np.abs(np.diff(dc)).max() >= 1024  # DC differences of category 11
    data = ref_file("33x31_444_q100", "noise")
    from deformgs import jpeg
    scan = data[jpeg.parse_header(data).scan_offset:]
    assert b"\xff\x00" in scan


@pytest.mark.parametrize("name", GROUPS)
def test_pil_opens_the_file_to_the_same_pixels(name):
    Image = pytest.importorskip("PIL.Image")
    size, sampling, quality, contents = group(name)
    for kind in contents:
        got = np.asarray(Image.open(io.BytesIO(ref_file(name, kind))).convert("RGB"))
        assert np.array_equal(got, golden(name, kind, "pix")), kind
