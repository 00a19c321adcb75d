"""CPU: the float64 restatement of PSNR / SSIM / MS-SSIM (tests/ms_ssim_ref.py) against closed forms, and the
argument handling of deformgs.image_metrics and of the metrics script that needs no GPU."""
import math

import pytest
import torch

import ms_ssim_ref as ref


def test_identical_images_give_one_at_every_level():
    img, _ = ref.pattern_pair(161, 163, seed=3)
    x = img.unsqueeze(0)
    ms, levels = ref.ms_ssim(x, x)
    # x*y == x*x bit for bit, so 2 s12 + C2 and s11 + s22 + C2 are the same number
    assert torch.equal(levels, torch.ones_like(levels))
    assert ms.item() == 1.0
    assert ref.ssim(x, x).item() == pytest.approx(1.0, abs=1e-15)
    assert ref.psnr(x, x)[0].item() == math.inf


def test_constant_images_closed_form():
    # even sides down to level 4 (176 -> 88 -> 44 -> 22 -> 11, 192 -> ... -> 12): no pool pads, so every
    # level is the same pair of constants and cs_l = C2 / C2
    a, b = 0.3, 0.8
    x = torch.full((1, 3, 176, 192), a, dtype=torch.float64)
    y = torch.full((1, 3, 176, 192), b, dtype=torch.float64)
    ms, levels = ref.ms_ssim(x, y)
    lum = (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)
    assert torch.allclose(levels[:, 0], torch.ones(1, 5, 3, dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(levels[:, 1], torch.full((1, 5, 3), lum, dtype=torch.float64), rtol=0, atol=1e-12)
    assert ms.item() == pytest.approx(lum ** 0.1333, abs=1e-12)
    assert ref.psnr(x, y)[1].item() == pytest.approx((a - b) ** 2, rel=1e-14)
    assert ref.psnr(x, y)[0].item() == pytest.approx(-20 * math.log10(abs(a - b)), rel=1e-14)


def test_anticorrelated_pair_is_exactly_zero():
    img, _ = ref.pattern_pair(161, 163, seed=5)
    x = img.unsqueeze(0)
    ms, levels = ref.ms_ssim(x, 1.0 - x)
    assert (levels[0, 0].min(0).values < 0).all()  # every channel has a negative cs at some level
    assert ms.item() == 0.0


def test_pooled_sizes():
    assert ref.pooled_sizes(161, 163) == [(161, 163), (81, 82), (41, 41), (21, 21), (11, 11)]
    x = torch.rand(1, 1, 161, 163, dtype=torch.float64)
    for (h, w), (ph, pw) in zip(ref.pooled_sizes(161, 163), ref.pooled_sizes(161, 163)[1:]):
        x = torch.nn.functional.avg_pool2d(x, 2, 2, padding=[h % 2, w % 2])
        assert tuple(x.shape[-2:]) == (ph, pw)


def test_pool_counts_the_padded_zeros():
    x = torch.ones(1, 1, 161, 163, dtype=torch.float64)
    p = torch.nn.functional.avg_pool2d(x, 2, 2, padding=[1, 1])
    assert p[0, 0, 0, 0].item() == 0.25 and p[0, 0, 0, 1].item() == 0.5 and p[0, 0, 1, 1].item() == 1.0
    assert p[0, 0, -1, -1].item() == 1.0  # an odd side ends on a full window: only the leading pad is read


def test_size_rule():
    x = torch.rand(1, 1, 160, 200, dtype=torch.float64)
    with pytest.raises(ValueError, match="160"):
        ref.ms_ssim(x, x)
    x = torch.rand(1, 1, 161, 161, dtype=torch.float64)
    assert ref.ms_ssim(x, x)[0].item() == 1.0


def test_ssim_restates_the_loss_mirror():
    """The float64 SSIM is deformgs.loss.ssim (the reference's, pinned by tests/golden/loss.npz) up to fp32."""
    from deformgs.loss import ssim as mirror
    img, gt = ref.pattern_pair(40, 52, seed=2)
    assert ref.ssim(img[None], gt[None]).item() == pytest.approx(mirror(img[None], gt[None]).item(), abs=2e-6)


def test_image_metrics_argument_errors():
    from deformgs.image_metrics import image_metrics
    x = torch.rand(2, 3, 161, 163)
    with pytest.raises(ValueError, match="CPU"):
        image_metrics(x, x)
    with pytest.raises(ValueError, match="lpips"):
        image_metrics(x, x, metrics=("psnr", "lpips"))
    with pytest.raises(ValueError):
        image_metrics(x, x, metrics=())
    with pytest.raises(ValueError, match="shape"):
        image_metrics(x, x[:, :, :-1])
    with pytest.raises(ValueError, match="sizes"):
        image_metrics([x[0], x[1, :, :-1]], [x[0], x[1, :, :-1]])


def test_script_parsers_accept_the_flags():
    from deformgs import metrics, train
    assert metrics.build_parser().parse_args(["-m", "out", "--ms_ssim"]).ms_ssim is True
    assert metrics.build_parser().parse_args(["-m", "out"]).ms_ssim is False
    assert train.build_parser().parse_args(["--report_ms_ssim"]).report_ms_ssim is True
    assert train.build_parser().parse_args([]).report_ms_ssim is False
