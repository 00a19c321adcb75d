"""CPU: the bars of tests/loss_ref.py are reachable by the fused loss's fp32 arithmetic before any GPU is involved.

The numpy restatement of the kernels (loss_ref.emulate) must sit within loss_ref.bars of the float64 oracle for every
shape, regime and lambda tests/test_gpu_loss_parity.py runs. The bars are relative to E32, the distance of the
reference's own fp32 loss from float64, and not fixed numbers, because E32 depends on the background: on white the
variances E[I^2] - mu^2 cancel at values near 1 against C2 and the reference's fp32 SSIM sits tens of times further
from float64 than on black (asserted below, so this paragraph stays true)."""
import pytest
import torch

import loss_ref as ref


@pytest.mark.parametrize("lam", ref.LAMBDAS)
@pytest.mark.parametrize("regime", ref.REGIMES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_is_within_the_bars(shape, regime, lam):
    H, W, C = shape
    d = ref.case(H, W, C, regime, lam)
    for contract in (False, True):
        got = ref.emulate(d["img"], d["gt"], lam, contract=contract)
        report, failures = ref.compare(got, d["f64"], d["f32"], d["mask"])
        print(f"contract={contract}: {ref.summary(report)}")
        assert not failures, (contract, failures)


def test_scene_regions():
    img, gt, mask = ref.scene(67, 97, 7, "train_white")
    assert img.dtype == gt.dtype == torch.float32 and img.shape == gt.shape == mask.shape == (3, 67, 97)
    bgm = ~mask
    assert mask.any() and bgm.any() and (gt[bgm] == 1.0).all()
    left = bgm & (torch.arange(97) < 48.5).expand(3, 67, 97)
    assert torch.equal(img[left], gt[left])                      # sign term 0
    d = (img - gt)[bgm & ~left]
    assert (d != 0).any() and d.abs().max() <= 3e-4 + 1e-7 and img.max() <= 1.0
    assert (img[mask] != gt[mask]).any()
    b_img, b_gt, _ = ref.scene(67, 97, 7, "train_black")
    assert (b_gt[bgm] == 0.0).all() and b_img.min() >= 0.0
    i_img, i_gt, _ = ref.scene(67, 97, 7, "identical")
    assert torch.equal(i_img, i_gt)
    assert ref.scene(33, 31, 7, "bright", channels=4)[0].max() > 1.0
    assert ref.scene(1, 1, 7, "near")[2].all()                   # a 1 x 1 image is all object: one region


def test_white_background_fp32_error_is_the_references_own():
    """The reference's fp32 SSIM on a near-target render: more than 10x further from float64 on a white background
    than on a black one."""
    e32 = {}
    for bg in (1.0, 0.0):
        img, gt, _ = ref.scene(67, 97, ref.seed_of(67, 97, 3), "near", bg=bg)
        e32[bg] = abs(ref.oracle(img, gt, 0.2, torch.float32)[2] - ref.oracle(img, gt, 0.2, torch.float64)[2])
    print(f"E32(SSIM) white {e32[1.0]:.3e}, black {e32[0.0]:.3e}")
    assert e32[1.0] > 10 * e32[0.0]
