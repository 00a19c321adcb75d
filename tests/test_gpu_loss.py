"""Fused HIP L1+SSIM (dgs_l1_ssim_*) vs the reference's own loss (golden) and the torch mirror.
Tolerance: loss / L1 / SSIM values to 1e-6 abs (2e-6 against the torch mirror); dL/dimg to 1e-5 relative to its max
(fp32 sums in a different order than the mirror's conv). These fixed bars hold for the inputs of this file only (the
golden pair, uniform noise): on a render close to a target on a white background the reference's own fp32 SSIM is
already 1e-5 from float64. tests/test_gpu_loss_parity.py covers that regime with bars relative to that error, per
region, against float64."""
import numpy as np
import pytest
import torch

from deformgs.loss import l1_loss, l1_ssim_loss, ssim

pytestmark = pytest.mark.gpu


def test_fused_loss_golden(golden_dir):
    f = np.load(f"{golden_dir}/loss.npz")
    img = torch.from_numpy(f["img1"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(f["img2"]).cuda()
    loss, l1, s = l1_ssim_loss(img, gt, 0.2)
    assert abs(l1.item() - float(f["l1"])) < 1e-6
    assert abs(s.item() - float(f["ssim"])) < 1e-6
    assert abs(loss.item() - float(f["loss"])) < 1e-6
    loss.backward()
    g = img.grad.cpu().numpy()
    assert np.abs(g - f["grad"]).max() <= 1e-5 * np.abs(f["grad"]).max()


@pytest.mark.parametrize("shape", [(3, 800, 800), (3, 61, 83), (1, 16, 16), (3, 5, 200)])
def test_fused_loss_vs_torch(shape):
    # the torch mirror runs on the CPU: on the GPU its conv2d goes through MIOpen, whose 1-channel
    # backward once aborted the whole test process on a fresh box (r4v); the HIP loss is what is tested
    torch.manual_seed(0)
    a = torch.rand(shape)
    b = torch.rand(shape)
    x1 = a.clone().requires_grad_(True)
    ref = 0.8 * l1_loss(x1, b) + 0.2 * (1.0 - ssim(x1, b))
    (3.0 * ref).backward()
    x2 = a.cuda().requires_grad_(True)
    loss, _, _ = l1_ssim_loss(x2, b.cuda(), 0.2)
    (3.0 * loss).backward()
    assert abs(loss.item() - ref.item()) < 2e-6
    gr, gg = x1.grad.cpu().numpy(), x2.grad.cpu().numpy()
    assert np.abs(gr - gg).max() <= 1e-5 * np.abs(gr).max()
