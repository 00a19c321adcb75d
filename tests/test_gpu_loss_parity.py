"""GPU: the fused L1+SSIM loss (csrc/ssim.hip: dgs_l1_ssim_forward / dgs_l1_ssim_backward) against the float64 oracle
of tests/loss_ref.py on the frames training gives it, and its exact properties through the C ABI.

Inputs (loss_ref.scene): an object on a flat white or black background, the render close to its target, half of the
background exactly equal to it (sign term 0); plus an identical pair, uniform noise and a render above 1. Shapes
(loss_ref.SHAPES): narrower than the 11-tap window in one or both directions, exactly one 32 x 32 tile, one pixel over
and under a tile, the 5-pixel halo on a tile edge, several tiles, 1026 tile blocks on a 1 x 10913 image (the final
reduction's strided loop wraps), C = 1 and C = 4. lambda 0.2 and 1.0.

Tolerances (loss_ref.bars), with E32 = |the reference's own loss in fp32 torch on the CPU - oracle| on the same input,
ulp = 2^-23, n = C H W:
  loss, L1, SSIM:        |gpu - oracle| <= max(4 E32, ulp)
  gradient, per region:  |gpu - oracle| <= max(4 max_region(E32), 4 ulp / n) for every element of the object and of
                         the background (where |g| is 10-100x smaller than on the object)
No fixed number is used: E32 of the SSIM mean is ~1e-5 on a white background and ~4e-7 on a black one (the reference's
own E[I^2] - mu^2 near 1; tests/test_loss_ref.py). tests/test_loss_ref.py shows on the CPU that the kernels' arithmetic
reaches these bars. Measured errors (MI355X): profiles/loss_parity.jsonl, written when DGS_PARITY_OUT names a file.

What these tests found (fixed in csrc/ssim.hip, csrc/metrics.hip and csrc/ssim_tile.h): the mean SSIM of an
`identical` pair on more than one tile came out 2-3 ulps below the reference's exact 1.0 (E32 = 0, so the bar is one
ulp). The compiler had vectorised the E[I^2] / E[G^2] tap sums in pairs and kept E[IG] scalar, contracted the two
differently and fused mu1^2 + mu2^2 on one side only, so pixels were 1 -+ 2^-24 and their fp32 tile sums lost more. The
forward tap sums are explicit fmaf now, ssim_pixel rounds every operation on its own and divides once: an identical pair
gives exactly 1.0, and every value is within half an ulp of loss_ref.emulate.
"""
import json
import os

import numpy as np
import pytest
import torch

import loss_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5  # a NaN: a guard read as a value shows up, and so does one overwritten by any number
GUARD = 1024
ABI_SHAPES = ((33, 31), (67, 97))


def shape_id(s):
    return "x".join(map(str, s))


def record(name, H, W, C, regime, lam, scale, got, d):
    """Compare with the bars, print the worst ratios, append them to DGS_PARITY_OUT; -> failures."""
    report, failures = ref.compare(got, d["f64"], d["f32"], d["mask"])
    emu = ref.emulate(d["img"], d["gt"], lam, dloss=scale)
    line = {"test": name, "H": H, "W": W, "C": C, "regime": regime, "lambda": lam, "upstream": scale,
            "device": torch.cuda.get_device_name(0), "oracle": {"loss": d["f64"][0], "l1": d["f64"][1], "ssim": d["f64"][2]},
            **report,
            "gpu_minus_emulation": {"loss": abs(got[0] - emu[0]), "l1": abs(got[1] - emu[1]), "ssim": abs(got[2] - emu[2]),
                                    "grad_max": (got[3].reshape(emu[3].shape) - emu[3]).abs().max().item()}}
    print(f"{H}x{W}x{C} {regime} lambda {lam}: {ref.summary(report)}")
    if os.environ.get("DGS_PARITY_OUT"):
        with open(os.environ["DGS_PARITY_OUT"], "a") as f:
            f.write(json.dumps(line) + "\n")
    return failures


def fused(img, gt, lam, scale=1.0):
    from deformgs.loss import l1_ssim_loss
    x = img.cuda().requires_grad_(True)
    loss, l1, s = l1_ssim_loss(x, gt.cuda(), lam)
    (loss if scale == 1.0 else scale * loss).backward()
    return loss.item(), l1.item(), s.item(), x.grad.cpu()


@pytest.mark.parametrize("lam", ref.LAMBDAS)
@pytest.mark.parametrize("regime", ref.REGIMES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_parity(shape, regime, lam):
    H, W, C = shape
    d = ref.case(H, W, C, regime, lam)
    failures = record("parity", H, W, C, regime, lam, 1.0, fused(d["img"], d["gt"], lam), d)
    assert not failures, failures


def test_parity_with_upstream_factor():
    H, W, C, regime, lam, scale = 67, 97, 3, "train_white", 0.2, 0.37
    d = ref.case(H, W, C, regime, lam, scale)
    failures = record("parity_upstream", H, W, C, regime, lam, scale, fused(d["img"], d["gt"], lam, scale), d)
    assert not failures, failures


# ---- the C ABI, called as dgs_train_step calls it ----
def filled(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def untouched(t):
    return bool((t == SENTINEL).all())


class Call:
    """out3, scratch (exactly dgs_l1_ssim_scratch_floats) and grad, each between two guards of GUARD sentinel floats."""

    def __init__(self, img, gt):
        from deformgs import _lib
        self.L, self.lib = _lib, _lib.load()
        self.img, self.gt = img.cuda().contiguous(), gt.cuda().contiguous()
        self.C, self.H, self.W = self.img.shape
        self.n_scratch = self.lib.dgs_l1_ssim_scratch_floats(self.C, self.H, self.W)
        self.raw = {"out3": filled(2 * GUARD + 3), "scratch": filled(2 * GUARD + self.n_scratch),
                    "grad": filled(2 * GUARD + self.img.numel())}

    def inner(self, k):
        return self.raw[k][GUARD:-GUARD]

    def f32(self, k):
        return self.inner(k).view(torch.float32)

    def guards_untouched(self):
        torch.cuda.synchronize()
        return all(untouched(t[:GUARD]) and untouched(t[-GUARD:]) for t in self.raw.values())

    def forward(self, lam, dims=None, **null):
        p = {k: None if k in null else self.L.ptr(v) for k, v in
             (("img", self.img), ("gt", self.gt), ("out3", self.inner("out3")), ("scratch", self.inner("scratch")))}
        C, H, W = dims or (self.C, self.H, self.W)
        return self.lib.dgs_l1_ssim_forward(C, H, W, p["img"], p["gt"], lam, p["out3"], p["scratch"], self.L.stream_ptr())

    def backward(self, lam, dloss=None, dims=None, **null):
        dl = None if dloss is None else torch.tensor([dloss], dtype=torch.float32, device="cuda")
        p = {k: None if k in null else self.L.ptr(v) for k, v in
             (("img", self.img), ("gt", self.gt), ("scratch", self.inner("scratch")), ("grad", self.inner("grad")))}
        C, H, W = dims or (self.C, self.H, self.W)
        rc = self.lib.dgs_l1_ssim_backward(C, H, W, p["img"], p["gt"], lam, p["scratch"], self.L.ptr(dl), p["grad"],
                                           self.L.stream_ptr())
        torch.cuda.synchronize()  # dl stays alive until the kernel has read it
        return rc


def train_white(H, W):
    d = ref.case(H, W, 3, "train_white", 0.2)
    return d["img"], d["gt"]


@pytest.mark.parametrize("hw", ABI_SHAPES, ids=shape_id)
def test_lambda_zero_is_the_l1_term_bit_for_bit(hw):
    img, gt = train_white(*hw)
    c = Call(img, gt)
    assert c.forward(0.0) == 0 and c.backward(0.0) == 0
    out3 = c.inner("out3").cpu()
    assert out3[0].item() == out3[1].item()                      # (int32 views: the bits)
    n32 = np.float32(3) * np.float32(hw[0]) * np.float32(hw[1])
    want = torch.sign(img - gt) * float(np.float32(1) / n32)
    assert want.dtype == torch.float32
    g = c.f32("grad").cpu().reshape(img.shape)
    assert torch.equal(g.view(torch.int32), want.view(torch.int32))
    assert (img == gt).any() and (g[img == gt] == 0).all()


@pytest.mark.parametrize("hw", ABI_SHAPES, ids=shape_id)
def test_lambda_one_is_one_minus_ssim(hw):
    c = Call(*train_white(*hw))
    assert c.forward(1.0) == 0
    torch.cuda.synchronize()
    out3 = c.f32("out3").cpu().numpy()
    assert out3[0].view(np.int32) == (np.float32(1) - out3[2]).view(np.int32)


@pytest.mark.parametrize("hw", ABI_SHAPES, ids=shape_id)
def test_upstream_gradient_none_one_half_zero(hw):
    c = Call(*train_white(*hw))
    assert c.forward(0.2) == 0
    grads = {}
    for key, dloss in (("none", None), ("one", 1.0), ("half", 0.5), ("zero", 0.0)):
        c.inner("grad").fill_(SENTINEL)
        assert c.backward(0.2, dloss) == 0
        grads[key] = c.f32("grad").clone()
    assert torch.isfinite(grads["none"]).all() and (grads["none"] != 0).any()
    assert torch.equal(grads["none"].view(torch.int32), grads["one"].view(torch.int32))   # the branch dgs_train_step takes
    assert torch.equal(grads["half"], 0.5 * grads["one"])
    assert (grads["zero"] == 0).all()


@pytest.mark.parametrize("hw", ABI_SHAPES, ids=shape_id)
def test_two_calls_are_bitwise_equal(hw):
    img, gt = train_white(*hw)
    a, b = Call(img, gt), Call(img, gt)
    for c in (a, b):
        assert c.forward(0.2) == 0 and c.backward(0.2) == 0
    for k in ("out3", "scratch", "grad"):
        assert torch.equal(a.inner(k), b.inner(k)), k


@pytest.mark.parametrize("hw", ((1, 1), (33, 31), (65, 33)), ids=shape_id)
def test_kernels_stay_inside_their_buffers(hw):
    img, gt = train_white(*hw)
    c = Call(img, gt)
    assert c.n_scratch == 3 * img.numel() + 2 * 3 * (-(-hw[0] // 32)) * (-(-hw[1] // 32))
    assert c.forward(0.2) == 0 and c.backward(0.2) == 0
    assert c.guards_untouched()
    assert torch.equal(c.img.cpu().view(torch.int32), img.view(torch.int32))
    assert torch.equal(c.gt.cpu().view(torch.int32), gt.view(torch.int32))
    assert torch.isfinite(c.f32("grad")).all() and torch.isfinite(c.f32("out3")).all()


def test_rejected_calls_return_the_args_error_and_write_nothing():
    c = Call(*train_white(33, 31))
    C, H, W = c.C, c.H, c.W
    for dims in ((0, H, W), (C, 0, W), (C, H, 0)):
        assert c.forward(0.2, dims=dims) == -1, dims
        assert c.backward(0.2, 1.0, dims=dims) == -1, dims
    for name in ("img", "gt", "out3", "scratch"):
        assert c.forward(0.2, **{name: True}) == -1, name
        assert b"dgs_l1_ssim_forward" in c.lib.dgs_last_error()
    for name in ("grad", "scratch", "img", "gt"):
        assert c.backward(0.2, 1.0, **{name: True}) == -1, name
        assert b"dgs_l1_ssim_backward" in c.lib.dgs_last_error()
    torch.cuda.synchronize()
    assert all(untouched(t) for t in c.raw.values()), "a rejected call launches nothing"
    assert c.forward(0.2) == 0 and c.backward(0.2) == 0 and c.guards_untouched()   # and the same buffers then work


# ---- the torch wrapper ----
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_wrapper_noncontiguous_batched_and_gt_grad():
    from deformgs.loss import l1_ssim_loss
    img, gt = train_white(33, 31)
    x = img.cuda().requires_grad_(True)
    base = l1_ssim_loss(x, gt.cuda(), 0.2)
    base[0].backward()
    # an HWC image viewed as CHW
    hwc = img.permute(1, 2, 0).contiguous().cuda()
    v = hwc.permute(2, 0, 1).detach().requires_grad_(True)
    assert not v.is_contiguous()
    out = l1_ssim_loss(v, gt.cuda(), 0.2)
    out[0].backward()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out, base))
    assert torch.equal(bits(v.grad), bits(x.grad))
    # (1, 3, H, W)
    b4 = img[None].cuda().requires_grad_(True)
    out4 = l1_ssim_loss(b4, gt[None].cuda(), 0.2)
    out4[0].backward()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out4, base))
    assert b4.grad.shape == (1, 3, 33, 31) and torch.equal(bits(b4.grad[0]), bits(x.grad))
    with pytest.raises(NotImplementedError):
        l1_ssim_loss(img.cuda(), gt.cuda().requires_grad_(True), 0.2)
