"""References for the fused L1+SSIM loss (csrc/ssim.hip: dgs_l1_ssim_forward / dgs_l1_ssim_backward) on the frames
training gives it, and the tolerances that follow from them. No GPU is used here.

  oracle(img, gt, lam, dtype)   deformgs.loss.l1_loss / ssim on the CPU with autograd, unchanged. float64 is the oracle
                                (create_window builds the reference's fp32-rounded 2-D window and casts it: the window
                                the kernel's taps were tuned against); float32 is the reference's own arithmetic. Its
                                distance from the oracle is called E32 below.
  emulate(img, gt, lam)         a numpy fp32 restatement of the kernels' arithmetic from the header comments of ssim.hip
                                and ssim_tile.h: taps of dgs_l1_ssim_window (a host call), zero-padded row pass then
                                column pass, ssim_pixel, the coefficient maps A / B / C and the backward
                                wl1 sign(I - G) - wss (w*A + 2 I w*B + G w*C); value sums in float64 over float32(n).
                                The tap sums are accumulated as fused multiply-adds (acc = fmaf(w, v, acc), as the
                                forward kernel states them); everything else is rounded operation by operation. It is a restatement, not a bit-exact model: it shows that the bars below are
                                reachable by that arithmetic and it localises a failure (kernel != emulation: the kernel).
  scene(H, W, seed, regime)     (img, gt, object_mask), float32 (C, H, W): an object (ms_ssim_ref.pattern_pair with
                                noise 0.03 inside a centred ellipse, semi-axes 0.3 H and 0.3 W) on a flat background. On
                                the left half of the background img == gt exactly (sign term 0), on the right half img
                                is gt moved towards the inside of [0, 1] by up to 3e-4.
  bars / compare                with ulp = 2^-23 and n = C H W:
                                  loss, L1, SSIM:  |got - oracle| <= max(4 E32, ulp)
                                  gradient, per region (the object mask; its complement where it is not empty), element by
                                  element:         |got - oracle| <= max(4 max_region(E32), 4 ulp / n)
                                4 is what tests/test_gpu_image_metrics.py uses for "the same arithmetic in another
                                summation order"; the floor is four ulps of the per-pixel L1 gradient 1 / n, needed
                                because E32 can be exactly 0 (a 1 x 1 identical pair). The bars come from the oracle and
                                E32 only, never from the output under test.

Why no fixed tolerance: on a white background the variances E[I^2] - mu^2 are differences of numbers near 1 that cancel
against C2 = 9e-4, so the reference's own fp32 SSIM sits ~1e-5 from float64, tens of times further than on a black
background (tests/test_loss_ref.py asserts the ratio), and no constant fits both.
"""
import ctypes
import functools

import numpy as np
import torch

import ms_ssim_ref

ULP = float(np.finfo(np.float32).eps)
REGIMES = ("train_white", "train_black", "near", "identical", "uniform", "bright")
_FLAT = {"train_white": (1.0, 0.02), "train_black": (0.0, 0.02), "near": (1.0, 0.002), "identical": (1.0, 0.02)}
# (H, W, C): narrower than the 11-tap window; one 32 x 32 tile; one pixel over / under a tile; the 5-pixel halo on a
# tile edge; several tiles; 342 x 3 = 1026 tile blocks (the final reduction's strided loop wraps); C = 1 and C = 4
SHAPES = ((1, 1, 3), (1, 40, 3), (40, 1, 3), (10, 11, 3), (32, 32, 3), (33, 31, 3), (37, 64, 3), (65, 33, 3),
          (67, 97, 3), (1, 10913, 3), (33, 31, 1), (33, 31, 4))
LAMBDAS = (0.2, 1.0)


def oracle(img, gt, lam, dtype=torch.float64, scale=1.0):
    """-> (loss, l1, ssim, grad): the reference's loss in `dtype` on the CPU; grad = d(scale * loss)/d img as float64."""
    from deformgs.loss import l1_loss, ssim
    x = img.detach().cpu().to(dtype).requires_grad_(True)
    y = gt.detach().cpu().to(dtype)
    l1 = l1_loss(x, y)
    s = ssim(x, y)
    loss = (1.0 - lam) * l1 + lam * (1.0 - s)
    (scale * loss).backward()
    return loss.item(), l1.item(), s.item(), x.grad.double()


@functools.lru_cache(maxsize=None)
def taps():
    """The kernel's 11 separable window taps (float32)."""
    from deformgs import _lib
    out = (ctypes.c_float * 11)()
    _lib.load().dgs_l1_ssim_window(out)
    return np.array(out[:], np.float32)


def _fma(a, b, c):
    # a * b is exact in float64 (24 + 24 bits); the sum is rounded to 53 bits, then to 24
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _filter(m, w):
    """(C, H, W) float32 -> the zero-padded 11-tap row pass, then the column pass, taps in ascending order."""
    C, H, W = m.shape
    p = np.zeros((C, H + 10, W + 10), np.float32)
    p[:, 5:5 + H, 5:5 + W] = m
    rows = np.zeros((C, H + 10, W), np.float32)
    for k in range(11):
        rows = _fma(np.broadcast_to(w[k], rows.shape), p[:, :, k:k + W], rows)
    out = np.zeros((C, H, W), np.float32)
    for k in range(11):
        out = _fma(np.broadcast_to(w[k], out.shape), rows[:, k:k + H, :], out)
    return out


def emulate(img, gt, lam, dloss=1.0, contract=False):
    """-> (loss, l1, ssim, grad float32 tensor): the kernels' fp32 arithmetic restated in numpy. contract=True also
    fuses the backward's sum of products, which the device compiler is free to do there (floating-point contraction is
    on outside ssim_pixel); the CPU test asks both roundings to hold."""
    f = np.float32
    I = np.ascontiguousarray(img.detach().cpu().numpy(), dtype=f)
    G = np.ascontiguousarray(gt.detach().cpu().numpy(), dtype=f)
    C, H, W = I.shape
    w = taps()
    with np.errstate(all="ignore"):
        mu1, mu2 = _filter(I, w), _filter(G, w)
        e11, e22, e12 = _filter(I * I, w), _filter(G * G, w), _filter(I * G, w)
        c1, c2, two = f(0.01) * f(0.01), f(0.03) * f(0.03), f(2)
        mu1s, mu2s, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        # ssim_pixel: contraction off, every operation rounded on its own, sv one division of the two products
        s11, s22, s12 = e11 - mu1s, e22 - mu2s, e12 - mu12
        n1, n2 = two * mu12 + c1, two * s12 + c2
        d1, d2 = mu1s + mu2s + c1, s11 + s22 + c2
        inv = f(1) / (d1 * d2)
        sv = (n1 * n2) / (d1 * d2)
        A = two * mu2 * n2 * inv - two * mu1 * sv / d1 + two * mu1 * sv / d2 - mu2 * two * n1 * inv
        B = -sv / d2
        Cc = two * n1 * inv
        n = f(C) * f(H) * f(W)
        l1 = f(np.abs(I - G).astype(np.float64).sum() / np.float64(n))
        ss = f(sv.astype(np.float64).sum() / np.float64(n))
        lam32 = f(lam)
        loss = (f(1) - lam32) * l1 + lam32 * (f(1) - ss)
        wl1, wss = (f(1) - lam32) / n, lam32 / n
        fa, fb, fc = _filter(A, w), _filter(B, w), _filter(Cc, w)
        d = I - G
        sg = np.where(d > 0, f(1), np.where(d < 0, f(-1), f(0))).astype(f)
        if contract:
            inner = _fma(G, fc, _fma(two * I, fb, fa))
            grad = f(dloss) * _fma(np.broadcast_to(-wss, inner.shape), inner, wl1 * sg)
        else:
            grad = f(dloss) * (wl1 * sg - wss * (fa + two * I * fb + G * fc))
    return float(loss), float(l1), float(ss), torch.from_numpy(grad.astype(f))


def scene(H, W, seed, regime, channels=3, bg=None):
    """-> (img, gt, object_mask): float32 (C, H, W) images and a bool (C, H, W) mask of the object region. `uniform`
    and `bright` are one region (the mask is all True). bg overrides the background value of the flat regimes."""
    gen = torch.Generator().manual_seed(seed)
    if regime in ("uniform", "bright"):
        a = torch.rand((channels, H, W), generator=gen)
        b = torch.rand((channels, H, W), generator=gen)
        return (1.5 * a if regime == "bright" else a), b, torch.ones((channels, H, W), dtype=torch.bool)
    value, diff = _FLAT[regime]
    if bg is not None:
        value = float(bg)
    pimg, pgt = ms_ssim_ref.pattern_pair(H, W, seed, channels=channels, noise=0.03, diff=diff)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    inside = ((yy - (H - 1) / 2) / (0.3 * H)) ** 2 + ((xx - (W - 1) / 2) / (0.3 * W)) ** 2 <= 1.0
    mask = inside.expand(channels, H, W).contiguous()
    gt = torch.where(mask, pgt, torch.full_like(pgt, value))
    if regime == "identical":
        return gt.clone(), gt, mask
    # towards the inside of [0, 1]: down from a background above 0.5, up from one below
    step = 3e-4 * torch.rand((channels, H, W), generator=gen) * (-1.0 if value > 0.5 else 1.0)
    right = (xx >= W / 2).expand(channels, H, W)
    flat = torch.where(right, gt + step, gt)
    return torch.where(mask, pimg, flat).contiguous(), gt, mask


# inputs replaced under the rule of tests/test_loss_ref.py (another seed of the same kind; the bar is never widened):
# on the default seed (1064) the reference's fp32 SSIM happened to land 1.2e-7 from float64, where the emulated
# arithmetic gives 8.3e-7 and the same scene with the eleven neighbouring seeds has E32 between 7e-7 and 7e-6
_RESEEDED = {(33, 31, 1, "near"): 1065}


def seed_of(H, W, C, regime=None):
    return _RESEEDED.get((H, W, C, regime), 1000 * C + H + W)


@functools.lru_cache(maxsize=None)
def case(H, W, C, regime, lam, scale=1.0):
    """Inputs, the float64 oracle and the reference's own fp32 result of one combination, computed once and shared
    (read-only) by the CPU and the GPU tests."""
    img, gt, mask = scene(H, W, seed_of(H, W, C, regime), regime, channels=C)
    return {"img": img, "gt": gt, "mask": mask, "f64": oracle(img, gt, lam, torch.float64, scale),
            "f32": oracle(img, gt, lam, torch.float32, scale)}


def regions(mask):
    out = [("object", mask)]
    if not bool(mask.all()):
        out.append(("background", ~mask))
    return out


def bars(f64, f32, mask):
    """-> {"loss", "l1", "ssim": (bar, E32)} and {"grad": [(region name, region mask, bar, max E32)]}."""
    out = {}
    for i, q in enumerate(("loss", "l1", "ssim")):
        e32 = abs(f32[i] - f64[i])
        out[q] = (max(4 * e32, ULP), e32)
    e32g = (f32[3] - f64[3]).abs()
    n = mask.numel()
    out["grad"] = [(name, m, max(4 * e32g[m].max().item(), 4 * ULP / n), e32g[m].max().item())
                   for name, m in regions(mask)]
    return out


def compare(got, f64, f32, mask):
    """got = (loss, l1, ssim, grad) -> (report, failures): per quantity the error against the oracle, its bar, E32
    and err / bar, err / E32 (None where E32 is 0); failures names what is over its bar (and, for a gradient region,
    where its worst element is)."""
    b = bars(f64, f32, mask)
    report, failures = {}, []

    def entry(err, bar, e32):
        return {"err": err, "bar": bar, "e32": e32, "err_over_bar": err / bar, "err_over_e32": err / e32 if e32 > 0 else None}
    for i, q in enumerate(("loss", "l1", "ssim")):
        bar, e32 = b[q]
        err = abs(float(got[i]) - f64[i])
        report[q] = entry(err, bar, e32)
        if not err <= bar:
            failures.append(f"{q}: err {err:.3e} > bar {bar:.3e} (E32 {e32:.3e})")
    g = got[3].detach().cpu().double().reshape(f64[3].shape)
    diff = (g - f64[3]).abs()
    for name, m, bar, e32 in b["grad"]:
        d = torch.where(m, diff, torch.zeros_like(diff))
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        err = d.max().item()
        report[f"grad_{name}"] = entry(err, bar, e32)
        if not err <= bar:
            c, y, x = np.unravel_index(int(d.argmax()), tuple(d.shape))
            failures.append(f"grad[{name}]: err {err:.3e} > bar {bar:.3e} (E32 {e32:.3e}) at c={c} y={y} x={x}, "
                            f"tile ({y // 32}, {x // 32}), {int((~(d <= bar) & m).sum())} elements over")
    return report, failures


def summary(report):
    return "; ".join(f"{q} err/bar {r['err_over_bar']:.3f}" +
                     (f" err/E32 {r['err_over_e32']:.3f}" if r["err_over_e32"] is not None else " (E32 0)")
                     for q, r in report.items())
