"""Torch (CPU) restatement of the three image metrics of deformgs/image_metrics.py, float64 by default.

  psnr     utils/image_utils.py:19-21 per frame: mse = mean (img - gt)^2 over C*H*W, 20 log10(1 / sqrt(mse))
  ssim     utils/loss_utils.py:41-73: 11x11 sigma-1.5 window, zero padding 5, C1 = 0.01^2, C2 = 0.03^2,
           mean over C*H*W
  ms_ssim  pytorch_msssim.ms_ssim(X, Y, data_range=1), per frame: the window g[k] = exp(-(k-5)^2 / (2 1.5^2)) over
           its sum, filtered separably (rows of H first) with no padding; five levels with
           avg_pool2d(kernel 2, stride 2, padding (h mod 2, w mod 2)) between them (padded zeros counted);
           prod_{l<4} relu(cs_l)^w_l * relu(ssim_4)^w_4 per channel, mean over channels
Every function takes (F, C, H, W) tensors and a dtype: float64 is the oracle, float32 is the same arithmetic at
the precision of the kernels, whose distance from the oracle sets the tolerance of the GPU tests.
"""
import math

import torch
import torch.nn.functional as Fn

C1, C2 = 0.01 ** 2, 0.03 ** 2
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LEVELS = 5
MIN_SIDE = (11 - 1) * 2 ** 4  # 160: min(H, W) must be larger


def window(dtype=torch.float64):
    k = torch.arange(11, dtype=dtype)
    g = torch.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def psnr(img, gt, dtype=torch.float64):
    """-> (psnr, mse), (F,) each; mse == 0 gives +inf."""
    x, y = img.to(dtype), gt.to(dtype)
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(1)
    return 20 * torch.log10(1.0 / torch.sqrt(mse)), mse


def ssim(img, gt, dtype=torch.float64):
    """-> (F,) mean SSIM, zero-padded 11x11 window."""
    x, y = img.to(dtype), gt.to(dtype)
    C = x.shape[1]
    g = window(dtype)
    w = torch.outer(g, g).expand(C, 1, 11, 11).contiguous()

    def f(t):
        return Fn.conv2d(t, w, padding=5, groups=C)
    mu1, mu2 = f(x), f(y)
    s11, s22, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return m.reshape(m.shape[0], -1).mean(1)


def pooled_sizes(h, w):
    """The five (h, w) of the pyramid: a side s becomes floor((s + 2 (s mod 2) - 2) / 2) + 1."""
    out = [(h, w)]
    for _ in range(LEVELS - 1):
        h, w = ((s + 2 * (s % 2) - 2) // 2 + 1 for s in (h, w))
        out.append((h, w))
    return out


def _valid_filter(t, g):
    C = t.shape[1]
    t = Fn.conv2d(t, g.view(1, 1, 11, 1).expand(C, 1, 11, 1), groups=C)
    return Fn.conv2d(t, g.view(1, 1, 1, 11).expand(C, 1, 1, 11), groups=C)


def ms_ssim(img, gt, dtype=torch.float64):
    """-> (ms_ssim (F,), levels (F, 2, 5, C)): levels[:, 0] the cs means, levels[:, 1] the ssim means."""
    x, y = img.to(dtype), gt.to(dtype)
    if min(x.shape[-2:]) <= MIN_SIDE:
        raise ValueError(f"MS-SSIM needs min(H, W) > {MIN_SIDE}, got {tuple(x.shape[-2:])}")
    g = window(dtype)
    cs_l, ss_l = [], []
    for level in range(LEVELS):
        mu1, mu2 = _valid_filter(x, g), _valid_filter(y, g)
        s11 = _valid_filter(x * x, g) - mu1 * mu1
        s22 = _valid_filter(y * y, g) - mu2 * mu2
        s12 = _valid_filter(x * y, g) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
        ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
        cs_l.append(cs_map.flatten(2).mean(-1))
        ss_l.append(ssim_map.flatten(2).mean(-1))
        if level < LEVELS - 1:
            pad = [s % 2 for s in x.shape[-2:]]
            x = Fn.avg_pool2d(x, kernel_size=2, stride=2, padding=pad)
            y = Fn.avg_pool2d(y, kernel_size=2, stride=2, padding=pad)
    cs, ss = torch.stack(cs_l, 1), torch.stack(ss_l, 1)  # (F, 5, C)
    terms = torch.cat([torch.relu(cs[:, :-1]), torch.relu(ss[:, -1:])], 1)
    ms = torch.prod(terms ** torch.tensor(WEIGHTS, dtype=dtype).view(1, -1, 1), 1).mean(1)
    return ms, torch.stack([cs, ss], 1)


def pattern_pair(h, w, seed, channels=3, noise=0.08, diff=0.02):
    """A (C, h, w) float32 pair in [0, 1]: gt = smooth seeded pattern + seeded noise, img = gt + smaller noise
    (every level's cs stays positive)."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    planes = []
    for _ in range(channels):
        fx, fy, ph = (torch.rand(3, generator=gen, dtype=torch.float64) * torch.tensor([0.09, 0.07, 2 * math.pi])).tolist()
        planes.append(0.5 + 0.25 * torch.sin(fx * xx + ph) * torch.cos(fy * yy - ph) + 0.1 * torch.sin(0.011 * (xx + 2 * yy)))
    smooth = torch.stack(planes)
    gt = (smooth + noise * torch.randn(smooth.shape, generator=gen, dtype=torch.float64)).clamp(0, 1)
    img = (gt + diff * torch.randn(smooth.shape, generator=gen, dtype=torch.float64)).clamp(0, 1)
    return img.float(), gt.float()
