"""LPIPS-VGG (lpips.LPIPS(net='vgg'), version 0.1) restated in plain torch on the CPU, float64 by default.

  1. normalize: v -> 2v - 1 (off by default: the reference's metrics.py passes [0, 1] images as they are)
  2. per channel (v - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
  3. VGG16 features: 13 convolutions 3x3 / stride 1 / zero padding 1 with bias and ReLU, a 2x2 / stride 2 max
     pool (floor) after the 2nd, 4th, 7th and 10th; taps = the ReLU outputs before each pool and at the end
  4. per tap: f / (sqrt(sum_c f^2) + 1e-10) for both images, squared difference, lin_k weights over channels,
     mean over pixels = layer term k
  5. LPIPS = the sum of the five layer terms
Also the seeded random weights and image pairs the tests share.
"""
import math

import torch
import torch.nn.functional as tnf

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
            (512, 512), (512, 512), (512, 512), (512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)  # index of the convolution whose ReLU output is tap k; a pool follows all but the last
TAP_CHANNELS = (64, 128, 256, 512, 512)
VGG_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # torchvision's features.N of the 13 convolutions


def random_weights(seed=0, negative_lin=False):
    """-> (13 conv weights, 13 biases, 5 lin (1, C, 1, 1)), float32. Conv N(0, 2 / (9 C_in)), bias N(0, 0.1^2),
    lin uniform in [0, 2 / C) (negative_lin: in [-1 / C, 1 / C)): taps stay O(1), about half of each is zero."""
    gen = torch.Generator().manual_seed(seed)
    ws, bs, lins = [], [], []
    for cin, cout in CHANNELS:
        ws.append(torch.randn((cout, cin, 3, 3), generator=gen) * math.sqrt(2.0 / (9 * cin)))
        bs.append(torch.randn((cout,), generator=gen) * 0.1)
    for c in TAP_CHANNELS:
        u = torch.rand((1, c, 1, 1), generator=gen)
        lins.append(((u - 0.5) if negative_lin else u) * (2.0 / c))
    return ws, bs, lins


def state_dicts(ws, bs, lins, vgg_prefix="features.", lin_style="lpips"):
    """The two files' state dicts in either of their key layouts."""
    vgg = {}
    for n, w, b in zip(VGG_KEYS, ws, bs):
        vgg[f"{vgg_prefix}{n}.weight"] = w
        vgg[f"{vgg_prefix}{n}.bias"] = b
    lin = {(f"lin{k}.model.1.weight" if lin_style == "lpips" else f"{k}.1.weight"): v for k, v in enumerate(lins)}
    return vgg, lin


def pairs(H, W, seed, frames=3, noise=0.08, diff=0.05):
    """-> img, gt (frames, 3, H, W) float32 in [0, 1]: gt = seeded smooth pattern + noise, img = gt + noise
    clamped; the last frame has img == gt."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    imgs, gts = [], []
    for f in range(frames):
        planes = []
        for _ in range(3):
            fx, fy, ph = (torch.rand(3, generator=gen, dtype=torch.float64) * torch.tensor([0.5, 0.4, 2 * math.pi])).tolist()
            planes.append(0.5 + 0.3 * torch.sin(fx * xx + ph) * torch.cos(fy * yy - ph))
        gt = (torch.stack(planes) + noise * torch.randn((3, H, W), generator=gen, dtype=torch.float64)).clamp(0, 1)
        img = (gt + diff * torch.randn((3, H, W), generator=gen, dtype=torch.float64)).clamp(0, 1)
        gts.append(gt)
        imgs.append(gt if f == frames - 1 else img)
    return torch.stack(imgs).float(), torch.stack(gts).float()


def taps(x, ws, bs, normalize=False, dtype=torch.float64):
    """x: (F, 3, H, W) -> the five taps, (F, C, Hk, Wk) each, computed in `dtype`."""
    v = x.to(dtype)
    if normalize:
        v = 2 * v - 1
    v = (v - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    out = []
    for i, (w, b) in enumerate(zip(ws, bs)):
        v = torch.relu(tnf.conv2d(v, w.to(dtype), b.to(dtype), stride=1, padding=1))
        if i in TAP_AFTER:
            out.append(v)
            if i != TAP_AFTER[-1]:
                v = tnf.max_pool2d(v, kernel_size=2, stride=2)
    return out


def layer_terms(tx, ty, lins):
    """taps of both images -> (F, 5) layer terms in the taps' dtype."""
    terms = []
    for fx, fy, lin in zip(tx, ty, lins):
        nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = (nx - ny).pow(2) * lin.to(fx.dtype).view(1, -1, 1, 1)
        terms.append(d.sum(1).mean((1, 2)))
    return torch.stack(terms, 1)


def lpips(x, y, weights, normalize=False, dtype=torch.float64):
    """x, y: (F, 3, H, W); weights = (ws, bs, lins) -> (lpips (F,), layer terms (F, 5)) in `dtype`."""
    ws, bs, lins = weights
    if min(x.shape[-2:]) < 16:
        raise ValueError("LPIPS-VGG needs min(H, W) >= 16")
    terms = layer_terms(taps(x, ws, bs, normalize, dtype), taps(y, ws, bs, normalize, dtype), lins)
    return terms.sum(1), terms
