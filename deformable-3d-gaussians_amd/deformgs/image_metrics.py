"""image_metrics(): N frame pairs in, N scores out, through dgs_image_metrics (csrc/metrics.hip).

PSNR (utils/image_utils.py:19-21) and SSIM (utils/loss_utils.py:41-73) as the reference defines them, and
MS-SSIM as pytorch_msssim.ms_ssim(X, Y, data_range=1) defines it (what the upstream Deformable-3D-Gaussians
metrics.py prints, with D-SSIM = (1 - MS-SSIM) / 2): five levels of an unpadded 11x11 sigma-1.5 filter with
avg_pool2d(2, 2, padding = side mod 2) between them, prod relu(cs_l)^w_l * relu(ssim_4)^w_4 per channel.
One call is a fixed number of launches for any number of frames and waits for nothing: the results are
device tensors and the caller decides when to read them.
"""
import torch

METRIC_BITS = {"psnr": 1, "ssim": 2, "ms_ssim": 4}  # DGS_METRIC_* (include/dgs.h)
LEVELS = 5
MS_SSIM_MIN_SIDE = 160  # (11 - 1) * 2^4: the fifth level must still hold one 11x11 window


def _batch(x, what):
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError(f"image_metrics: empty list of {what}")
        if any(not torch.is_tensor(t) for t in x):
            raise ValueError(f"image_metrics: {what} must be tensors")
        if any(t.shape != x[0].shape for t in x):
            raise ValueError(f"image_metrics: {what} of different sizes in one call: "
                             f"{sorted({tuple(t.shape) for t in x})}")
        x = torch.stack(list(x)) if x[0].dim() == 3 else torch.cat(list(x))
    if not torch.is_tensor(x):
        raise ValueError(f"image_metrics: {what} must be a tensor or a list of tensors")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError(f"image_metrics: {what} must be (F, C, H, W) or (C, H, W), got {tuple(x.shape)}")
    return x


def image_metrics(renders, gts, metrics=("psnr", "ssim", "ms_ssim")):
    """renders, gts: (F, C, H, W) or (C, H, W) device float tensors in [0, 1], or lists of such of one size.
    -> {name: (F,) device tensor for every name in `metrics`, "levels": (F, 2, 5, C)}: levels[:, 0] are
    the per-level, per-channel cs means of the MS-SSIM pyramid, levels[:, 1] the ssim means (NaN when
    ms_ssim is not asked for). PSNR of identical images is +inf. Raises ValueError on CPU tensors (there is
    no fallback), mismatched shapes, unknown names and MS-SSIM on a side of 160 pixels or less."""
    if isinstance(metrics, str):
        metrics = (metrics,)
    names = tuple(metrics)
    unknown = [n for n in names if n not in METRIC_BITS]
    if unknown or not names:
        raise ValueError(f"image_metrics: unknown metrics {unknown}; choose from {sorted(METRIC_BITS)}")
    what = 0
    for n in names:
        what |= METRIC_BITS[n]
    a, b = _batch(renders, "renders"), _batch(gts, "gts")
    if a.shape != b.shape:
        raise ValueError(f"image_metrics: renders {tuple(a.shape)} and gts {tuple(b.shape)} differ in shape")
    from . import _lib
    _lib.require_cuda(a, b)
    if a.device != b.device:
        raise ValueError(f"image_metrics: renders on {a.device}, gts on {b.device}")
    F, C, H, W = a.shape
    if "ms_ssim" in names and min(H, W) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"image_metrics: MS-SSIM needs min(H, W) > {MS_SSIM_MIN_SIDE} (five levels of an unpadded "
                         f"11-tap filter: (11 - 1) * 2^4 = 160); got {H} x {W}")
    lib = _lib.load()
    a, b = a.float().contiguous(), b.float().contiguous()
    out = torch.empty((F, 3 + 2 * LEVELS * C), dtype=torch.float32, device=a.device)
    scratch = torch.empty(lib.dgs_image_metrics_scratch_bytes(F, C, H, W, what), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.dgs_image_metrics(F, C, H, W, _lib.ptr(a), _lib.ptr(b), what, _lib.ptr(out), _lib.ptr(scratch),
                                         _lib.stream_ptr(a.device)), "image_metrics")
    res = {n: out[:, ("psnr", "ssim", "ms_ssim").index(n)] for n in names}
    res["levels"] = out[:, 3:].view(F, 2, LEVELS, C)
    return res
