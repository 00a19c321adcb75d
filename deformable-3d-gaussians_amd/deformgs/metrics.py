"""python -m deformgs.metrics -m MODEL [MODEL ...] — the counterpart of metrics.py:39-98.

For every <MODEL>/test/ours_* directory: per-view and mean PSNR (loss.psnr) and SSIM between renders/ and gt/
(8-bit RGB PNGs read with deformgs/png.py, scaled to [0, 1] as torchvision's to_tensor does), written to
<MODEL>/results.json ({method: {"SSIM", "PSNR", "LPIPS"}}) and <MODEL>/per_view.json ({method: {metric:
{file name: value}}}) in the reference's layout. SSIM is the fused HIP loss kernel's mean SSIM
(dgs_l1_ssim_forward: the reference's 11x11 sigma-1.5 window). LPIPS is recorded as null unless the two weight
files are given: they are the user's to supply, and nothing here ships or fetches them.

--lpips_vgg VGG16.pth --lpips_lin VGG_LIN.pth: fills "LPIPS" in both files with LPIPS-VGG (deformgs.lpips: the
lpips package's net='vgg', version 0.1, on the [0, 1] images as the reference passes them) from torchvision's
VGG16 state dict and the LPIPS linear-layer file: one batched call per group of equally sized images (at least
16 pixels a side), the mean taken over the per-view values. --lpips_normalize maps the images through 2v - 1
first. One of the two files without the other is an error.

--ms_ssim: adds "MS-SSIM" (pytorch_msssim.ms_ssim's definition, data_range 1) and "D-SSIM" = (1 - MS-SSIM) / 2, the
two further columns of the upstream Deformable-3D-Gaussians metrics.py, to both files: one batched
deformgs.image_metrics call per group of equally sized images (they must be larger than 160 pixels a side).
Without the flag both files are what they always were.

--synthetic N: when <MODEL>/test holds no ours_* directory yet, the test set of the synthetic scene is
rendered first (deformgs.render_cli --mode render), so the script runs with no dataset.
"""
import argparse
import json
import os

import torch

from .loss import l1_ssim_forward, psnr
from .png import read_png


def fused_ssim(img, gt):
    """Mean SSIM of two (1, 3, H, W) device images from the fused L1 + SSIM forward kernel."""
    return l1_ssim_forward(img[0].float().contiguous(), gt[0].float().contiguous(), 0.2)[0][2]


def read_images(renders_dir, gt_dir, device):
    """-> (renders, gts, names): (1, 3, H, W) float tensors in [0, 1] (metrics.py:25-36)."""
    renders, gts, names = [], [], []
    for fname in sorted(os.listdir(renders_dir)):
        if not fname.endswith(".png"):
            continue
        pair = []
        for d in (renders_dir, gt_dir):
            a = read_png(os.path.join(d, fname))
            if a.ndim != 3:
                raise ValueError(f"{os.path.join(d, fname)}: expected an 8-bit RGB PNG")
            pair.append((torch.from_numpy(a).to(device).permute(2, 0, 1).contiguous().float() / 255.0).unsqueeze(0))
        renders.append(pair[0])
        gts.append(pair[1])
        names.append(fname)
    return renders, gts, names


def by_size(renders, gts, score):
    """score(renders, gts) -> (n,) device tensor, called once per group of equally sized (1, 3, H, W) pairs;
    -> the values in the order of `renders`, read back after the last call."""
    groups = {}
    for i, r in enumerate(renders):
        groups.setdefault(tuple(r.shape), []).append(i)
    parts = [(idx, score([renders[i] for i in idx], [gts[i] for i in idx])) for idx in groups.values()]
    values = [0.0] * len(renders)
    for idx, v in parts:
        for i, x in zip(idx, v.tolist()):
            values[i] = x
    return values


def batched_ms_ssim(renders, gts):
    """MS-SSIM of every (1, 3, H, W) pair: one image_metrics call per image size, one host read."""
    from .image_metrics import image_metrics
    return by_size(renders, gts, lambda r, g: image_metrics(r, g, ("ms_ssim",))["ms_ssim"])


def batched_lpips(renders, gts, weights, normalize=False):
    """LPIPS-VGG of every (1, 3, H, W) pair: one lpips call per image size, one host read."""
    from .lpips import lpips
    return by_size(renders, gts, lambda r, g: lpips(r, g, weights, normalize=normalize))


def evaluate(model_paths, ssim_fn=None, device="cuda", ms_ssim=False, lpips_weights=None, lpips_normalize=False):
    """Writes results.json / per_view.json under every model path; -> {model path: results dict}.
    lpips_weights: deformgs.lpips weights on `device`, or None to record LPIPS as null."""
    ssim_fn = ssim_fn or fused_ssim
    full = {}
    for scene_dir in model_paths:
        print("Scene:", scene_dir)
        full[scene_dir], per_view = {}, {}
        test_dir = os.path.join(scene_dir, "test")
        for method in sorted(os.listdir(test_dir)):
            if not method.startswith("ours"):
                continue
            print("Method:", method)
            renders, gts, names = read_images(os.path.join(test_dir, method, "renders"),
                                              os.path.join(test_dir, method, "gt"), device)
            ssims = [float(ssim_fn(r, g)) for r, g in zip(renders, gts)]
            psnrs = [float(psnr(r, g)) for r, g in zip(renders, gts)]
            m_ssim, m_psnr = torch.tensor(ssims).mean().item(), torch.tensor(psnrs).mean().item()
            print("  SSIM : {:>12.7f}".format(m_ssim))
            print("  PSNR : {:>12.7f}".format(m_psnr))
            m_lpips, lpipss = None, [None] * len(names)
            if lpips_weights is None:
                print("  LPIPS: not computed\n")
            else:
                lp = torch.tensor(batched_lpips(renders, gts, lpips_weights, lpips_normalize))
                m_lpips, lpipss = lp.mean().item(), lp.tolist()
                print("  LPIPS: {:>12.7f}\n".format(m_lpips))
            full[scene_dir][method] = {"SSIM": m_ssim, "PSNR": m_psnr, "LPIPS": m_lpips}
            per_view[method] = {"SSIM": dict(zip(names, torch.tensor(ssims).tolist())),
                                "PSNR": dict(zip(names, torch.tensor(psnrs).tolist())),
                                "LPIPS": dict(zip(names, lpipss))}
            if ms_ssim:
                ms = torch.tensor(batched_ms_ssim(renders, gts))
                m_ms = ms.mean().item()
                print("  MS-SSIM: {:>10.7f}".format(m_ms))
                print("  D-SSIM : {:>10.7f}\n".format((1.0 - m_ms) / 2.0))
                full[scene_dir][method].update({"MS-SSIM": m_ms, "D-SSIM": (1.0 - m_ms) / 2.0})
                per_view[method].update({"MS-SSIM": dict(zip(names, ms.tolist())),
                                         "D-SSIM": dict(zip(names, ((1.0 - ms.double()) / 2.0).tolist()))})
        with open(os.path.join(scene_dir, "results.json"), "w") as fp:
            json.dump(full[scene_dir], fp, indent=True)
        with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
            json.dump(per_view, fp, indent=True)
    return full


def build_parser():
    ap = argparse.ArgumentParser(description="PSNR / SSIM of rendered test sets (metrics.py counterpart)")
    ap.add_argument("--model_paths", "-m", required=True, nargs="+")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    ap.add_argument("--res", type=int, nargs=2, default=[800, 800], metavar=("W", "H"))
    ap.add_argument("--ms_ssim", action="store_true",
                    help="also write MS-SSIM and D-SSIM = (1 - MS-SSIM) / 2 (images larger than 160 pixels a side)")
    ap.add_argument("--png", choices=["zlib", "gpu"], default="zlib", help="--synthetic: the PNG writer of the render step")
    ap.add_argument("--lpips_vgg", metavar="VGG16.pth", help="torchvision's VGG16 state dict; with --lpips_lin: write LPIPS-VGG")
    ap.add_argument("--lpips_lin", metavar="VGG_LIN.pth", help="the LPIPS linear-layer weights that go with --lpips_vgg")
    ap.add_argument("--lpips_normalize", action="store_true", help="map the images through 2v - 1 before LPIPS")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if bool(args.lpips_vgg) != bool(args.lpips_lin):
        ap.error("--lpips_vgg and --lpips_lin go together: LPIPS-VGG needs both weight files")
    if args.lpips_normalize and not args.lpips_vgg:
        ap.error("--lpips_normalize needs --lpips_vgg and --lpips_lin")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.synthetic:
        from . import render_cli
        for m in args.model_paths:
            t = os.path.join(m, "test")
            if not (os.path.isdir(t) and any(d.startswith("ours") for d in os.listdir(t))):
                render_cli.main(["-m", m, "--synthetic", str(args.synthetic), "--res", str(args.res[0]), str(args.res[1]),
                                 "--mode", "render", "--skip_train", "--png", args.png])
    weights = None
    if args.lpips_vgg:
        from .lpips import load_weights
        weights = load_weights(args.lpips_vgg, args.lpips_lin, "cuda")
    return evaluate(args.model_paths, ms_ssim=args.ms_ssim, lpips_weights=weights, lpips_normalize=args.lpips_normalize)


if __name__ == "__main__":
    main()
