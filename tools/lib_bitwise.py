#!/usr/bin/env python3
"""Bitwise comparison of two builds of libdgs_hip.so on the fused MLP, on the SSIM kernels or on the image codecs
(a kernel restructuring that keeps every summation order must reproduce the previous build's bits).
  python3 tools/lib_bitwise.py dump OUT.npz      (with DGS_LIB=... selecting the build)
  python3 tools/lib_bitwise.py dump_ssim OUT.npz
  python3 tools/lib_bitwise.py dump_codecs OUT.npz
  python3 tools/lib_bitwise.py cmp A.npz B.npz
dump runs DeformNetworkBaseline forward + backward (blender and non-blender; frame-uniform t and
per-point t; ragged N), then the same forward under torch.no_grad (the inference kernels), and stores
the outputs and every parameter gradient. dump_ssim stores l1_ssim_loss's three outputs and dL/dimg
(upstream gradient 1 and 3) and image_metrics' raw (F, 3 + 10 C) output, NaN slots included, on seeded
images. dump_codecs stores the packed streams, offsets and lengths of png_gpu.encode_streams and of
jpeg_gpu.encode_streams (with its flags; three samplings, qualities 75 / 90 / 100, and once a capacity that the
frames exceed) on seeded frames: 256x256 discs, noise, constants, odd sizes, two 800x800 renders of the synthetic
scene; and the uint8 output of the device JPEG decoder on the files of tests/golden/jpeg_ingest.npz. cmp compares
bytes, not values."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))


def dump(path):
    import torch
    from deformgs.deform_network import DeformNetworkBaseline
    dev = torch.device("cuda", 0)
    out = {}
    for blender in (True, False):
        for N in (100_000, 4099, 70001, 17):
            for uniform in (True, False):
                torch.manual_seed(N + 7 * blender)
                net = DeformNetworkBaseline(is_blender=blender).to(dev)
                x = torch.rand(N, 3, device=dev) * 2.6 - 1.3
                t = torch.full((1, 1), 0.3, device=dev).expand(N, -1) if uniform else torch.rand(N, 1, device=dev)
                d_xyz, d_rot, d_s = net(x, t)
                (d_xyz.square().sum() + d_rot.sum() + d_s.abs().sum()).backward()
                key = f"{'bl' if blender else 'nb'}_{N}_{'u' if uniform else 'p'}"
                for name, v in (("d_xyz", d_xyz), ("d_rot", d_rot), ("d_s", d_s)):
                    out[f"{key}/{name}"] = v.detach().cpu().numpy()
                for name, p in net.named_parameters():
                    out[f"{key}/g_{name}"] = p.grad.detach().cpu().numpy()
                # the inference forward (no saved activations): the folded-t_emb kernel for the stride-0
                # t (DGS_MLP_UNIFORM_T, as renderer.py calls it), the per-point kernel otherwise
                with torch.no_grad():
                    for name, v in zip(("d_xyz", "d_rot", "d_s"), net(x, t)):
                        out[f"{key}/nograd_{name}"] = v.cpu().numpy()
    np.savez(path, **out)
    print(f"dumped {len(out)} arrays to {path}")


def dump_ssim(path):
    import torch
    from deformgs.image_metrics import image_metrics
    from deformgs.loss import l1_ssim_loss
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)

    def pair(*shape):  # a target and a render close to it, as the loss and the scores see them
        gt = torch.rand(shape, generator=gen)
        return (gt + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1).to(dev), gt.to(dev)

    out = {}
    for shape in ((3, 800, 800), (3, 61, 83), (1, 16, 16), (3, 5, 200)):
        img, gt = pair(*shape)
        for up in (1.0, 3.0):
            x = img.clone().requires_grad_(True)
            loss, l1, s = l1_ssim_loss(x, gt)
            (up * loss).backward()
            key = "loss_" + "x".join(map(str, shape)) + f"_up{up:g}"
            out[key + "/out3"] = torch.stack([loss.detach(), l1, s]).cpu().numpy()
            out[key + "/dimg"] = x.grad.cpu().numpy()
    # the CASES of tests/test_gpu_image_metrics.py (F, H, W; three channels), every metric; a small batch without MS-SSIM
    for (F, H, W), names in (((3, 161, 163), ("psnr", "ssim", "ms_ssim")), ((3, 200, 176), ("psnr", "ssim", "ms_ssim")),
                             ((1, 161, 163), ("psnr", "ssim", "ms_ssim")), ((2, 37, 45), ("psnr", "ssim"))):
        img, gt = pair(F, 3, H, W)
        raw = image_metrics(img, gt, names)["levels"]._base  # the (F, 3 + 10 C) tensor dgs_image_metrics wrote
        assert raw.shape == (F, 33), raw.shape
        out[f"metrics_{F}x3x{H}x{W}"] = raw.cpu().numpy()
    np.savez(path, **out)
    print(f"dumped {len(out)} arrays to {path}")


def dump_codecs(path):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from deformgs import ingest, jpeg_gpu, png_gpu
    from encode_time import render
    from png_fixtures import disc_image
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)

    def discs(h, w, t, bg):
        d = disc_image(w, h, t, n_discs=5, seed=3).astype(np.int32)
        return ((d[:, :, :3] * d[:, :, 3:] + bg * (255 - d[:, :, 3:]) + 127) // 255).astype(np.uint8)

    rgb = {"discs_256": np.stack([discs(256, 256, 0.2, 0), discs(256, 256, 0.7, 255)]),
           "noise_120x160": rng.integers(0, 256, (1, 120, 160, 3), dtype=np.uint8),
           "const_256": np.stack([np.full((256, 256, 3), 77, np.uint8), np.zeros((256, 256, 3), np.uint8)]),
           "mixed_67x173": np.stack([discs(67, 173, 0.1, 0), rng.integers(0, 256, (67, 173, 3), dtype=np.uint8),
                                     np.full((67, 173, 3), 9, np.uint8)]),
           "one_pixel": rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8),
           "render_800": render(2, 800, 100000, dev).cpu().numpy()}
    grey = {"grey_discs_250x300": discs(250, 300, 0.6, 0)[None, :, :, 1], "grey_zeros_64x1024": np.zeros((1, 64, 1024), np.uint8),
            "grey_7x1": rng.integers(0, 256, (1, 7, 1), dtype=np.uint8)}
    out = {}

    def store(key, packed, offsets, lengths, flags=None):
        where = torch.stack([offsets, lengths]).cpu().numpy()
        end = min(int(where[0, -1] + where[1, -1]), packed.numel())
        if flags is not None:  # a frame that did not fit was not written: its bytes are whatever the buffer held
            out[key + "/flags"] = flags.cpu().numpy()
            ok = np.flatnonzero(out[key + "/flags"] == 0)
            end = int(where[0, ok[-1]] + where[1, ok[-1]]) if ok.size else 0
        out[key + "/packed"], out[key + "/offsets"], out[key + "/lengths"] = packed[:end].cpu().numpy(), where[0], where[1]

    for name, a in {**rgb, **grey}.items():
        store("png_" + name, *png_gpu.encode_streams(torch.from_numpy(np.ascontiguousarray(a)).to(dev)))
    for name, a in rgb.items():
        frames = torch.from_numpy(a).to(dev)
        for sub in jpeg_gpu.SAMPLING:
            for q in (75, 90, 100):
                store(f"jpeg_{name}_{sub}_q{q}", *jpeg_gpu.encode_streams(frames, q, sub, capacity=4 * a.size + 4096))
    a = rgb["mixed_67x173"]  # the noise frame does not fit: flagged, and only the frame before it is written
    store("jpeg_mixed_67x173_4:2:0_q90_cap8000", *jpeg_gpu.encode_streams(torch.from_numpy(a).to(dev), 90, "4:2:0", capacity=8000))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_ingest.npz"))
    for c in gold["cases"]:
        out[f"decode_{c}"] = ingest.ingest_images([gold[f"{c}_jpg"].tobytes()], False, device=dev, return_uint8=True)[1][0].cpu().numpy()
    np.savez(path, **out)
    print(f"dumped {len(out)} arrays to {path}")


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "different keys"
    bad = [k for k in a.files if a[k].tobytes() != b[k].tobytes()]
    print(f"{len(a.files)} arrays, {len(bad)} differ bitwise")
    for k in bad[:20]:
        d = np.nanmax(np.abs(a[k].astype(np.float64) - b[k]))
        print(f"  {k}: max|d| {d:.3g} (max|a| {np.abs(a[k]).max():.3g})")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] in ("dump", "dump_ssim", "dump_codecs"):
        {"dump": dump, "dump_ssim": dump_ssim, "dump_codecs": dump_codecs}[sys.argv[1]](sys.argv[2])
    else:
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
