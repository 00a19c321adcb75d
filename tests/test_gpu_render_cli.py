"""The render and metrics scripts end to end on the synthetic scene (2000 Gaussians, 64 x 48)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ARGS = ["--synthetic", "2000", "--res", "64", "48"]


def test_time_mode_writes_the_frames_of_a_direct_call(tmp_path):
    from deformgs import render_cli
    from deformgs.png import read_png
    from deformgs.render_frames import render_frames
    m = str(tmp_path / "model")
    argv = ["-m", m, *ARGS, "--mode", "time", "--frames", "5", "--view_index", "2", "--skip_train"]
    (out,) = render_cli.main(argv)
    assert out == os.path.join(m, "test", "interpolate_0")
    for sub in ("renders", "depth"):
        assert sorted(os.listdir(os.path.join(out, sub))) == [f"{i:05d}.png" for i in range(5)]
    assert not os.path.exists(os.path.join(out, "gt"))
    # the same frames from a direct call on the saved model
    gaussians, deform, cams, bg, it = render_cli.load_scene(render_cli.build_parser().parse_args(argv))
    assert it == 0
    view = cams.test[2]
    direct = render_frames([view] * 5, gaussians, deform, bg, times=[i / 4 for i in range(5)], outputs=("rgb8", "depth8"))
    assert direct["rgb8"].float().std() > 1  # a real image
    for i in range(5):
        rgb = read_png(os.path.join(out, "renders", f"{i:05d}.png"))
        dep = read_png(os.path.join(out, "depth", f"{i:05d}.png"))
        assert rgb.shape == (48, 64, 3) and dep.shape == (48, 64)
        assert np.array_equal(rgb, direct["rgb8"][i].cpu().numpy())
        assert np.array_equal(dep, direct["depth8"][i].cpu().numpy())


def test_render_then_metrics(tmp_path):
    from deformgs import loss, metrics, render_cli
    from deformgs.png import read_png
    m = str(tmp_path / "model")
    (out,) = render_cli.main(["-m", m, *ARGS, "--mode", "render", "--skip_train"])
    assert out == os.path.join(m, "test", "ours_0")
    names = sorted(os.listdir(os.path.join(out, "renders")))
    assert names == [f"{i:05d}.png" for i in range(5)] and sorted(os.listdir(os.path.join(out, "gt"))) == names
    metrics.main(["-m", m])
    with open(os.path.join(m, "results.json")) as f:
        results = json.load(f)
    with open(os.path.join(m, "per_view.json")) as f:
        per_view = json.load(f)
    assert list(results) == ["ours_0"] and results["ours_0"]["LPIPS"] is None
    t = lambda a: (torch.from_numpy(a).cuda().permute(2, 0, 1).contiguous().float() / 255.0).unsqueeze(0)  # noqa: E731
    pairs = [(t(read_png(os.path.join(out, "renders", n))), t(read_png(os.path.join(out, "gt", n)))) for n in names]
    ps = [float(loss.psnr(r, g)) for r, g in pairs]
    assert results["ours_0"]["PSNR"] == torch.tensor(ps).mean().item()
    assert [per_view["ours_0"]["PSNR"][n] for n in names] == torch.tensor(ps).tolist()
    # the fused kernel's SSIM against the torch statement of the same window: tests/test_gpu_loss.py holds the
    # kernel to 1e-6 of the golden value; 10x that here for the summation order of torch's device convolution
    ss = [float(loss.ssim(r, g)) for r, g in pairs]
    print("SSIM fused", results["ours_0"]["SSIM"], "torch", float(np.mean(ss)))
    assert abs(results["ours_0"]["SSIM"] - float(np.mean(ss))) < 1e-5
    assert 0.0 < results["ours_0"]["SSIM"] <= 1.0 and np.isfinite(results["ours_0"]["PSNR"])
