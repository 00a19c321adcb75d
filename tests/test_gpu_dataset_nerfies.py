"""GPU: a Nerfies-format directory (tests/golden/nerfies_tiny copied under a parent named NeRF-x: RGB, 44x28,
ragged against the 16-pixel raster tile and the 32-pixel SSIM tile on both axes) through ingest, one training
step, and train -> render -> metrics through the three scripts' main(argv), in process. Sixty iterations prove
plumbing, not quality: there is no PSNR bar."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

IDS = [f"{i:06d}" for i in range(12)]
VAL = IDS[1::4]


@pytest.fixture(scope="module")
def src(golden_dir, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nerfies") / "NeRF-x" / "nerfies_tiny")
    shutil.copytree(os.path.join(golden_dir, "nerfies_tiny"), out)
    return out


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "nerfies_tiny.npz")))


@pytest.mark.parametrize("resolution", [1, 2], ids=["1x", "r2"])
def test_device_ingest_of_rgb_equals_the_cpu_path(src, gold, resolution):
    from deformgs import ingest
    from deformgs.dataset import target_resolution
    paths = [os.path.join(src, "rgb", "1x", n + ".png") for n in IDS]
    size = lambda w, h: target_resolution(w, h, resolution)  # noqa: E731
    for white in (False, True):  # no alpha: the background must not matter
        dev, dev8 = ingest.ingest_images(paths, white, size=size, device="cuda", return_uint8=True)
        cpu, cpu8 = ingest.ingest_images(paths, white, size=size, device="cpu", return_uint8=True)
        assert dev.shape == ((12, 3, 28, 44) if resolution == 1 else (12, 3, 14, 22)) and dev.is_cuda
        assert torch.equal(dev.cpu(), cpu) and torch.equal(dev8.cpu(), cpu8)
    if resolution == 2:
        assert np.array_equal(dev.cpu().numpy(), gold["resized_1x_22x14"])  # the reference's own PILtoTorch


def _scene(src, model):
    from deformgs.arguments import ModelParams
    from deformgs.dataset import Scene
    from deformgs.gaussian_model import GaussianModel
    g = GaussianModel(3)
    return Scene(ModelParams(source_path=src, model_path=model, eval=True, is_blender=False, data_device="cuda:0"), g), g


def _models(g0, opt, seed=0):
    """A fresh copy of the scene's initial Gaussians and a seeded non-blender network with small heads."""
    from deformgs.deform_model import DeformModelBaseline
    from deformgs.gaussian_model import GaussianModel
    gs = GaussianModel(3)
    gs.from_tensors(g0._xyz, g0._features_dc, g0._features_rest, g0._scaling, g0._rotation, g0._opacity,
                    active_sh_degree=0)
    torch.manual_seed(seed)
    deform = DeformModelBaseline(is_blender=False, is_6dof=False, device=g0._xyz.device)
    with torch.no_grad():  # a trained network's small deltas
        for h in (deform.deform.gaussian_warp, deform.deform.gaussian_rotation, deform.deform.gaussian_scaling):
            h.weight.mul_(0.01)
            h.bias.mul_(0.01)
    return gs, deform


def _params(gs, deform):
    return [gs._xyz, gs._features_dc, gs._features_rest, gs._scaling, gs._rotation, gs._opacity] + \
        list(deform.deform.parameters())


def test_one_step_at_44x28_matches_the_torch_glue(src, tmp_path):
    """The fused step (native path: HIP network, raster, L1 + SSIM) on a fixture camera against the same step
    through the torch glue, at the bars of tests/test_gpu_train.py for this comparison: losses within 2e-4
    relative; Gaussian tensors ||a - b|| <= 1e-3 ||b|| and network tensors 10 %, applied here to the step's
    gradients (one Adam step from fresh moments keeps only their signs). Then two iterations of training()
    both ways (one optimizer step in between): the same Gaussian count and losses within 2e-4."""
    from deformgs.arguments import ModelParams, OptimizationParams, PipelineParams
    from deformgs.renderer import set_fused
    from deformgs.train import _glue_step, training
    from deformgs.train_step import train_step
    scene, g0 = _scene(src, str(tmp_path / "model"))
    dev = g0._xyz.device
    assert g0._xyz.shape[0] == 500
    cam = scene.getTrainCameras()[4]
    gt = cam.original_image
    assert gt.shape == (3, 28, 44) and gt.is_contiguous()
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    noise = torch.full((1, 1), -0.013, device=dev)
    opt = OptimizationParams()
    runs = {}
    for fused in (True, False):
        gs, deform = _models(g0, opt)
        gs.training_setup(opt)
        deform.train_setting(opt)
        if fused:
            loss, pkg, redone = train_step(gs, deform, cam, gt, pipe, bg, False, opt.lambda_dssim, True, noise,
                                           deferred_count=False)
            assert getattr(gs, "_dgs_native", None) is not None, "train_step must take the native path here"
            assert not redone and pkg["num_rendered"] > 0
        else:
            set_fused(False)
            try:
                loss, pkg = _glue_step(gs, deform, cam, gt, pipe, bg, False, opt.lambda_dssim, True, noise)
            finally:
                set_fused(True)
        torch.cuda.synchronize()
        assert pkg["render"].shape == (3, 28, 44) and int(pkg["visibility_filter"].sum()) > 100
        runs[fused] = (float(loss.detach()), pkg["render"].detach().clone(), [p.grad.detach().clone() for p in _params(gs, deform)])
    (la, ia, ga), (lb, ib, gb) = runs[True], runs[False]
    print("loss", la, lb, "image max diff", float((ia - ib).abs().max()))
    assert math.isfinite(la) and abs(la - lb) <= 2e-4 * abs(lb)
    for i, (a, b) in enumerate(zip(ga, gb)):
        err, ref = float((a - b).norm()), float(b.norm())
        print("grad", i, tuple(a.shape), err, ref)
        assert err <= (1e-3 if i < 6 else 0.1) * ref, (i, err, ref)
    assert float(gb[0].norm()) > 0 and float(gb[6].norm()) > 0
    hist = {}
    for fused in (True, False):
        gs, deform = _models(g0, opt)
        hist[fused] = training(ModelParams(is_blender=False), OptimizationParams(iterations=2, warm_up=1, sequence_length=8),
                               pipe, [], [], scene, gs, deform, fused=fused, seed=0)
    assert hist[True]["n"] == hist[False]["n"] == [500, 500]
    ha, hb = np.array(hist[True]["loss"]), np.array(hist[False]["loss"])
    print("loop losses", ha, hb)
    assert np.all(np.isfinite(ha)) and np.all(np.abs(ha - hb) <= 2e-4 * np.abs(hb))


def test_train_render_metrics_on_a_nerfies_directory(src, tmp_path, monkeypatch, capsys):
    from deformgs import metrics, render_cli, train
    from deformgs.png import read_png
    m = str(tmp_path / "model")
    seen = []
    real_training = train.training

    def spy(dataset, opt, pipe, tests, saves, scene, gaussians, *a, **kw):
        seen.append((dataset, scene, gaussians))
        return real_training(dataset, opt, pipe, tests, saves, scene, gaussians, *a, **kw)

    monkeypatch.setattr(train, "training", spy)
    out = train.main(["-s", src + "/", "-m", m, "--non-blender", "--eval", "--iterations", "60", "--warm-up", "20",
                      "--sequence-length", "8", "--save_iterations", "60"])
    assert math.isfinite(out["final_loss"]) and out["iterations"] == 60
    (dataset, scene, gaussians), = seen
    assert not dataset.is_blender and scene.format == "Nerfies"
    assert len(scene.getTrainCameras()) == 9 and len(scene.getTestCameras()) == 3
    assert scene.getTrainCameras()[0].original_image.shape == (3, 28, 44)
    assert getattr(gaussians, "_dgs_native", None) is not None, "the loop must take the native step"
    assert out["final_gaussians"] == 500 and "warning" not in capsys.readouterr().out
    for rel in ("point_cloud/iteration_60/point_cloud.ply", "deform/iteration_60/deform.pth", "cameras.json",
                "cfg_args", "input.ply"):
        assert os.path.isfile(os.path.join(m, rel)), rel
    with open(os.path.join(m, "cameras.json")) as f:
        assert [c["img_name"] for c in json.load(f)][:3] == VAL

    (done,) = render_cli.main(["-m", m, "-s", src, "--non_blender", "--skip_train"])
    assert done == os.path.join(m, "test", "ours_60")
    for sub in ("renders", "depth", "gt"):
        assert sorted(os.listdir(os.path.join(done, sub))) == ["00000.png", "00001.png", "00002.png"]
    for i, name in enumerate(VAL):
        want = read_png(os.path.join(src, "rgb", "1x", name + ".png"))
        assert want.shape == (28, 44, 3)
        assert np.array_equal(read_png(os.path.join(done, "gt", f"{i:05d}.png")), want)
        assert read_png(os.path.join(done, "renders", f"{i:05d}.png")).shape == (28, 44, 3)
    # the other modes, and -r 2 without --res: the dataset's own size after the -r rule
    for mode in ("time", "view", "all", "pose", "original"):
        (d,) = render_cli.main(["-m", m, "-s", src, "--non_blender", "--skip_train", "--mode", mode, "--frames", "3",
                                "--view_index", "1", "-r", "2"])
        files = sorted(os.listdir(os.path.join(d, "renders")))
        assert files and read_png(os.path.join(d, "renders", files[0])).shape == (14, 22, 3), mode

    metrics.main(["-m", m])
    with open(os.path.join(m, "results.json")) as f:
        res = json.load(f)["ours_60"]
    assert math.isfinite(res["PSNR"]) and math.isfinite(res["SSIM"])
    with open(os.path.join(m, "per_view.json")) as f:
        assert sorted(json.load(f)["ours_60"]["PSNR"]) == ["00000.png", "00001.png", "00002.png"]


def test_training_a_nerfies_directory_with_the_blender_network_warns(src, tmp_path, capsys):
    from deformgs import train
    out = train.main(["-s", src, "-m", str(tmp_path / "model"), "--eval", "--iterations", "2", "--warm-up", "1",
                      "--sequence-length", "8"])
    assert math.isfinite(out["final_loss"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("warning")]
    assert len(lines) == 1 and "Nerfies" in lines[0] and "--non-blender" in lines[0]
