"""GPU: a Colmap directory (tests/golden/colmap_tiny: ten 44x28 baseline JPEGs, 4:4:4 and 4:2:0 alternating, names
whose string order is not their numeric order) through ingest on the device and train -> render -> metrics
through the three scripts' main(argv), in process. Sixty iterations prove plumbing, not quality: there is no PSNR
bar."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SORTED = ["0", "1", "10", "11", "2", "3", "4", "5", "6", "7"]
TEST = ["0", "6"]
TRAIN = [n for n in SORTED if n not in TEST]


@pytest.fixture(scope="module")
def src(golden_dir, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("colmap") / "colmap_tiny")
    shutil.copytree(os.path.join(golden_dir, "colmap_tiny"), out)
    return out


class _NoGaussians:
    def create_from_pcd(self, pcd, extent, device=None):
        pass


def _scene(src, model, device, **kw):
    """The CPU scene only loads images: its Gaussians are a stand-in (the initialisation's kNN is a device op)."""
    from deformgs.arguments import ModelParams
    from deformgs.dataset import Scene
    from deformgs.gaussian_model import GaussianModel
    g = GaussianModel(3) if device != "cpu" else _NoGaussians()
    return Scene(ModelParams(source_path=src, model_path=model, eval=True, is_blender=False, data_device=device, **kw), g), g


@pytest.mark.parametrize("resolution", [-1, 2], ids=["1x", "r2"])
def test_loaded_images_equal_the_cpu_path(src, golden_dir, tmp_path, resolution):
    dev, _ = _scene(src, str(tmp_path / "dev"), "cuda:0", resolution=resolution)
    cpu, _ = _scene(src, str(tmp_path / "cpu"), "cpu", resolution=resolution)
    gold = np.load(os.path.join(golden_dir, "colmap_tiny.npz"))
    for a, b in ((dev.getTrainCameras(), cpu.getTrainCameras()), (dev.getTestCameras(), cpu.getTestCameras())):
        assert [c.image_name for c in a] == [c.image_name for c in b] and len(a) in (8, 2)
        for x, y in zip(a, b):
            assert x.original_image.is_cuda and x.original_image.shape == ((3, 28, 44) if resolution == -1 else (3, 14, 22))
            assert torch.equal(x.original_image.cpu(), y.original_image)
            if resolution == 2:  # the reference's own PILtoTorch
                assert np.array_equal(x.original_image.cpu().numpy(), gold["half_22x14"][SORTED.index(x.image_name)])
    assert [c.image_name for c in dev.getTrainCameras()] == TRAIN and [c.image_name for c in dev.getTestCameras()] == TEST


def test_train_render_metrics_on_a_colmap_directory(src, tmp_path, monkeypatch, capsys):
    from deformgs import metrics, render_cli, train
    from deformgs.jpeg import read_jpeg
    from deformgs.png import read_png
    m = str(tmp_path / "model")
    seen = []
    real_training = train.training

    def spy(dataset, opt, pipe, tests, saves, scene, gaussians, *a, **kw):
        seen.append((dataset, scene, gaussians))
        return real_training(dataset, opt, pipe, tests, saves, scene, gaussians, *a, **kw)

    monkeypatch.setattr(train, "training", spy)
    out = train.main(["-s", src, "-m", m, "--non-blender", "--eval", "--iterations", "60", "--warm-up", "20",
                      "--sequence-length", "8", "--save_iterations", "60"])
    assert math.isfinite(out["final_loss"]) and out["iterations"] == 60
    (dataset, scene, gaussians), = seen
    assert not dataset.is_blender and scene.format == "Colmap" and dataset.images == "images"
    assert [c.image_name for c in scene.getTrainCameras()] == TRAIN and [c.image_name for c in scene.getTestCameras()] == TEST
    assert scene.getTrainCameras()[0].original_image.shape == (3, 28, 44)
    assert getattr(gaussians, "_dgs_native", None) is not None, "the loop must take the native step"
    assert out["final_gaussians"] == 300 and "warning" not in capsys.readouterr().out
    for rel in ("point_cloud/iteration_60/point_cloud.ply", "deform/iteration_60/deform.pth", "cameras.json",
                "cfg_args", "input.ply"):
        assert os.path.isfile(os.path.join(m, rel)), rel
    with open(os.path.join(m, "cameras.json")) as f:
        assert [c["img_name"] for c in json.load(f)][:2] == TEST
    assert not os.path.exists(os.path.join(src, "sparse", "0", "points3D.ply"))  # SOURCE is not written

    (done,) = render_cli.main(["-m", m, "-s", src, "--non_blender", "--skip_train"])
    assert done == os.path.join(m, "test", "ours_60")
    for sub in ("renders", "depth", "gt"):
        assert sorted(os.listdir(os.path.join(done, sub))) == ["00000.png", "00001.png"]
    for i, name in enumerate(TEST):
        want = read_jpeg(os.path.join(src, "images", name + ".jpg"))
        assert want.shape == (28, 44, 3)
        assert np.array_equal(read_png(os.path.join(done, "gt", f"{i:05d}.png")), want)
        assert read_png(os.path.join(done, "renders", f"{i:05d}.png")).shape == (28, 44, 3)
    # -r 2 without --res: the dataset's own size after the -r rule; --res: that size
    (d,) = render_cli.main(["-m", m, "-s", src, "--non_blender", "--skip_train", "--mode", "time", "--frames", "3",
                            "--view_index", "1", "-r", "2"])
    files = sorted(os.listdir(os.path.join(d, "renders")))
    assert files and read_png(os.path.join(d, "renders", files[0])).shape == (14, 22, 3)
    (d,) = render_cli.main(["-m", m, "-s", src, "--non_blender", "--skip_test", "--res", "20", "12", "-i", "images"])
    assert read_png(os.path.join(d, "gt", "00000.png")).shape == (12, 20, 3) and len(os.listdir(os.path.join(d, "gt"))) == 8

    metrics.main(["-m", m])
    with open(os.path.join(m, "results.json")) as f:
        res = json.load(f)["ours_60"]
    assert math.isfinite(res["PSNR"]) and math.isfinite(res["SSIM"])
    with open(os.path.join(m, "per_view.json")) as f:
        assert sorted(json.load(f)["ours_60"]["PSNR"]) == ["00000.png", "00001.png"]


def test_training_a_colmap_directory_with_the_blender_network_warns(src, tmp_path, capsys):
    from deformgs import train
    out = train.main(["-s", src, "-m", str(tmp_path / "model"), "--eval", "--iterations", "2", "--warm-up", "1",
                      "--sequence-length", "8"])
    assert math.isfinite(out["final_loss"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("warning")]
    assert len(lines) == 1 and "Colmap" in lines[0] and "--non-blender" in lines[0]
