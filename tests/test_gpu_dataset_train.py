"""GPU: train -> render -> metrics on tests/golden/dnerf_tiny through the three scripts' main(argv), in process.
Sixty iterations prove plumbing, not quality: there is no PSNR bar."""
import json
import math
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


def test_train_render_metrics_on_a_dataset_directory(golden_dir, tmp_path):
    from deformgs import ingest, metrics, render_cli, train
    from deformgs.png import read_png
    tiny = os.path.join(golden_dir, "dnerf_tiny")
    m = str(tmp_path / "model")
    out = train.main(["-s", tiny, "-m", m, "--eval", "--init_points", "2000", "--iterations", "60", "--warm-up", "20",
                      "--save_iterations", "60"])
    assert math.isfinite(out["final_loss"]) and out["iterations"] == 60
    for rel in ("point_cloud/iteration_60/point_cloud.ply", "deform/iteration_60/deform.pth", "cameras.json",
                "cfg_args", "input.ply"):
        assert os.path.isfile(os.path.join(m, rel)), rel
    with open(os.path.join(m, "cameras.json")) as f:
        assert len(json.load(f)) == 8

    (done,) = render_cli.main(["-m", m, "-s", tiny, "--res", "32", "32", "--skip_train"])
    assert done == os.path.join(m, "test", "ours_60")
    assert sorted(os.listdir(os.path.join(done, "gt"))) == ["00000.png", "00001.png"]
    rgba = read_png(os.path.join(tiny, "test", "r_000.png"))
    assert rgba.shape == (32, 32, 4)
    assert np.array_equal(read_png(os.path.join(done, "gt", "00000.png")), ingest.composite_numpy(rgba, False))

    metrics.main(["-m", m])
    with open(os.path.join(m, "results.json")) as f:
        res = json.load(f)["ours_60"]
    assert math.isfinite(res["PSNR"]) and math.isfinite(res["SSIM"])
