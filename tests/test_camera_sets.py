"""CPU: the render script's camera sets, the training readers' point-cloud start-up (without a model_path and
with one) and Scene's written files against tests/golden/camera_sets.npz, which
tests/golden/make_golden_camera_sets.py recorded from the code before the data layer's shared steps were
stated once. Every comparison is exact: equal names, dtypes, shapes and values.

Scene is built whole, with data_device "cpu" and a stand-in Gaussian model that only keeps what create_from_pcd
is handed: cameras.json, input.ply, cameras_extent and both camera lists are Scene's own."""
import os

import numpy as np
import pytest

import camera_sets_cases as cases


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "camera_sets.npz")))


def _side(gold, prefix):
    return sorted(k for k in gold if k.startswith(prefix))


def test_render_side(gold):
    got = cases.render_side("cpu")
    assert sorted(got) == _side(gold, "render/")
    cases.compare(got, gold)
    # what the cases are there for: both grounds differ, a forced size keeps the files' views, "other" has no test set
    assert not np.array_equal(gold["render/dnerf_white/train/image0"], gold["render/dnerf_black/train/image0"])
    assert gold["render/colmap_res20x12/train/image0"].shape == (3, 12, 20)
    assert gold["render/colmap_r2/train/image0"].shape == (3, 14, 22)
    assert gold["render/nerfies_none_r-1/test/uid"].shape == (0,) and gold["render/nerfies_vrig_r-1/test/uid"].size > 0


def test_training_side(gold, tmp_path):
    got = cases.training_side(str(tmp_path))
    assert sorted(got) == _side(gold, "train/")
    cases.compare(got, gold)
    assert gold["train/dnerf_memory/ply_path"] == "none" and gold["train/colmap_model/ply_path"] == "MODEL/input.ply"


def test_scene(gold, tmp_path):
    got = cases.scene_side(str(tmp_path))
    assert sorted(got) == _side(gold, "scene/")
    cases.compare(got, gold)
