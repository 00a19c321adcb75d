"""CPU: the Nerfies-format reader (NeRF-DS / HyperNeRF) on tests/golden/nerfies_tiny against
tests/golden/nerfies_tiny.npz, a run of the reference's own readNerfiesCameras / getNerfppNorm / PILtoTorch
(tests/golden/make_golden_nerfies.py). The fixture is copied under a parent directory named for each split
branch. The float64 camera fields are the reference's expressions in its order: they are compared bitwise."""
import json
import os
import shutil

import numpy as np
import pytest

from deformgs import dataset
from deformgs.png import read_png

PARENTS = {"vrig": "vrig-x", "nerf": "NeRF-x", "interp": "interp-x", "other": "misc"}
IDS = [f"{i:06d}" for i in range(12)]
VAL = IDS[1::4]
TRAIN = [n for n in IDS if n not in VAL]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "nerfies_tiny.npz")))


@pytest.fixture(scope="module")
def copies(golden_dir, tmp_path_factory):
    """{branch: a copy of nerfies_tiny/ under the parent directory that selects the branch}; read only."""
    root = tmp_path_factory.mktemp("nerfies")
    out = {}
    for b, parent in PARENTS.items():
        out[b] = str(root / parent / "nerfies_tiny")
        shutil.copytree(os.path.join(golden_dir, "nerfies_tiny"), out[b])
    return out


def _tree(root):
    return sorted((os.path.relpath(os.path.join(d, f), root), os.path.getsize(os.path.join(d, f)))
                  for d, _, fs in os.walk(root) for f in fs)


def _same_cameras(cams, train_num, gold, b):
    assert train_num == int(gold[f"{b}_train_num"])
    assert [c.image_name for c in cams] == gold[f"{b}_name"].tolist()
    assert [c.uid for c in cams] == list(range(len(cams)))
    assert [c.width for c in cams] == gold[f"{b}_width"].tolist()
    assert [c.height for c in cams] == gold[f"{b}_height"].tolist()
    for key in ("R", "T", "FovX", "FovY", "fid"):
        got = np.stack([np.asarray(getattr(c, key), np.float64) for c in cams])
        want = gold[f"{b}_{key}"]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (b, key, np.abs(got - want).max())


@pytest.mark.parametrize("b", list(PARENTS))
def test_split_branch_reproduces_the_reference(copies, gold, b):
    cams, train_num, center, scale = dataset.read_nerfies_cameras(copies[b])
    _same_cameras(cams, train_num, gold, b)
    assert (center, scale) == ([0.3, -0.2, 1.1], 0.35)
    size, n = {"vrig": ((11, 7), 12), "nerf": ((44, 28), 12), "interp": ((22, 14), 6), "other": ((22, 14), 3)}[b]
    assert len(cams) == n and {(c.width, c.height) for c in cams} == {size}
    assert all(c.image_path == os.path.join(copies[b], "rgb", f"{44 // size[0]}x", c.image_name + ".png") for c in cams)
    for ev, suffix in ((True, ""), (False, "_all")):
        info = dataset.read_nerfies(copies[b], ev)
        norm = info.nerf_normalization
        assert np.asarray(norm["translate"]).tobytes() == gold[f"{b}_translate{suffix}"].tobytes()
        assert np.asarray(norm["radius"]).tobytes() == gold[f"{b}_radius{suffix}"].tobytes()
    assert 1.0 < float(gold[f"{b}_radius"]) < 10.0


def test_split_rule_names(copies):
    names = {b: [c.image_name for c in dataset.read_nerfies_cameras(copies[b])[0]] for b in PARENTS}
    assert names["vrig"] == names["nerf"] == TRAIN + VAL
    assert names["interp"] == IDS[::4] + IDS[2::4]
    assert names["other"] == IDS[::4]
    for name, kind in (("vrig-x", "vrig"), ("NeRF-DS", "nerf"), ("nerfds", "nerf"), ("interp_a", "interp"),
                       ("hypernerf", "interp"), ("misc", "other"), ("Vrig", "other")):
        assert dataset.nerfies_kind_of(f"/data/{name}/scene") == kind
        assert dataset.nerfies_kind_of(f"/data/{name}/scene/") == kind


@pytest.mark.parametrize("b", list(PARENTS))
def test_trailing_slash_and_relative_path_do_not_change_the_split(copies, gold, b, monkeypatch):
    cams, train_num, _, _ = dataset.read_nerfies_cameras(copies[b] + "/")
    _same_cameras(cams, train_num, gold, b)
    monkeypatch.chdir(copies[b])
    rel, rel_num, _, _ = dataset.read_nerfies_cameras(".")
    assert rel_num == train_num and [c.image_name for c in rel] == [c.image_name for c in cams]
    assert [c.fid for c in rel] == [c.fid for c in cams]


def test_nerfies_kind_overrides_the_directory_name(copies, gold):
    for b in PARENTS:  # every branch, read from the copy whose parent directory says `other`
        cams, train_num, _, _ = dataset.read_nerfies_cameras(copies["other"], nerfies_kind=b)
        assert train_num == int(gold[f"{b}_train_num"])
        assert [c.image_name for c in cams] == gold[f"{b}_name"].tolist()
        assert np.array([c.fid for c in cams]).tobytes() == gold[f"{b}_fid"].tobytes()
    info = dataset.read_nerfies(copies["vrig"], True, nerfies_kind="nerf")
    assert (info.train_cameras[0].width, len(info.test_cameras)) == (44, 3)
    with pytest.raises(ValueError):
        dataset.read_nerfies_cameras(copies["other"], nerfies_kind="colmap")


def test_fid_is_time_id_over_the_largest_selected_time_id(copies):
    with open(os.path.join(copies["nerf"], "metadata.json")) as f:
        meta = json.load(f)
    for b, top in (("nerf", 16), ("other", 13)):  # `other` selects ids 0, 4, 8: its largest time_id is 13
        cams = dataset.read_nerfies_cameras(copies[b])[0]
        times = [meta[c.image_name]["time_id"] for c in cams]
        assert max(times) == top and min(times) == 3
        assert [c.fid for c in cams] == [t / top for t in times]
        assert max(c.fid for c in cams) == 1.0 and min(c.fid for c in cams) > 0.0
        # neither the frame count nor count - 1 gives these times
        assert all(c.fid != t / len(cams) and c.fid != t / (len(cams) - 1) for c, t in zip(cams, times))


def test_camera_fields_follow_the_written_formulas(copies):
    """Independent of the golden run: position = (position - center) * scale, R = orientation^T, T = -position R,
    focal * ratio, the fields of view from the PNG header's size; the old `tangential` key is accepted."""
    for b, ratio in (("vrig", 0.25), ("nerf", 1.0), ("interp", 0.5)):
        for cam in dataset.read_nerfies_cameras(copies[b])[0]:
            with open(os.path.join(copies[b], "camera", cam.image_name + ".json")) as f:
                cj = json.load(f)
            assert ("tangential" in cj) == (cam.image_name == "000003") == ("tangential_distortion" not in cj)
            pos = (np.array(cj["position"]) - np.array([0.3, -0.2, 1.1])) * 0.35
            assert abs(np.linalg.norm(pos) - 4.0) < 1e-9  # the fixture's orbit, in the scaled frame
            assert np.array_equal(cam.R, np.array(cj["orientation"]).T)
            assert np.allclose(cam.T, -np.array(cj["orientation"]) @ pos, atol=1e-12)
            w, h = dataset.png_size(cam.image_path)
            assert (w, h) == (round(44 * ratio), round(28 * ratio)) == (cam.width, cam.height)
            assert cam.FovX == dataset.focal2fov(40.0 * ratio, w) and cam.FovY == dataset.focal2fov(40.0 * ratio, h)
            # the camera looks at the origin of the scaled frame: it maps to (0, 0, 4) in view space
            assert np.allclose(cam.R.T @ np.zeros(3) + cam.T, [0, 0, 4.0], atol=1e-9)


def test_eval_off_merges_test_into_train(copies):
    on = dataset.read_nerfies(copies["nerf"], True)
    off = dataset.read_nerfies(copies["nerf"], False)
    assert [c.image_name for c in on.train_cameras] == TRAIN and [c.image_name for c in on.test_cameras] == VAL
    assert [c.image_name for c in off.train_cameras] == TRAIN + VAL and off.test_cameras == []
    assert [c.uid for c in on.test_cameras] == [9, 10, 11]
    assert dataset.read_nerfies(copies["other"], True).test_cameras == []


def test_point_cloud_from_points_npy_and_read_only_source(copies, tmp_path):
    src = copies["nerf"]
    before = _tree(src)
    model = str(tmp_path / "model")
    info = dataset.read_nerfies(src, True, model_path=model)
    want = (np.load(os.path.join(src, "points.npy")) - [0.3, -0.2, 1.1]) * 0.35
    pts, col = np.asarray(info.point_cloud.points), np.asarray(info.point_cloud.colors)
    assert pts.shape == (500, 3) and pts.dtype == np.float32 and np.array_equal(pts, want.astype(np.float32))
    assert 0.3 < pts.std() < 0.5 and np.abs(pts.mean(0)).max() < 0.1  # the fixture's blob around the origin
    # SH2RGB(U[0, 1) / 255) = 0.5 + C0 * tiny: 127 or 128 of 255 after the file's 8 bits
    assert set(np.unique(np.round(col * 255).astype(int))) <= {127, 128}
    assert info.ply_path == os.path.join(model, "input.ply") and os.path.isfile(info.ply_path)
    again = dataset.read_nerfies(src, True)  # no MODEL: the same cloud, nothing written
    assert again.ply_path is None
    assert np.array_equal(again.point_cloud.points, pts) and np.array_equal(again.point_cloud.colors, col)
    assert _tree(src) == before  # nothing is created under SOURCE
    assert os.listdir(model) == ["input.ply"]


def test_points3d_ply_is_used_and_a_missing_cloud_raises(copies, tmp_path):
    src = str(tmp_path / "NeRF-y" / "scene")
    shutil.copytree(copies["nerf"], src)
    xyz = np.random.default_rng(1).uniform(-1, 1, (9, 3))
    dataset.store_ply(os.path.join(src, "points3d.ply"), xyz, np.full((9, 3), 200.7))
    own = dataset.read_nerfies(src, True, model_path=str(tmp_path / "m"))
    assert np.array_equal(own.point_cloud.points, xyz.astype(np.float32))
    assert np.allclose(own.point_cloud.colors, 200 / 255.0)
    assert own.ply_path == os.path.join(src, "points3d.ply") and not os.path.exists(str(tmp_path / "m" / "input.ply"))
    os.remove(os.path.join(src, "points3d.ply"))
    os.remove(os.path.join(src, "points.npy"))
    with pytest.raises(ValueError, match=r"points3d\.ply.*points\.npy"):
        dataset.read_nerfies(src, True)


class _Gaussians:
    def create_from_pcd(self, pcd, extent, device=None):
        self.pcd, self.extent = pcd, extent


def _args(src, model, **kw):
    from deformgs.arguments import ModelParams
    return ModelParams(source_path=src, model_path=model, eval=True, data_device="cpu", **kw)


@pytest.mark.parametrize("marker,name", [("sparse", "Colmap"), ("cameras_sphere.npz", "DTU"),
                                         ("poses_bounds.npy", "plenoptic"), ("transforms.json", "Dynamic-360")])
def test_unsupported_formats_raise(tmp_path, marker, name):
    src = tmp_path / "src"
    if marker == "sparse":
        os.makedirs(src / marker)
    else:
        os.makedirs(src)
        (src / marker).write_bytes(b"")
    with pytest.raises(ValueError, match=f"{name}.*unsupported"):
        dataset.Scene(_args(str(src), str(tmp_path / "model")), _Gaussians())
    assert not os.path.exists(tmp_path / "model")


def test_unrecognised_directory_raises(tmp_path):
    os.makedirs(tmp_path / "src")
    with pytest.raises(ValueError, match="recognise"):
        dataset.Scene(_args(str(tmp_path / "src"), str(tmp_path / "model")), _Gaussians())


def test_dispatch_order_is_the_reference_s(copies, golden_dir, tmp_path):
    """scene/__init__.py:45-63: sparse/ wins over everything, transforms_train.json over dataset.json."""
    assert dataset.dataset_format(copies["nerf"]) == "Nerfies"
    assert dataset.dataset_format(os.path.join(golden_dir, "dnerf_tiny")) == "D-NeRF"
    both = str(tmp_path / "both")
    shutil.copytree(os.path.join(golden_dir, "dnerf_tiny"), both)
    shutil.copy(os.path.join(copies["nerf"], "dataset.json"), both)
    assert dataset.dataset_format(both) == "D-NeRF"
    os.makedirs(os.path.join(both, "sparse"))
    with pytest.raises(ValueError, match="Colmap"):
        dataset.dataset_format(both)


def test_scene_on_a_nerfies_directory(copies, gold, tmp_path):
    src = copies["nerf"]
    before = _tree(src)
    model = str(tmp_path / "model")
    g = _Gaussians()
    scene = dataset.Scene(_args(src, model, white_background=True, init_points=7), g)
    assert scene.format == "Nerfies"
    train, test = scene.getTrainCameras(), scene.getTestCameras()
    assert [c.image_name for c in train] == TRAIN and [c.image_name for c in test] == VAL
    batch = train[0].original_image._base
    assert batch is not None and batch.shape == (9, 3, 28, 44)  # one ingest batch per set
    for cams, b in ((train, batch), (test, test[0].original_image._base)):
        for i, cam in enumerate(cams):
            px = read_png(os.path.join(src, "rgb", "1x", cam.image_name + ".png"))
            assert px.shape == (28, 44, 3) and (cam.image_width, cam.image_height) == (44, 28)
            # RGB bytes / 255: no composite (white_background has no effect), no resize
            assert np.array_equal(cam.original_image.numpy(), px.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
            assert cam.original_image.data_ptr() == b[i].data_ptr()
    k = list(gold["nerf_name"]).index(train[4].image_name)
    assert float(train[4].fid) == np.float32(gold["nerf_fid"][k]) and train[4].FoVx == gold["nerf_FovX"][k]
    assert scene.cameras_extent == float(gold["nerf_radius"])
    assert g.pcd.points.shape == (500, 3) and g.extent == scene.cameras_extent  # init_points is ignored
    with open(os.path.join(model, "cameras.json")) as f:
        cj = json.load(f)
    assert [c["img_name"] for c in cj] == VAL + TRAIN and [c["id"] for c in cj] == list(range(12))  # test first
    assert {(c["width"], c["height"]) for c in cj} == {(44, 28)}
    assert all(abs(c["fx"] - 40.0) < 1e-9 and abs(c["fy"] - 40.0) < 1e-9 for c in cj)
    assert sorted(os.listdir(model)) == ["cameras.json", "cfg_args", "input.ply"]
    assert _tree(src) == before


def test_scene_resolution_2_matches_the_reference_resize(copies, gold, tmp_path):
    scene = dataset.Scene(_args(copies["nerf"], str(tmp_path / "model"), resolution=2), _Gaussians())
    cams = scene.getTrainCameras() + scene.getTestCameras()
    assert len(cams) == 12
    for cam in cams:
        assert (cam.image_width, cam.image_height) == (22, 14)
        assert np.array_equal(cam.original_image.numpy(), gold["resized_1x_22x14"][IDS.index(cam.image_name)])


def test_a_dnerf_directory_still_goes_to_the_dnerf_reader(golden_dir, tmp_path):
    tiny = os.path.join(golden_dir, "dnerf_tiny")
    g = _Gaussians()
    scene = dataset.Scene(_args(tiny, str(tmp_path / "model"), init_points=300), g)
    assert scene.format == "D-NeRF"
    assert len(scene.getTrainCameras()) == 6 and len(scene.getTestCameras()) == 2
    assert scene.getTrainCameras()[0].original_image.shape == (3, 32, 32) and g.pcd.points.shape == (300, 3)
    want = dataset.read_nerf_synthetic(tiny, False, True, init_points=300)
    assert [float(c.fid) for c in scene.getTrainCameras()] == [np.float32(c.fid) for c in want.train_cameras]


def test_script_parsers_take_nerfies_kind():
    from deformgs import render_cli, train
    assert train.build_parser().parse_args([]).nerfies_kind is None
    assert train.build_parser().parse_args(["--nerfies_kind", "vrig"]).nerfies_kind == "vrig"
    a = render_cli.build_parser().parse_args(["-m", "M"])
    assert (a.res, a.resolution, a.nerfies_kind) == (None, -1, None)
    b = render_cli.build_parser().parse_args(["-m", "M", "-r", "2", "--nerfies_kind", "interp", "--res", "8", "6"])
    assert (b.res, b.resolution, b.nerfies_kind) == ([8, 6], 2, "interp")
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--nerfies_kind", "colmap"])
