"""CPU: the Colmap reader on tests/golden/colmap_tiny (and its text twin colmap_tiny_txt) against
tests/golden/colmap_tiny.npz, a run of the reference's own readColmapSceneInfo / getNerfppNorm / PILtoTorch
(tests/golden/make_golden_colmap.py). The float64 camera fields are the reference's expressions in its order:
they are compared bitwise. Ten 44x28 JPEGs named 0..7, 10, 11: as strings they sort 0, 1, 10, 11, 2, ..."""
import json
import os
import shutil
import struct

import numpy as np
import pytest

from deformgs import dataset
from png_fixtures import disc_image, encode_png_filtered

SORTED = ["0", "1", "10", "11", "2", "3", "4", "5", "6", "7"]
FILE_ORDER = ["5", "0", "11", "3", "7", "1", "10", "2", "6", "4"]
TEST = ["0", "6"]  # every 8th of SORTED
TRAIN = [n for n in SORTED if n not in TEST]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "colmap_tiny.npz")))


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return os.path.join(golden_dir, "colmap_tiny")


@pytest.fixture(scope="module")
def tiny_txt(golden_dir, tmp_path_factory):
    """The text model with the images of the binary one copied next to it."""
    out = str(tmp_path_factory.mktemp("colmap") / "txt")
    shutil.copytree(os.path.join(golden_dir, "colmap_tiny_txt"), out)
    shutil.copytree(os.path.join(golden_dir, "colmap_tiny", "images"), os.path.join(out, "images"))
    return out


def _tree(root):
    out = []
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), "rb") as fh:
                out.append((os.path.relpath(os.path.join(d, f), root), fh.read()))
    return sorted(out)


def _same(cams, gold, key):
    assert [c.image_name for c in cams] == gold[f"{key}_name"].tolist()
    for f in ("width", "height", "uid"):
        assert [getattr(c, f) for c in cams] == gold[f"{key}_{f}"].tolist()
    for f in ("R", "T", "FovX", "FovY", "fid"):
        got = np.stack([np.asarray(getattr(c, f), np.float64) for c in cams])
        want = gold[f"{key}_{f}"]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (key, f)


@pytest.mark.parametrize("which", ["bin", "txt"])
def test_reader_reproduces_the_reference(tiny, tiny_txt, gold, which):
    src = tiny if which == "bin" else tiny_txt
    assert dataset.dataset_format(src) == "Colmap"
    on, off = dataset.read_colmap(src, True), dataset.read_colmap(src, False)
    _same(on.train_cameras, gold, "eval_train")
    _same(on.test_cameras, gold, "eval_test")
    _same(off.train_cameras, gold, "all")
    assert off.test_cameras == []
    assert [c.image_name for c in off.train_cameras] == SORTED
    assert [c.image_name for c in on.test_cameras] == TEST and [c.image_name for c in on.train_cameras] == TRAIN
    for info, suffix in ((on, ""), (off, "_all")):
        assert np.asarray(info.nerf_normalization["translate"]).tobytes() == gold[f"translate{suffix}"].tobytes()
        assert np.asarray(info.nerf_normalization["radius"]).tobytes() == gold[f"radius{suffix}"].tobytes()
        pts, col = np.asarray(info.point_cloud.points), np.asarray(info.point_cloud.colors)
        assert pts.dtype == np.float32 and pts.shape == (300, 3) and pts.tobytes() == gold["points"].tobytes()
        assert col.dtype == np.float64 and col.tobytes() == gold["colors"].tobytes()
        assert info.ply_path is None  # no MODEL: nothing written
    assert 4.0 < float(gold["radius"]) < 5.0  # the fixture's radius-4 orbit, x 1.1
    assert all(c.image_path == os.path.join(src, "images", c.image_name + ".jpg") for c in off.train_cameras)


def test_bin_and_txt_models_agree(tiny, tiny_txt):
    a, b = dataset.read_colmap_cameras(tiny), dataset.read_colmap_cameras(tiny_txt)
    assert [c.image_name for c in a] == FILE_ORDER == [c.image_name for c in b]  # the order of the images file
    for x, y in zip(a, b):
        assert x.R.tobytes() == y.R.tobytes() and x.T.tobytes() == y.T.tobytes()
        assert (x.FovX, x.FovY, x.fid, x.uid, x.width, x.height) == (y.FovX, y.FovY, y.fid, y.uid, y.width, y.height)
    pa = dataset.read_colmap_points(os.path.join(tiny, "sparse", "0", "points3D.bin"))
    pb = dataset.read_colmap_points(os.path.join(tiny_txt, "sparse", "0", "points3D.txt"))
    assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes() and pa[0].shape == (300, 3)


def test_camera_fields_follow_the_written_formulas(tiny):
    cams = {c.image_name: c for c in dataset.read_colmap_cameras(tiny)}
    assert {c.uid for c in cams.values()} == {1, 2}
    for name, c in cams.items():
        assert c.fid == int(name) / 9 and (c.width, c.height) == (44, 28) == dataset.image_size(c.image_path)
        if c.uid == 1:  # PINHOLE: fx 40, fy 38.5
            assert (c.FovX, c.FovY) == (dataset.focal2fov(40.0, 44), dataset.focal2fov(38.5, 28))
        else:  # SIMPLE_PINHOLE: f 41.25
            assert (c.FovX, c.FovY) == (dataset.focal2fov(41.25, 44), dataset.focal2fov(41.25, 28))
        assert np.allclose(c.R @ c.R.T, np.eye(3), atol=1e-12)
        # the camera looks at the origin from 4 away: the origin maps to (0, 0, 4) in view space
        assert np.allclose(c.R.T @ np.zeros(3) + c.T, [0, 0, 4.0], atol=1e-9)
    assert max(c.fid for c in cams.values()) == 11 / 9  # the names, not the count, give the time


def test_images_flag_selects_the_directory(tiny, golden_dir, tmp_path):
    src = str(tmp_path / "src")
    shutil.copytree(os.path.join(golden_dir, "colmap_tiny_txt"), src)
    shutil.copytree(os.path.join(tiny, "images"), os.path.join(src, "images_2"))
    with pytest.raises(FileNotFoundError):
        dataset.read_colmap(src, True)
    info = dataset.read_colmap(src, True, images="images_2")
    assert info.train_cameras[0].image_path == os.path.join(src, "images_2", "1.jpg")
    from deformgs import render_cli, train
    assert train.build_parser().parse_args([]).images == "images"
    assert train.build_parser().parse_args(["-i", "images_2"]).images == "images_2"
    assert render_cli.build_parser().parse_args(["-m", "M", "--images", "x"]).images == "x"
    from deformgs.arguments import ModelParams
    assert ModelParams().images == "images"


class _Gaussians:
    def create_from_pcd(self, pcd, extent, device=None):
        self.pcd, self.extent = pcd, extent


def _args(src, model, **kw):
    from deformgs.arguments import ModelParams
    return ModelParams(source_path=src, model_path=model, eval=True, data_device="cpu", **kw)


def test_scene_on_a_colmap_directory(tiny, gold, golden_dir, tmp_path):
    src = str(tmp_path / "src")
    shutil.copytree(tiny, src)
    before = _tree(src)
    model = str(tmp_path / "model")
    g = _Gaussians()
    scene = dataset.Scene(_args(src, model, white_background=True, init_points=7), g)
    assert scene.format == "Colmap"
    train, test = scene.getTrainCameras(), scene.getTestCameras()
    assert [c.image_name for c in train] == TRAIN and [c.image_name for c in test] == TEST
    jg = np.load(os.path.join(golden_dir, "jpeg_ingest.npz"))
    assert train[0].original_image._base.shape == (8, 3, 28, 44)  # one ingest batch per set, 4:4:4 and 4:2:0 mixed
    from deformgs.jpeg import read_jpeg
    for cam in train + test:
        px = read_jpeg(os.path.join(src, "images", cam.image_name + ".jpg"))
        assert (cam.image_width, cam.image_height) == (44, 28)
        assert np.array_equal(cam.original_image.numpy(), px.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    k = list(gold["all_name"]).index(train[3].image_name)
    assert float(train[3].fid) == np.float32(gold["all_fid"][k]) and train[3].FoVx == gold["all_FovX"][k]
    assert scene.cameras_extent == float(gold["radius"])
    assert g.pcd.points.tobytes() == gold["points"].tobytes() and g.pcd.colors.tobytes() == gold["colors"].tobytes()
    with open(os.path.join(model, "cameras.json")) as f:
        cj = json.load(f)
    assert [c["img_name"] for c in cj] == TEST + TRAIN and {(c["width"], c["height"]) for c in cj} == {(44, 28)}
    assert sorted(os.listdir(model)) == ["cameras.json", "cfg_args", "input.ply"]
    with open(os.path.join(model, "cfg_args")) as f:
        assert "images='images'" in f.read()
    assert _tree(src) == before  # SOURCE is byte-identical: no sparse/0/points3D.ply is written
    assert jg["libjpeg_turbo_version"].shape == ()


def test_scene_resolution_2_matches_the_reference_resize(tiny, gold, tmp_path):
    scene = dataset.Scene(_args(tiny, str(tmp_path / "model"), resolution=2), _Gaussians())
    cams = scene.getTrainCameras() + scene.getTestCameras()
    assert len(cams) == 10
    for cam in cams:
        assert (cam.image_width, cam.image_height) == (22, 14)
        assert np.array_equal(cam.original_image.numpy(), gold["half_22x14"][SORTED.index(cam.image_name)])


def test_points3d_ply_in_source_is_used(tiny, tmp_path):
    src = str(tmp_path / "src")
    shutil.copytree(tiny, src)
    xyz = np.random.default_rng(1).uniform(-1, 1, (9, 3))
    dataset.store_ply(os.path.join(src, "sparse", "0", "points3D.ply"), xyz, np.full((9, 3), 200.7))
    own = dataset.read_colmap(src, True, model_path=str(tmp_path / "m"))
    assert np.array_equal(own.point_cloud.points, xyz.astype(np.float32))
    assert own.ply_path == os.path.join(src, "sparse", "0", "points3D.ply") and not os.path.exists(str(tmp_path / "m"))
    for name in ("points3D.ply", "points3D.bin"):
        os.remove(os.path.join(src, "sparse", "0", name))
    with pytest.raises(ValueError, match="points3D"):
        dataset.read_colmap(src, True)


def _rewrite_cameras(src, model_id, n_params):
    with open(os.path.join(src, "sparse", "0", "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", 2))
        for cid in (1, 2):
            f.write(struct.pack("<iiQQ", cid, model_id, 44, 28) + struct.pack(f"<{n_params}d", *([40.0] * n_params)))


def test_refusals(tiny, tmp_path):
    src = str(tmp_path / "src")
    shutil.copytree(tiny, src)
    _rewrite_cameras(src, 4, 8)  # OPENCV: a distorted model, with the reference's wording
    with pytest.raises(ValueError, match="OPENCV.*only undistorted datasets .PINHOLE or SIMPLE_PINHOLE cameras. supported"):
        dataset.read_colmap(src, True)
    _rewrite_cameras(src, 42, 3)
    with pytest.raises(ValueError, match="unknown Colmap camera model id 42"):
        dataset.read_colmap(src, True)
    # a non-integer image name (text model: easy to edit)
    txt = str(tmp_path / "txt")
    shutil.copytree(os.path.join(os.path.dirname(tiny), "colmap_tiny_txt"), txt)
    shutil.copytree(os.path.join(tiny, "images"), os.path.join(txt, "images"))
    p = os.path.join(txt, "sparse", "0", "images.txt")
    with open(p) as f:
        lines = f.read()
    with open(p, "w") as f:
        f.write(lines.replace(" 7.jpg", " frame_7.jpg"))
    os.rename(os.path.join(txt, "images", "7.jpg"), os.path.join(txt, "images", "frame_7.jpg"))
    with pytest.raises(ValueError, match="frame_7.*frame number"):
        dataset.read_colmap(txt, True)
    # a single-image model
    with open(p, "w") as f:
        f.write("\n".join(lines.splitlines()[:3] + lines.splitlines()[3:5]) + "\n")
    with pytest.raises(ValueError, match="1 image"):
        dataset.read_colmap(txt, True)
    # an RGBA PNG where an image should be
    rgba = str(tmp_path / "rgba")
    shutil.copytree(tiny, rgba)
    with open(os.path.join(rgba, "images", "3.jpg"), "wb") as f:
        f.write(encode_png_filtered(disc_image(44, 28, 0.2), [0] * 28))
    with pytest.raises(ValueError, match="alpha.*unsupported"):
        dataset.read_colmap(rgba, True)
    # a truncated binary model
    cut = str(tmp_path / "cut")
    shutil.copytree(tiny, cut)
    with open(os.path.join(cut, "sparse", "0", "images.bin"), "r+b") as f:
        f.truncate(200)
    with pytest.raises(ValueError, match="truncated"):
        dataset.read_colmap(cut, True)


def test_sparse_without_a_model_is_refused_before_model_is_created(tmp_path):
    src = tmp_path / "src"
    os.makedirs(src / "sparse" / "0")
    (src / "sparse" / "0" / "images.bin").write_bytes(b"")  # no cameras file: not a pair
    with pytest.raises(ValueError, match="Colmap.*unsupported"):
        dataset.Scene(_args(str(src), str(tmp_path / "model")), _Gaussians())
    assert not os.path.exists(tmp_path / "model")


def test_an_rgb_png_is_a_valid_colmap_image(tiny, tmp_path):
    src = str(tmp_path / "src")
    shutil.copytree(tiny, src)
    rgb = np.ascontiguousarray(disc_image(44, 28, 0.2)[:, :, :3])
    with open(os.path.join(src, "images", "3.jpg"), "wb") as f:  # the signature decides
        f.write(encode_png_filtered(rgb, [1] * 28))
    scene = dataset.Scene(_args(src, str(tmp_path / "model")), _Gaussians())
    cam = [c for c in scene.getTrainCameras() if c.image_name == "3"][0]
    assert np.array_equal(cam.original_image.numpy(), rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
