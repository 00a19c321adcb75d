"""What tests/golden/camera_sets.npz records (tests/golden/make_golden_camera_sets.py) and what
tests/test_camera_sets.py and tests/test_gpu_camera_sets.py take again: the render script's camera sets, the
training readers' point clouds and Scene's written files on the three tiny dataset directories. Every value is
an array under a flat "case/field" name; nothing here knows what the values should be."""
import json
import os
from argparse import Namespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DNERF, NERFIES, COLMAP = (os.path.join(GOLDEN, d) for d in ("dnerf_tiny", "nerfies_tiny", "colmap_tiny"))
DNERF_POINTS = 500  # the random cloud of a D-NeRF directory: 100 000 by default, which no fixture should carry
# (case, directory, the reader's own arguments): nerfies_tiny lies under golden/, so None takes the "other" branch
# (rgb/2x, no test set) and "vrig" the train / val one (rgb/4x)
DATASETS = (("nerfies_none", NERFIES, dict(nerfies_kind=None)), ("nerfies_vrig", NERFIES, dict(nerfies_kind="vrig")),
            ("colmap", COLMAP, dict(images=None)))
# (case, --res, -r)
SIZES = (("r-1", None, -1), ("r2", None, 2), ("res20x12", (20, 12), -1))


def _stack(values, dtype, shape=()):
    return np.asarray(list(values), dtype).reshape((-1,) + shape)


def record_cameras(out, key, cams):
    """Per Camera of one set: R, T, FoVx, FoVy, fid, uid, image_width, image_height, whether original_image is
    present, and the present ones' values in order."""
    out[f"{key}/R"] = _stack((c.R for c in cams), np.float64, (3, 3))
    out[f"{key}/T"] = _stack((c.T for c in cams), np.float64, (3,))
    for f in ("FoVx", "FoVy"):
        out[f"{key}/{f}"] = _stack((getattr(c, f) for c in cams), np.float64)
    out[f"{key}/fid"] = _stack((c.fid.cpu().numpy() for c in cams), np.float32, (1,))
    for f in ("uid", "image_width", "image_height"):
        out[f"{key}/{f}"] = _stack((getattr(c, f) for c in cams), np.int64)
    images = [getattr(c, "original_image", None) for c in cams]
    out[f"{key}/has_image"] = _stack((im is not None for im in images), np.bool_)
    for k, im in enumerate(images):
        if im is not None:
            assert str(im.device.type) == str(cams[k].data_device.type)
            out[f"{key}/image{k}"] = im.cpu().numpy()


def dataset_sets(render_cli, directory, res, resolution, device, kw):
    """The camera sets of a Nerfies or Colmap directory through the entry point load_scene uses for it. On the
    commit the fixture was made from that was read_nerfies_sets / read_colmap_sets."""
    if hasattr(render_cli, "read_dataset_sets"):
        from deformgs.dataset import render_format
        return render_cli.read_dataset_sets(directory, render_format(directory), res, resolution, device, **kw)
    if "images" in kw:
        return render_cli.read_colmap_sets(directory, res, resolution, device, **kw)
    return render_cli.read_nerfies_sets(directory, res, resolution, device, **kw)


def render_side(device):
    from deformgs import render_cli
    out = {}
    for ground, white in (("white", True), ("black", False)):
        sets = render_cli.read_transforms(DNERF, 16, 12, device, white_background=white)
        record_cameras(out, f"render/dnerf_{ground}/train", sets.train)
        record_cameras(out, f"render/dnerf_{ground}/test", sets.test)
    for case, directory, kw in DATASETS:
        for size, res, resolution in SIZES:
            sets = dataset_sets(render_cli, directory, res, resolution, device, kw)
            record_cameras(out, f"render/{case}_{size}/train", sets.train)
            record_cameras(out, f"render/{case}_{size}/test", sets.test)
    return out


def _record_cloud(out, key, pcd):
    for f in ("points", "colors", "normals"):
        out[f"{key}/{f}"] = np.asarray(getattr(pcd, f))


def training_side(tmp):
    """read_scene_info without a model_path and with one under `tmp` (a directory)."""
    from deformgs import dataset
    out = {}
    cases = (("dnerf", DNERF, dict(init_points=DNERF_POINTS)),) + tuple((c, d, kw) for c, d, kw in DATASETS)
    for case, directory, kw in cases:
        for where in ("memory", "model"):
            model = os.path.join(tmp, f"{case}_model") if where == "model" else None
            info = dataset.read_scene_info(directory, False, True, model_path=model, **kw)
            key = f"train/{case}_{where}"
            _record_cloud(out, key, info.point_cloud)
            if info.ply_path is None:
                place = "none"
            elif model and info.ply_path == os.path.join(model, "input.ply"):
                place = "MODEL/input.ply"
            else:
                place = "SOURCE/" + os.path.relpath(info.ply_path, directory)
            out[f"{key}/ply_path"] = np.array(place)
            out[f"{key}/names"] = np.array([c.image_name for c in info.train_cameras] + ["|"] +
                                           [c.image_name for c in info.test_cameras])
            out[f"{key}/translate"] = np.asarray(info.nerf_normalization["translate"])
            out[f"{key}/radius"] = np.asarray(info.nerf_normalization["radius"])
            if model:
                with open(os.path.join(model, "input.ply"), "rb") as f:
                    out[f"{key}/input_ply"] = np.frombuffer(f.read(), np.uint8)
    return out


class _Gaussians:
    """The stand-in model: keeps what Scene hands to create_from_pcd."""

    def create_from_pcd(self, pcd, spatial_lr_scale, device="cuda"):
        self.pcd, self.extent, self.device = pcd, spatial_lr_scale, str(device)


def scene_side(tmp):
    """Scene on dnerf_tiny with data_device cpu and the stand-in model."""
    from deformgs.dataset import Scene
    model = os.path.join(tmp, "scene_model")
    g = _Gaussians()
    scene = Scene(Namespace(source_path=DNERF, model_path=model, white_background=True, eval=True, resolution=-1,
                            init_points=DNERF_POINTS, data_device="cpu"), g)
    out = {}
    with open(os.path.join(model, "cameras.json")) as f:
        out["scene/cameras_json"] = np.array(json.dumps(json.load(f), sort_keys=True))
    with open(os.path.join(model, "input.ply"), "rb") as f:
        out["scene/input_ply"] = np.frombuffer(f.read(), np.uint8)
    out["scene/written"] = np.array(sorted(os.listdir(model)))
    out["scene/cameras_extent"] = np.asarray(scene.cameras_extent)
    out["scene/create_extent"] = np.asarray(g.extent)
    _record_cloud(out, "scene/cloud", g.pcd)
    record_cameras(out, "scene/train", scene.getTrainCameras())
    record_cameras(out, "scene/test", scene.getTestCameras())
    return out


def compare(got, gold, keys=None):
    """Exact: the same names, dtypes, shapes and values."""
    keys = sorted(got) if keys is None else keys
    assert keys, "nothing to compare"
    for k in keys:
        assert k in gold, f"{k}: not in the fixture"
        a, b = got[k], gold[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), k
