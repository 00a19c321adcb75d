"""Writes tests/golden/nerfies_tiny/ and tests/golden/nerfies_tiny.npz (run by hand where a checkout of the
reference and PIL exist; the tests only read the results):

    python tests/golden/make_golden_nerfies.py --reference /path/to/Deformable-3D-Gaussians

nerfies_tiny/: a Nerfies-format directory (the layout of NeRF-DS and HyperNeRF) of 12 ids
  dataset.json    ids (12), train_ids (9), val_ids (3: every fourth id from the second)
  metadata.json   per id: camera_id (two cameras, alternating) and time_id = 3 + i, + 2 from the seventh id on
                  (the times do not start at 0 and have a gap, so time_id / max differs from any count-based rule)
  scene.json      scale 0.35, center (0.3, -0.2, 1.1), near / far
  camera/<id>.json  orientation (rows: right, down, forward in the world), position in the raw frame
                  (center + orbit position / scale: a radius-4 orbit around the origin of the scaled frame),
                  focal_length 40 at 44x28, principal point, skew, distortion; id 000003 carries the old
                  `tangential` key instead of `tangential_distortion`
  points.npy      500 float32 points: a Gaussian blob of sigma 0.4 around the origin of the scaled frame, stored
                  in the raw frame
  rgb/1x 44x28, rgb/2x 22x14, rgb/4x 11x7: RGB (colour type 2) PNGs of tests/png_fixtures.disc_image at the
                  id's time, per-row filter types cycling 0..4. 44x28 is ragged against the 16-pixel raster
                  tile and the 32-pixel SSIM tile on both axes, and not square.

nerfies_tiny.npz: for each split branch b in vrig, nerf, interp, other, from a copy of nerfies_tiny/ under a
parent directory named vrig-x, NeRF-x, interp-x, misc:
  <b>_R (n,3,3), <b>_T (n,3), <b>_FovX, <b>_FovY, <b>_fid (n) float64; <b>_width, <b>_height (n) int64;
  <b>_name (n) str; <b>_train_num; <b>_translate (3), <b>_radius: getNerfppNorm over the first train_num
  cameras (eval); <b>_translate_all, <b>_radius_all: over all of them (no eval)
These are a run of the reference's own readNerfiesCameras and getNerfppNorm (scene/dataset_readers.py:398-473,
77-98), not restated formulas. scene/dataset_readers.py is imported from the checkout under a `scene` package
whose __init__ is not executed (it pulls in the whole training stack), with empty stand-in modules for what
the file imports at module level and this path never calls: cv2, imageio, plyfile, and scene.gaussian_model
(only its BasicPointCloud tuple, taken from utils/graphics_utils.py, where the reference defines it too).
  resized_1x_22x14  float32 (12, 3, 14, 22), in the order of `ids`: the reference's own PILtoTorch
                  (utils/general_utils.py:23-29) on rgb/1x/<id>.png at (22, 14): the -r 2 path
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from png_fixtures import disc_image, encode_png_filtered  # noqa: E402

N_IDS = 12
SIZES = {"1x": (44, 28), "2x": (22, 14), "4x": (11, 7)}
SCALE, CENTER = 0.35, [0.3, -0.2, 1.1]
PARENTS = {"vrig": "vrig-x", "nerf": "NeRF-x", "interp": "interp-x", "other": "misc"}


def ids():
    return [f"{i:06d}" for i in range(N_IDS)]


def time_id(i):
    return 3 + i + (2 if i >= 6 else 0)


def orbit(azimuth, elevation, radius):
    """-> (orientation: rows right, down, forward; position), a camera looking at the origin."""
    pos = np.array([radius * np.cos(elevation) * np.sin(azimuth), -radius * np.cos(elevation) * np.cos(azimuth),
                    radius * np.sin(elevation)])
    fwd = -pos / np.linalg.norm(pos)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack([right, down, fwd]), pos


def write_nerfies_tiny(root):
    if os.path.isdir(root):
        shutil.rmtree(root)
    names = ids()
    for sub in ["camera"] + [os.path.join("rgb", k) for k in SIZES]:
        os.makedirs(os.path.join(root, sub))
    val = names[1::4]
    with open(os.path.join(root, "dataset.json"), "w") as f:
        json.dump({"count": N_IDS, "num_exemplars": 9, "ids": names, "train_ids": [n for n in names if n not in val],
                   "val_ids": val}, f, indent=1)
    with open(os.path.join(root, "metadata.json"), "w") as f:
        json.dump({n: {"warp_id": time_id(i), "appearance_id": time_id(i), "time_id": time_id(i), "camera_id": i % 2}
                   for i, n in enumerate(names)}, f, indent=1)
    with open(os.path.join(root, "scene.json"), "w") as f:
        json.dump({"scale": SCALE, "center": CENTER, "near": 0.05, "far": 2.5}, f, indent=1)
    for i, n in enumerate(names):
        # two rigs: camera 1 sits 0.25 rad further round and higher than camera 0
        az = 2 * np.pi * (i / 16.0) + 0.25 * (i % 2)
        el = 0.25 + 0.1 * np.sin(1.3 * i) + 0.15 * (i % 2)
        orientation, pos = orbit(az, el, 4.0)
        cam = {"orientation": orientation.tolist(), "position": (np.array(CENTER) + pos / SCALE).tolist(),
               "focal_length": 40.0, "principal_point": [22.0, 14.0], "skew": 0.0, "pixel_aspect_ratio": 1.0,
               "radial_distortion": [0.01, -0.002, 0.0], "image_size": [44, 28]}
        cam["tangential" if i == 3 else "tangential_distortion"] = [0.0005, -0.0003]
        with open(os.path.join(root, "camera", f"{n}.json"), "w") as f:
            json.dump(cam, f, indent=1)
        t = time_id(i) / time_id(N_IDS - 1)
        for k, (w, h) in SIZES.items():
            img = disc_image(w, h, t)[:, :, :3]
            with open(os.path.join(root, "rgb", k, f"{n}.png"), "wb") as f:
                f.write(encode_png_filtered(img, [(y + i) % 5 for y in range(h)], level=9))
    pts = np.random.default_rng(20241019).normal(0.0, 0.4, (500, 3))
    np.save(os.path.join(root, "points.npy"), (np.array(CENTER) + pts / SCALE).astype(np.float32))


def import_reference_reader(reference):
    """scene/dataset_readers.py of the checkout, without scene/__init__.py and the libraries it never calls on
    the Nerfies path (see the module docstring)."""
    sys.path.insert(0, reference)
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = None
    sys.modules.setdefault("plyfile", ply)
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(reference, "scene")]
    sys.modules["scene"] = pkg
    from utils.graphics_utils import BasicPointCloud
    gm = types.ModuleType("scene.gaussian_model")
    gm.BasicPointCloud = BasicPointCloud
    sys.modules["scene.gaussian_model"] = gm
    import scene.dataset_readers as readers
    return readers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of preacherwhite/Deformable-3D-Gaussians")
    args = ap.parse_args()
    root = os.path.join(HERE, "nerfies_tiny")
    write_nerfies_tiny(root)
    readers = import_reference_reader(os.path.abspath(args.reference))
    from PIL import Image
    from utils.general_utils import PILtoTorch  # the reference's own function
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for b, parent in PARENTS.items():
            copy = os.path.join(os.path.realpath(tmp), parent, "nerfies_tiny")
            shutil.copytree(root, copy)
            cams, train_num, _, _ = readers.readNerfiesCameras(copy)
            out[f"{b}_R"] = np.stack([c.R for c in cams])
            out[f"{b}_T"] = np.stack([c.T for c in cams])
            for key, field in (("FovX", "FovX"), ("FovY", "FovY"), ("fid", "fid")):
                out[f"{b}_{key}"] = np.array([getattr(c, field) for c in cams], np.float64)
            out[f"{b}_width"] = np.array([c.width for c in cams], np.int64)
            out[f"{b}_height"] = np.array([c.height for c in cams], np.int64)
            out[f"{b}_name"] = np.array([c.image_name for c in cams])
            out[f"{b}_train_num"] = np.int64(train_num)
            for suffix, part in (("", cams[:train_num]), ("_all", cams)):
                norm = readers.getNerfppNorm(part)
                out[f"{b}_translate{suffix}"] = np.asarray(norm["translate"])
                out[f"{b}_radius{suffix}"] = np.asarray(norm["radius"])
    out["resized_1x_22x14"] = np.stack([PILtoTorch(Image.open(os.path.join(root, "rgb", "1x", f"{n}.png")), (22, 14)).numpy()
                                        for n in ids()])
    np.savez_compressed(os.path.join(HERE, "nerfies_tiny.npz"), **out)
    print("wrote nerfies_tiny/ and", len(out), "arrays")


if __name__ == "__main__":
    main()
