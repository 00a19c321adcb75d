"""Writes tests/golden/camera_sets.npz: what the render script's camera sets, the training readers' point clouds
and Scene's written files were on commit f15a06a, before deformgs/dataset.py, ingest.py and render_cli.py were
reduced to one statement of each shared step. Run once, on the CPU, with that commit's code:

    python tests/golden/make_golden_camera_sets.py

The cases and the recorded fields are stated in tests/camera_sets_cases.py, which tests/test_camera_sets.py
runs again; the fixture is data only (arrays under "case/field" names), all on device "cpu":

  render/dnerf_{white,black}/{train,test}/...   render_cli.read_transforms on dnerf_tiny at 16 x 12
  render/{nerfies_none,nerfies_vrig,colmap}_{r-1,r2,res20x12}/{train,test}/...
                                                the render script's sets of nerfies_tiny (nerfies_kind None and
                                                "vrig") and colmap_tiny: -r -1, -r 2, --res 20 12
      per set: R, T, FoVx, FoVy (float64), fid (float32), uid, image_width, image_height, has_image, image<k>
  train/{dnerf,nerfies_none,nerfies_vrig,colmap}_{memory,model}/...
                                                read_scene_info with eval, without a model_path and with one:
      points, colors, normals (their dtypes are part of the record), ply_path ("none", "SOURCE/<file>" or
      "MODEL/input.ply"), the split's names, translate, radius, and input_ply: the written file's bytes
  scene/...                                     Scene on dnerf_tiny with a stand-in Gaussian model: cameras.json
                                                (parsed, then dumped with sorted keys), input.ply, the names of
                                                the written files, cameras_extent, the cloud handed to
                                                create_from_pcd, both camera lists
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "deformable-3d-gaussians_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import camera_sets_cases as cases  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = {**cases.render_side("cpu"), **cases.training_side(tmp), **cases.scene_side(tmp)}
    path = os.path.join(HERE, "camera_sets.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
