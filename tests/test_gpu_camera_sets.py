"""GPU: the render-side cases of tests/golden/camera_sets.npz again with device "cuda". The fixture was recorded on
the CPU; the device ingest is bit-exact to the numpy path by design, so every original_image must equal it
bitwise, and the camera fields are host arithmetic. The shapes are the golden directories' own: 32 x 32 RGBA PNGs
to 16 x 12 (composite on white and on black, both resample passes), 44 x 28 JPEGs and 22 x 14 / 11 x 7 RGB PNGs at
their own size, halved by -r 2 and forced to 20 x 12."""
import os

import numpy as np
import pytest

import camera_sets_cases as cases
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


def test_render_side_on_the_device(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "camera_sets.npz")))
    got = cases.render_side("cuda")  # record_cameras asserts that every image lies on the cameras' device
    assert sorted(got) == sorted(k for k in gold if k.startswith("render/"))
    cases.compare(got, gold)
