#!/usr/bin/env python3
"""Writes tests/golden/png_encode_streams.npz: the zlib streams the device PNG encoder of a parent revision writes
for PIN_CASES of tests/test_gpu_png_encode.py, which test_streams_equal_the_recorded_ones holds the current encoder
to. Needs a GPU. The library is never the current tree's: build the parent's with
  SRC="png_encode jpeg_encode jpeg" REV=<parent> tools/ab_build.sh        (-> lib/diag/libdgs_base.so)
and run
  DGS_LIB=<that library> tests/golden/make_golden_png_encode.py <parent> [out.npz]
Per case `<name>_packed` (uint8), `<name>_offsets`, `<name>_lengths` (int64) of png_gpu.encode_streams on the one
frame; `cases`; `parent`, the revision given."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "deformable-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    lib = os.environ.get("DGS_LIB", "")
    assert lib and os.path.isfile(lib), "DGS_LIB must point at the parent revision's library (tools/ab_build.sh)"
    parent = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "png_encode_streams.npz")
    from test_gpu_png_encode import PIN_CASES, pin_streams
    out = {"cases": np.array(sorted(PIN_CASES)), "parent": np.array(parent)}
    for name, img in PIN_CASES.items():
        out[f"{name}_packed"], out[f"{name}_offsets"], out[f"{name}_lengths"] = pin_streams(img[None])
    np.savez_compressed(path, **out)
    print(f"{path}: {len(PIN_CASES)} cases from {parent} ({lib}), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
