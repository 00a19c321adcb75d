"""Host audit of the SSIM tile kernels' addressing (tools/ssim_index_audit.cpp): every thread of every
workgroup of k_ssim_fwd / k_ssim_final / k_ssim_bwd (csrc/ssim.hip) and of k_tile<false> / k_tile<true> /
k_pool (csrc/metrics.hip) replayed on the CPU with the kernels' index expressions (the shared ones are
csrc/ssim_tile.h's), each global and LDS address checked against its buffer's extent, for the shapes the GPU
loss tests use (tests/test_gpu_loss.py, among them the (3,61,83) run that preceded the r4v abort), ragged /
degenerate ones, and every pyramid level tests/test_gpu_image_metrics.py reaches. No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("audit") / "ssim_index_audit"
    subprocess.run(["g++", "-O2", "-Wall", "-o", str(path), os.path.join(ROOT, "tools", "ssim_index_audit.cpp")],
                   check=True)
    return str(path)


def test_ssim_addresses_in_bounds(exe):
    shapes = [(3, 61, 83), (1, 16, 16), (3, 5, 200), (3, 256, 256), (3, 400, 400), (1, 1, 1), (2, 33, 31),
              (3, 32, 32), (3, 31, 65)]
    args = [str(v) for s in shapes for v in s]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 out of bounds") == len(shapes), r.stdout


def test_loss_parity_shapes_in_bounds(exe):
    # tests/test_gpu_loss_parity.py (loss_ref.SHAPES as (C, H, W)): narrower than the window, tile edges +-1, the halo
    # on a tile edge, 1026 tile blocks for k_ssim_final's strided loop, C = 1 and 4
    import loss_ref
    shapes = [(c, h, w) for h, w, c in loss_ref.SHAPES]
    assert (3, 1, 10913) in shapes and (3, 37, 64) in shapes and (4, 33, 31) in shapes
    r = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 out of bounds") == len(shapes), r.stdout


def test_metrics_addresses_in_bounds(exe):
    # tests/test_gpu_image_metrics.py: CASES (F, H, W) with three channels -> F * 3 planes; the pyramids'
    # level sizes are fixed here, not taken from the program under test
    pyramids = {(161, 163): ["161x163", "81x82", "41x41", "21x21", "11x11"],
                (200, 176): ["200x176", "100x88", "50x44", "25x22", "13x11"]}
    runs = [(9, 161, 163), (9, 200, 176), (3, 161, 163)]
    args = []
    for p, h, w in runs:
        args += ["ms", p, h, w, "same", p, h, w]
    args += ["same", 6, 37, 45]
    r = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    # per pyramid: five tile passes and four pools; per zero-padded pass: one line
    assert len(lines) == 9 * len(runs) + len(runs) + 1, r.stdout
    assert all(ln.endswith(" 0 out of bounds") and " 0 addresses" not in ln for ln in lines), r.stdout
    for p, h, w in runs:
        sizes = pyramids[(h, w)]
        for l, size in enumerate(sizes):
            assert f"k_tile<true> level {l} {size} ({p} planes)" in r.stdout, r.stdout
        for a, b in zip(sizes, sizes[1:]):
            assert f"k_pool {a} -> {b} ({p} planes)" in r.stdout, r.stdout
        assert f"k_tile<false> {h}x{w} ({p} planes)" in r.stdout, r.stdout
    assert "k_tile<false> 37x45 (6 planes)" in r.stdout, r.stdout
