"""The rasterizer's run-time toggles (csrc/dgs_common.h Toggle, csrc/raster.hip): the default each takes from
its environment variable on the first read, and that an explicit set wins over the environment whether it
comes before or after that read. One fresh child process per case (the first read latches the default for
the life of a process); no GPU call is made, the library only has to load."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deformable-3d-gaussians_amd")
VARS = ("DGS_TILE_SORT", "DGS_DETERMINISTIC")
GETTERS = {"tile_sort": "dgs_debug_get_tile_sort", "det": "dgs_raster_get_deterministic"}

CASES = {
    # name: (environment, calls before the getters are printed, expected getter values)
    "unset": ({}, "", {"tile_sort": 1, "det": 0}),
    "tile_sort=0": ({"DGS_TILE_SORT": "0"}, "", {"tile_sort": 0}),
    "tile_sort=1": ({"DGS_TILE_SORT": "1"}, "", {"tile_sort": 1}),
    "det=1": ({"DGS_DETERMINISTIC": "1"}, "", {"det": 1}),
    "set_before_read": ({"DGS_TILE_SORT": "0"}, "lib.dgs_debug_set_tile_sort(1)", {"tile_sort": 1}),
    "set_after_read": ({"DGS_TILE_SORT": "0"}, "assert lib.dgs_debug_get_tile_sort() == 0; lib.dgs_debug_set_tile_sort(1)",
                       {"tile_sort": 1}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_toggle_semantics(name):
    setenv, pre, expected = CASES[name]
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env.update(setenv)
    code = (f"import sys; sys.path.insert(0, {PKG!r})\n"
            "from deformgs import _lib\n"
            "lib = _lib.load()\n"
            f"{pre}\n"
            f"print('TOGGLES', {', '.join(f'lib.{fn}()' for fn in GETTERS.values())})\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("TOGGLES")][-1]
    got = dict(zip(GETTERS, map(int, line[1:])))
    print(name, got)
    assert len(got) == len(GETTERS)
    for k, v in expected.items():
        assert got[k] == v, (name, got)
