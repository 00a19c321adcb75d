"""bench.py's output line keeps the driver's contract (task README / DESIGN.md §5): one JSON line on
stdout with the required keys, a whole-job value consistent with ms_per_step, and the roofline
object of the dominant kernel (frac = achieved / peak). A short run (one child process, small
scene, no CPU leg) — the numbers are not checked, the shape is."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

REQUIRED = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int,
            "ms_per_step": float, "higher_is_better": bool, "scaling": str, "dtype": str, "data": str,
            "config": dict, "roofline": dict}


def _plain_run(dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "8", "--warmup", "2", "--n", "20000",
           "--res", "256", "--no-cpu-baseline", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    return out, {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One plain run with --dump-outputs, shared by the tests below: (process result, {name: array})."""
    return _plain_run(tmp_path_factory.mktemp("bench") / "out")


def test_bench_line_contract(plain_run):
    out, arrs = plain_run
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k, t in REQUIRED.items():
        assert k in d, k
        assert isinstance(d[k], t) or (t is float and isinstance(d[k], int)), (k, type(d[k]))
    assert d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert "vs_baseline" in d
    # whole-job throughput: iterations per second of the timed steps
    assert d["value"] == pytest.approx(1000.0 / d["ms_per_step"], rel=1e-6)
    assert "workload" in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-6)
    assert 0.0 < r["frac"] < 1.0
    # a plain run has no CPU leg (--full); --dump-outputs wrote the last timed step's results
    assert d["cpu_baseline"] is None
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["render"].shape == (3, 256, 256) and arrs["loss"].shape == (1,)
    assert arrs["radii"].shape == (20000,) and arrs["grad_xyz"].shape == (20000, 3)
    assert np.abs(arrs["grad_xyz"]).max() > 0 and np.abs(arrs["grad_deform_linear.0.weight"]).max() > 0


def test_dumped_outputs_repeat_between_runs(plain_run, tmp_path):
    """A second process with the same arguments writes the same arrays up to the rounding of one step's
    float atomics (the dumped step starts from the run's starting parameters, bench.py). Bound: a sum of n
    float32 terms added in another order moves by at most (n - 1) u sum|t|, u = 6e-8; with the ~100
    contributions a gradient element of this scene collects, each at most the array's largest magnitude,
    that is 1e-5 of the largest magnitude. Arrays without atomics (image, depth, radii) meet it trivially."""
    _, a = plain_run
    _, b = _plain_run(tmp_path / "out")
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape
        worst, scale = float(np.abs(a[k].astype(np.float64) - b[k]).max()), float(np.abs(a[k]).max())
        print(f"{k}: max diff {worst:.3e}, largest magnitude {scale:.3e}")
        assert worst <= 1e-5 * scale, (k, worst, scale)


def test_bench_full_adds_the_cpu_baseline():
    """--full: the same line with the CPU leg measured (one CPU step here), after the timed GPU steps."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--n", "20000",
           "--res", "256", "--full", "--cpu-warmup", "0", "--cpu-steps", "1"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["value"] == pytest.approx(1000.0 / d["ms_per_step"], rel=1e-6)
    c = d["cpu_baseline"]
    assert "error" not in c, c
    assert c["unit"] == "iters/s" and c["value"] > 0 and c["value"] == pytest.approx(1.0 / c["median_s"], rel=1e-6)


def test_bench_self_launches_two_ranks_gloo_rehearsal():
    """`bench.py --gpus 2` invoked directly (no WORLD_SIZE) launches its own two ranks through
    torch.distributed.run; on a one-GPU box both ranks share cuda:0 over gloo (DGS_DEVICE=0,
    DGS_DIST_BACKEND=gloo: RCCL refuses two ranks on one GPU). Rank 0's single line reports n_gpus 2, the
    backend and what every rank saw."""
    env = dict(os.environ, DGS_DEVICE="0", DGS_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
           "--n", "20000", "--res", "256", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 2
    assert d["dist"]["world_size"] == 2 and d["dist"]["backend"] == "gloo"
    assert sorted(r["rank"] for r in d["dist"]["ranks"]) == [0, 1]
    assert all(r["world_seen"] == 2 for r in d["dist"]["ranks"])
    assert d["value"] == pytest.approx(2 * 1000.0 / d["ms_per_step"], rel=1e-6)
