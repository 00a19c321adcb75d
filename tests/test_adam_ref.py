"""CPU: the bars of tests/adam_ref.py are reachable by fp32 arithmetic of the kernel's form, and tight enough that
each listed mis-statement of the Adam update breaks one on at least one of the states the GPU test runs
(tests/test_gpu_adam_parity.py). The GPU test compares with step64 only; step32 is the stand-in for a kernel here."""
import numpy as np
import pytest

import adam_ref as ref


def ratios(state, wrong=None):
    """Worst |step32 - step64| / bar over the tensors of a state -> {"p", "m", "v"}."""
    c = ref.cases()[state]
    out = {"p": 0.0, "m": 0.0, "v": 0.0}
    tensors = c["tensors"]
    for k, ten in enumerate(tensors):
        nb = tensors[(k + 1) % len(tensors)]
        ss_other = ref.scalars(nb["lr"], c["b1"], c["b2"], nb["t"])[0]
        got = ref.step32(ten["p"], ten["g"], ten["m"], ten["v"], ten["lr"], c["b1"], c["b2"], c["eps"], ten["t"],
                         wrong=wrong, ss_other=ss_other)
        for key, r in ref.compare(got, ten, c["b1"], c["b2"], c["eps"]).items():
            out[key] = max(out[key], r)
    return out


def test_cases_are_what_the_gpu_test_needs():
    cs = ref.cases()
    assert tuple(cs) == ref.STATES
    for name, c in cs.items():
        assert tuple(t["numel"] for t in c["tensors"]) == ref.NUMELS == (1, 3, 2047, 2048, 2049, 4101, 70001)
        for t in c["tensors"]:
            for a in "pgmv":
                assert t[a].dtype == np.float32 and t[a].shape == (t["numel"],) and np.isfinite(t[a]).all()
            assert (t["v"] >= 0).all()
        steps = {ref.scalars(t["lr"], c["b1"], c["b2"], t["t"])[0] for t in c["tensors"]}
        assert len(steps) == (1 if name == "lr_zero" else len(ref.NUMELS)), "every tensor has its own step_size"
        assert c["eps"] == (1e-8 if name == "eps_1e-8" else 1e-15)
    near = np.abs(np.concatenate([t["g"] for t in cs["near_eps"]["tensors"]]))
    assert near.min() < 1e-16 and near.max() > 1e-14 and near.max() <= 1.01e-13
    big = np.abs(np.concatenate([t["g"] for t in cs["large_gradient"]["tensors"]]))
    assert 100.0 < big.max() <= 1000.0
    t = cs["cancelling"]["tensors"][-1]
    assert (t["g"] == t["m"]).any() and (np.abs(t["g"] - t["m"]) <= 1e-5 * np.abs(t["m"])).all()
    assert (t["m"] > 0).any() and (t["m"] < 0).any()
    assert all(t["t"] == 40000 for t in cs["late_step"]["tensors"])
    assert all((t["g"] == 0).all() for t in cs["zero_gradient"]["tensors"])


def test_scalars_are_the_tables_fp32():
    import ctypes
    for lr, t in ((1.6e-4, 1), (8e-4, 7), (1.6e-6, 40000)):
        ss, bc = ref.scalars(lr, 0.9, 0.999, t)
        assert ss.dtype == bc.dtype == np.float32
        # a ctypes float field (deformgs/_lib.py AdamTensor) rounds the same double the same way
        assert ctypes.c_float(lr / (1.0 - 0.9 ** t)).value == float(ss)
        assert ctypes.c_float((1.0 - 0.999 ** t) ** 0.5).value == float(bc)


@pytest.mark.parametrize("state", ref.STATES)
def test_fp32_arithmetic_meets_the_bars(state):
    r = ratios(state)
    print(state, r)
    assert max(r.values()) <= 1.0, r


def test_lr_zero_leaves_p_bitwise():
    c = ref.cases()["lr_zero"]
    for ten in c["tensors"]:
        p1, m1, v1 = ref.step32(ten["p"], ten["g"], ten["m"], ten["v"], 0.0, c["b1"], c["b2"], c["eps"], ten["t"])
        assert np.array_equal(p1.view(np.int32), ten["p"].view(np.int32))
        assert (m1 != ten["m"]).any() and (v1 != ten["v"]).any()


@pytest.mark.parametrize("wrong", ref.MUTANTS)
def test_a_wrong_update_breaks_a_bar(wrong):
    broken = {}
    for state in ref.STATES:
        r = ratios(state, wrong)
        if max(r.values()) > 1.0:
            broken[state] = {k: round(v, 1) for k, v in r.items() if v > 1.0}
    print(wrong, broken)
    assert broken, wrong
    # the states the listed errors need: eps against sqrt(v) only shows where the two are comparable
    if wrong in ("eps_before_division", "eps_inside_sqrt"):
        assert "near_eps" in broken


def test_accumulated_bars_hold_over_steps():
    """accumulate() bounds fp32 moments against float64 ones over 30 steps of the same gradients."""
    rng = np.random.default_rng(5)
    n, b1, b2 = 4096, 0.9, 0.999
    f = np.float32
    m32, v32 = np.zeros(n, f), np.zeros(n, f)
    m64, v64 = np.zeros(n), np.zeros(n)
    am, av = np.zeros(n), np.zeros(n)
    p = np.zeros(n, f)
    for t in range(1, 31):
        g = (1e-4 * rng.standard_normal(n)).astype(f)
        am, av = ref.accumulate(am, av, g, m64, v64, b1, b2)
        if t == 30:  # they stay a rounding bound: 1e-4 relative on the last step's gradient is outside them
            _, mw, vw = ref.step32(p, g * f(1.0001), m32, v32, 1e-3, b1, b2, 1e-15, t)
        _, m32, v32 = ref.step32(p, g, m32, v32, 1e-3, b1, b2, 1e-15, t)
        _, m64, v64 = ref.step64(p, g, m64, v64, 1e-3, b1, b2, 1e-15, t)
        assert ref.worst(m32, m64, am) <= 1.0 and ref.worst(v32, v64, av) <= 1.0, t
    assert (np.abs(mw - m64) > am).mean() > 0.5
