"""Float64 reference, error bars and single-step states for the multi-tensor Adam (csrc/adam.hip, k_adam).

The update (header of csrc/adam.hip; torch.optim.Adam with amsgrad and weight decay off):

    m' = m + (1 - b1) (g - m)
    v' = b2 v + (1 - b2) g g
    p' = p - step_size * m' / (sqrt(v') / bc2_sqrt + eps)

step_size = lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) are computed in double on the host and rounded to fp32 for
the kernel's table (deformgs/_lib.py AdamTensor); `scalars` does the same, so `step64` sees the two numbers the kernel
sees. Everything else in `step64` is exact double arithmetic on the fp32 inputs: 1 - b1, b2, 1 - b2 and eps are the
doubles themselves, while the kernel rounds each of them to fp32 once (Jobs::omb1, b2, omb2, eps).

`step32` restates the kernel's expression order in numpy fp32, one rounding per operation and no FMA. It exists to
show on the CPU that fp32 arithmetic of this form meets the bars (tests/test_adam_ref.py) and to carry the deliberate
mis-statements of the update; no GPU test compares with it.

Bars (`bars`), per element, u = 2^-24 (the unit roundoff of fp32: one rounded operation or one rounded constant
changes its result by at most u relative). Derivation, first order in u; an FMA only removes roundings:

  m'  d = g - m rounds once, and |d| <= |g| + |m| <= 2 A with A = max(|m|, |g|). The fp32 constant c1 = 1 - b1 and
      the product c1 d each add u |c1 d|, so c1 d carries 3u c1 |d| <= 6u c1 A. The final sum rounds by u |m'|, and
      m' lies between m and g (0 < c1 < 1), so |m'| <= A. Together (6 c1 + 1) u A <= 4u A for c1 <= 0.5, which
      torch's lerp branch already assumes.
          bar_m = 4u max(|m|, |g|)
      It is relative to the operands, not to m': g - m may cancel, and then m' itself is far smaller than A.
  v'  b2 (fp32) and the product each add u b2 v; g g, c2 = 1 - b2 (fp32) and their product add 3u c2 g^2; the sum
      rounds by u v'. All terms are non-negative, so v' <= max(v, g^2) and the total is at most
      (2 b2 + 3 c2 + 1) u max(v, g^2) = (3 + c2) u max(v, g^2).
          bar_v = 4u max(v, g^2)
      The same count bounds the error relative to v' itself by 4u (no cancellation), which the next line uses.
  p'  sqrt halves the 4u of v' and rounds once (3u), the division by bc2_sqrt rounds once (4u), eps as an fp32
      constant and the sum add at most 2u: denom is within 6u. q = m' / denom inherits bar_m / denom from m', 6u |q|
      from denom and u |q| from the division; the product with step_size adds u |q| (none when fused). That is 8u;
      the bar allows 16u, which covers a division or square root of 2.5 ulp instead of a correctly rounded one. The
      final sum rounds to the nearest fp32, half an ulp of a value no larger than |p'| + E:
          E     = step_size (bar_m / denom + 16u |m'| / denom)
          bar_p = 0.5 ulp(|p'| + E) + E
      With lr = 0 the bar is half an ulp of p and p' = p exactly; the test asks for bitwise equality there.

Each bar has a floor of one fp32 denormal step (2^-149): a result that underflows is rounded on that grid, not
relative to itself.

`accumulate` carries the bars of m and v through several steps (the moments are never reset by a step):
A_m' = b1 A_m + 4u max(|m| + A_m, |g|), likewise for v. The parameter is not accumulated this way: a many-step test
compares its error with that of an fp32 torch.optim.Adam on the same run.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
NUMELS = (1, 3, 2047, 2048, 2049, 4101, 70001)
B1, B2, EPS = 0.9, 0.999, 1e-15


def scalars(lr, b1, b2, t):
    """(step_size, bc2_sqrt) as the kernel's table holds them: computed in double, rounded to fp32."""
    return np.float32(lr / (1.0 - b1 ** t)), np.float32(math.sqrt(1.0 - b2 ** t))


def ulp32(x):
    """Spacing of fp32 at the double value(s) x."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.maximum(np.ldexp(1.0, e - 24), TINY)


def step64(p, g, m, v, lr, b1, b2, eps, t):
    """One Adam step in float64 from fp32 inputs -> (p', m', v') as float64 arrays."""
    ss, bc = (float(x) for x in scalars(lr, b1, b2, t))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m1 = m + (1.0 - b1) * (g - m)
    v1 = b2 * v + (1.0 - b2) * g * g
    p1 = p - ss * m1 / (np.sqrt(v1) / bc + eps)
    return p1, m1, v1


def step32(p, g, m, v, lr, b1, b2, eps, t, wrong=None, ss_other=None):
    """adam1 of csrc/adam.hip in numpy fp32, every operation rounded on its own -> (p', m', v') fp32.

    wrong: one of MUTANTS, a deliberate mis-statement of the update (ss_other: the neighbouring tensor's step_size
    for "neighbour_step_size")."""
    f = np.float32
    ss, bc = scalars(lr, b1, b2, t)
    c1, b2f, c2, epsf = f(1.0 - b1), f(b2), f(1.0 - b2), f(eps)
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    if wrong == "swap_m_v":
        m, v = v, m
    if wrong == "neighbour_step_size":
        ss = f(ss_other)
    if wrong == "bc2_for_bc2_sqrt":
        bc = f(float(bc) ** 2)
    with np.errstate(all="ignore"):
        m1 = m + (f(b1) if wrong == "m_weight_b1" else c1) * (g - m)
        v1 = v * b2f + c2 * (g if wrong == "v_from_g" else g * g)
        if wrong == "eps_before_division":
            denom = (np.sqrt(v1) + epsf) / bc
        elif wrong == "eps_inside_sqrt":
            denom = np.sqrt(v1 + epsf) / bc
        else:
            denom = np.sqrt(v1) / bc + epsf
        p1 = p + (-ss) * (m1 / denom)
    if wrong == "swap_m_v":
        m1, v1 = v1, m1
    assert p1.dtype == m1.dtype == v1.dtype == f
    return p1, m1, v1


MUTANTS = ("bc2_for_bc2_sqrt", "eps_before_division", "eps_inside_sqrt", "v_from_g", "m_weight_b1",
           "neighbour_step_size", "swap_m_v")


def bars(p, g, m, v, lr, b1, b2, eps, t):
    """(bar_p, bar_m, bar_v): per-element bounds on |fp32 result - step64| (module docstring)."""
    ss, bc = (float(x) for x in scalars(lr, b1, b2, t))
    g64, m64, v64 = (np.asarray(a, np.float64) for a in (g, m, v))
    p1, m1, v1 = step64(p, g, m, v, lr, b1, b2, eps, t)
    bar_m = 4.0 * U * np.maximum(np.abs(m64), np.abs(g64))
    bar_v = 4.0 * U * np.maximum(v64, g64 * g64)
    denom = np.sqrt(v1) / bc + eps
    E = abs(ss) * (bar_m / denom + 16.0 * U * np.abs(m1) / denom)
    bar_p = 0.5 * ulp32(np.abs(p1) + E) + E
    return np.maximum(bar_p, TINY), np.maximum(bar_m, TINY), np.maximum(bar_v, TINY)


def accumulate(acc_m, acc_v, g, m, v, b1, b2):
    """Bars of the moments after one more step, from the bars before it (acc_*), the float64 reference's moments
    before the step (m, v) and the step's gradient."""
    g, m, v = (np.asarray(a, np.float64) for a in (g, m, v))
    am = b1 * acc_m + 4.0 * U * np.maximum(np.abs(m) + acc_m, np.abs(g))
    av = b2 * acc_v + 4.0 * U * np.maximum(v + acc_v, g * g)
    return np.maximum(am, TINY), np.maximum(av, TINY)


def worst(got, want, bar):
    """max over elements of |got - want| / bar (0 for an empty array)."""
    r = np.abs(np.asarray(got, np.float64) - want) / bar
    return float(r.max()) if r.size else 0.0


def compare(got, tensor, b1, b2, eps):
    """{"p": ratio, "m": ratio, "v": ratio}: the worst |got - step64| / bar of one tensor of a case; got = (p', m', v')."""
    args = (tensor["p"], tensor["g"], tensor["m"], tensor["v"], tensor["lr"], b1, b2, eps, tensor["t"])
    want, bar = step64(*args), bars(*args)
    return {k: worst(a, w, b) for k, a, w, b in zip("pmv", got, want, bar)}


# ---- the single-step states ----
def _prior(rng, n, gscale, steps, b1=B1, b2=B2):
    """Moments after `steps` steps of gradients ~ gscale N(0, 1), rounded to fp32."""
    m, v = np.zeros(n), np.zeros(n)
    for _ in range(steps):
        g = gscale * rng.standard_normal(n)
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
    return m.astype(np.float32), v.astype(np.float32)


def _signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _state(name, rng, n, k):
    """One tensor of state `name`: fp32 p, g, m, v and its own lr and step count t (k: its index in the call)."""
    f = np.float32
    p = rng.standard_normal(n).astype(f)
    lr, t = 1.6e-4 * (1.0 + 0.25 * k), 4 + k
    if name in ("training", "eps_1e-8", "lr_zero"):
        g = (1e-4 * rng.standard_normal(n)).astype(f)
        m, v = _prior(rng, n, 1e-4, 3)
        if name == "lr_zero":
            lr = 0.0
    elif name == "first_step":
        g = (1e-4 * rng.standard_normal(n)).astype(f)
        m, v, t = np.zeros(n, f), np.zeros(n, f), 1
    elif name == "late_step":
        g = (1e-4 * rng.standard_normal(n)).astype(f)
        m, v = _prior(rng, n, 1e-4, 40)
        lr, t = 1.6e-6 * (1.0 + 0.25 * k), 40000
    elif name == "zero_gradient":
        g = np.zeros(n, f)
        m, v = _prior(rng, n, 1e-4, 40)
        t = 5000
    elif name == "near_eps":  # sqrt(v') / bc2_sqrt = |g| at t = 1: 1e-17 .. 1e-13 around eps = 1e-15
        g = (_signs(rng, n) * 10.0 ** rng.uniform(-17.0, -13.0, n)).astype(f)
        m, v, t = np.zeros(n, f), np.zeros(n, f), 1
        lr = 1e-3 * (1.0 + 0.25 * k)
    elif name == "large_gradient":
        g = (_signs(rng, n) * 10.0 ** rng.uniform(-3.0, 3.0, n)).astype(f)
        m, v = _prior(rng, n, 30.0, 2)
        t = 3
    elif name == "cancelling":  # g within a few ulps of m, some equal to it, both signs
        m = (1e-3 * rng.standard_normal(n)).astype(f)
        g = (m.astype(np.float64) * (1.0 + 1e-6 * rng.standard_normal(n))).astype(f)
        g[::7] = m[::7]
        v = (m.astype(np.float64) ** 2 * rng.uniform(0.5, 2.0, n)).astype(f)
        t = 100
    else:
        raise KeyError(name)
    return {"p": p, "g": g, "m": m, "v": v, "lr": lr, "t": t, "numel": n}


STATES = ("training", "first_step", "late_step", "zero_gradient", "near_eps", "large_gradient", "lr_zero",
          "cancelling", "eps_1e-8")
_CASES = None


def cases():
    """{state: {"b1", "b2", "eps", "tensors": [one per NUMELS]}}: every tensor of a state goes into one
    dgs_adam_step call, with its own lr and step count. Built once from fixed seeds; do not modify the arrays."""
    global _CASES
    if _CASES is None:
        _CASES = {}
        for i, name in enumerate(STATES):
            rng = np.random.default_rng(1000 + i)
            tensors = [_state(name, rng, n, k) for k, n in enumerate(NUMELS)]
            for ten in tensors:
                for a in "pgmv":
                    ten[a].setflags(write=False)
            _CASES[name] = {"b1": B1, "b2": B2, "eps": 1e-8 if name == "eps_1e-8" else EPS, "tensors": tensors}
    return _CASES
