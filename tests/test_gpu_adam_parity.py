"""GPU: the multi-tensor Adam (csrc/adam.hip k_adam / dgs_adam_step, deformgs/adam.py step_all) against the float64
reference and the derived bars of tests/adam_ref.py. tests/test_adam_ref.py shows on the CPU that fp32 arithmetic of
the kernel's form meets those bars and that a mis-stated update does not. tests/test_gpu_adam.py keeps the plain
comparison with torch.optim.Adam in fp32.

(a) one step from each state of adam_ref.cases() through the C ABI. Every numel (1, 3, 2047, 2048, 2049, 4101,
    70001: scalar only, one ragged block, one exact float4 block, a float4 block plus a scalar block, several of
    each) goes into the call eight times, with the (p, g, m, v) pointers at the float phases of PHASES: all four
    16-byte aligned (the float4 path), all shifted by one float, each pointer alone off alignment, and mixed ones, so
    that every pointer takes every phase (56 tensors: two launch tables). The tensors of a role live in one
    torch.empty arena, 1 to 3 sentinel floats apart; afterwards p, m, v are within the bars of step64 element by
    element, and every sentinel and the whole g arena are bit-identical.
(b) the aligned copy and the copies shifted off alignment of the same data come out bitwise equal: the float4 and the
    element path run the same arithmetic (adam1 states its three FMAs explicitly; left to the compiler the element path
    had rounded b2 v and (1 - b2) g g separately while the float4 path fused them).
(c) 1, 40, 41 and 85 table entries in one call, sizes from {1, 5, 2048, 2049, 6000}, every tensor with its own
    step_size and bc2_sqrt, with empty entries (numel 0, null or valid pointers) that take no slot of the 40-job
    launch table; n = 0 and a null pointer with numel > 0 (in the first launch's range and beyond it) write nothing.
(d) step_all on a 3000-row GaussianModel (6 tensors), the 6-DoF blender DeformNetwork (28) and a third optimizer of 8
    small tensors: 42 tensors, so the call spans two launch tables. About 30 steps with the events of training
    (TrainingScript) against torch.optim.Adam(foreach=False) on float64 CPU copies given the same gradients and edits,
    and against torch.optim.Adam in fp32 on the GPU through the same script. Measured errors: profiles/adam_parity.jsonl.
(e) betas / eps of a group changed after step_all cached its launch tables.
"""
import functools

import numpy as np
import pytest
import torch

import adam_ref as ref
from helpers import write_stats

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5  # a NaN: a gap read as a value shows up, and so does one overwritten by any number
GUARD = 64
# (p, g, m, v) start phases in floats past 16-byte alignment: all aligned, one pointer off at a time (the float4 path
# must test all four), and two mixed ones that complete 0..3 for every role
PHASES = ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (2, 3, 1, 2), (3, 1, 2, 3))
assert all({ph[r] for ph in PHASES} == {0, 1, 2, 3} for r in range(4))
ROLES = "pgmv"


# ---- arenas ----
def layout(numels, phases):
    """Offsets (in floats) of every tensor in the four role arenas: the tensors of a role are 1 to 3 floats apart and
    tensor i of role r starts at phase phases[i][r]. The order of the tensors is chosen so that such a gap exists
    (a gap of 0 or 4 floats is never used; the first tensor follows the leading guard at any phase).
    -> (order, {role: offsets by position}, arena length)."""
    n = len(numels)
    if phases is None:  # no phases asked for: the order as given, the same gaps (cycling through 1, 2, 3) in every
        # role, so the four pointers of a tensor share a phase and about a quarter of the tensors take the float4 path
        offs, cur = {r: [] for r in range(4)}, {r: GUARD for r in range(4)}
        for k in range(n):
            for r in range(4):
                offs[r].append(cur[r] + 1 + (k + k // 3) % 3)
                cur[r] = offs[r][-1] + numels[k]
        return list(range(n)), offs, max(cur.values()) + 3 + GUARD

    def follows(a, b):  # b may come after a: in every role b's phase is not the one a ends on
        return all((phases[b][r] - phases[a][r] - numels[a]) % 4 != 0 for r in range(4))

    rng = np.random.default_rng(0)
    for _ in range(5000):  # shuffled greedy orders (fixed seed) until one has such a gap everywhere
        todo, order = list(rng.permutation(n)), []
        while todo:
            # the tensor with the fewest possible successors left first: the hard ones are not kept for the end
            fits = [i for i in todo if not order or follows(order[-1], i)]
            if not fits:
                break
            pick = min(fits, key=lambda i: sum(follows(i, j) for j in todo if j != i))
            todo.remove(pick)
            order.append(int(pick))
        if not todo:
            break
    assert not todo, "no order of these tensors with 1-3 float gaps throughout was found"
    cur = {r: GUARD for r in range(4)}
    offs = {r: [] for r in range(4)}
    for pick in order:
        for r in range(4):
            start = cur[r] + (phases[pick][r] - cur[r]) % 4
            offs[r].append(start)
            cur[r] = start + numels[pick]
    return order, offs, max(cur.values()) + 3 + GUARD


class Call:
    """One dgs_adam_step call on tensors (dicts with fp32 p, g, m, v, lr, t) placed in four sentinel-filled arenas."""

    def __init__(self, tensors, phases, b1, b2, eps):
        from deformgs import _lib
        self.L, self.lib = _lib, _lib.load()
        self.tensors, self.cfg = tensors, (b1, b2, eps)
        numels = [t["numel"] for t in tensors]
        self.order, offs, total = layout(numels, phases)
        self.where = [None] * len(tensors)  # tensor -> (offset per role)
        for pos, i in enumerate(self.order):
            self.where[i] = tuple(offs[r][pos] for r in range(4))
        self.host = np.full((4, total), SENTINEL, np.int32)
        self.data = np.zeros((4, total), bool)
        for i, t in enumerate(tensors):
            for r, role in enumerate(ROLES):
                o = self.where[i][r]
                self.host[r, o:o + numels[i]] = t[role].view(np.int32)
                self.data[r, o:o + numels[i]] = True
        assert (~self.data[:, :GUARD]).all() and (~self.data[:, -GUARD:]).all()
        self.dev = []
        for r in range(4):
            a = torch.empty(total, dtype=torch.int32, device="cuda")
            a.copy_(torch.from_numpy(self.host[r]))
            assert a.data_ptr() % 16 == 0
            self.dev.append(a)

    def phase(self, i):
        return tuple((self.dev[r].data_ptr() // 4 + self.where[i][r]) % 4 for r in range(4))

    def entry(self, i, null=()):
        t = self.tensors[i]
        ss, bc = ref.scalars(t["lr"], self.cfg[0], self.cfg[1], t["t"])
        ptrs = [None if role in null else self.dev[r][self.where[i][r]:].data_ptr() for r, role in enumerate(ROLES)]
        return self.L.AdamTensor(*ptrs, t["numel"], float(ss), float(bc))

    def run(self, table):
        """table: AdamTensor entries (or an empty list) -> the call's return code, after a synchronize."""
        arr = (self.L.AdamTensor * max(len(table), 1))(*table)
        rc = self.lib.dgs_adam_step(len(table), arr, *self.cfg, self.L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def fetch(self):
        self.out = np.stack([a.cpu().numpy() for a in self.dev])
        return self.out

    def untouched(self):
        """Nothing but the p, m, v extents changed: every sentinel and the whole g arena keep their bits."""
        out = self.fetch()
        return bool((out[~self.data] == SENTINEL).all()) and np.array_equal(out[1], self.host[1])

    def unchanged(self):
        return np.array_equal(self.fetch(), self.host)

    def result(self, i):
        """(p', m', v') of tensor i as fp32 arrays (after fetch / untouched)."""
        n = self.tensors[i]["numel"]
        return tuple(self.out[r, self.where[i][r]:self.where[i][r] + n].view(np.float32) for r in (0, 2, 3))


def check_tensors(call, b1, b2, eps, what):
    worst, failures = {"p": 0.0, "m": 0.0, "v": 0.0}, []
    for i, t in enumerate(call.tensors):
        r = ref.compare(call.result(i), t, b1, b2, eps)
        for k, x in r.items():
            worst[k] = max(worst[k], x)
        if max(r.values()) > 1.0 or not all(np.isfinite(a).all() for a in call.result(i)):
            failures.append((i, t["numel"], call.phase(i), r))
    print(f"{what}: worst |gpu - float64| / bar  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")
    return worst, failures


# ---- (a), (b): one step from a given state ----
@functools.lru_cache(maxsize=None)
def state_call(state):
    c = ref.cases()[state]
    tensors = [t for t in c["tensors"] for _ in PHASES]
    phases = [ph for _ in c["tensors"] for ph in PHASES]
    call = Call(tensors, phases, c["b1"], c["b2"], c["eps"])
    for i in range(len(tensors)):
        assert call.phase(i) == phases[i]
    gaps = {call.where[b][r] - call.where[a][r] - tensors[a]["numel"]
            for a, b in zip(call.order, call.order[1:]) for r in range(4)}
    assert gaps <= {1, 2, 3}, gaps
    assert call.run([call.entry(i) for i in range(len(tensors))]) == 0
    clean = call.untouched()
    return call, clean


@pytest.mark.parametrize("state", ref.STATES)
def test_one_step_within_bars_of_float64(state):
    c = ref.cases()[state]
    call, clean = state_call(state)
    assert clean, "a sentinel or the gradient arena changed"
    worst, failures = check_tensors(call, c["b1"], c["b2"], c["eps"], state)
    assert not failures, failures[:5]
    if state == "lr_zero":  # step_size 0: p keeps its bits while the moments move
        for i, t in enumerate(call.tensors):
            p1, m1, v1 = call.result(i)
            assert np.array_equal(p1.view(np.int32), t["p"].view(np.int32))
            assert (m1 != t["m"]).any() and (v1 != t["v"]).any()


@pytest.mark.parametrize("state", ref.STATES)
def test_float4_and_element_paths_are_bitwise_equal(state):
    """Slot 0 of every numel has all four pointers 16-byte aligned (whole blocks take the float4 path), the others have
    at least one pointer off it (element path throughout): same data, same bits."""
    call, _ = state_call(state)
    k = len(PHASES)
    for base in range(0, len(call.tensors), k):
        assert call.phase(base) == (0, 0, 0, 0)
        want = call.result(base)
        for i in range(base + 1, base + k):
            assert any(call.phase(i))
            for name, a, b in zip("pmv", call.result(i), want):
                diff = a.view(np.int32) != b.view(np.int32)
                assert not diff.any(), (state, call.tensors[i]["numel"], call.phase(i), name, int(diff.sum()),
                                        "first at", int(np.argmax(diff)))


# ---- (c): the launch table ----
SIZES = (1, 5, 2048, 2049, 6000)


def chunk_tensors(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [SIZES[(3 * k + k // 5) % 5] for k in range(n)]
    return [ref._state("training", rng, s, k) for k, s in enumerate(sizes)]


# entries -> positions of empty entries ("null": numel 0 and null pointers; "valid": numel 0, valid pointers)
CHUNKS = {1: {}, 40: {}, 41: {17: "null"}, 85: {0: "null", 39: "valid", 40: "null", 84: "valid"}}


@pytest.mark.parametrize("n", sorted(CHUNKS))
def test_table_chunks(n):
    """n entries; with the empty ones left out 1, 40, 40 (one launch each) and 81 (three launches) jobs."""
    empties = CHUNKS[n]
    tensors = chunk_tensors(n - len(empties), seed=n)
    if n == 1:
        tensors[0] = ref._state("training", np.random.default_rng(1), 2049, 0)
    assert len({ref.scalars(t["lr"], ref.B1, ref.B2, t["t"]) for t in tensors}) == len(tensors)
    call = Call(tensors, None, ref.B1, ref.B2, ref.EPS)
    aligned = sum(call.phase(i) == (0, 0, 0, 0) for i in range(len(tensors)))
    assert n == 1 or 0 < aligned < len(tensors)  # both paths of k_adam in the call
    table, k = [], 0
    for pos in range(n):
        if pos in empties:
            e = call.entry(0, null=ROLES if empties[pos] == "null" else ())
            e.numel = 0
            table.append(e)
        else:
            table.append(call.entry(k))
            k += 1
    assert k == len(tensors) and len(table) == n
    assert call.run(table) == 0
    assert call.untouched(), "a sentinel or the gradient arena changed"
    _, failures = check_tensors(call, ref.B1, ref.B2, ref.EPS, f"{n} entries")
    assert not failures, failures[:5]


def test_refused_and_empty_calls_write_nothing():
    tensors = chunk_tensors(85, seed=7)
    call = Call(tensors, None, ref.B1, ref.B2, ref.EPS)
    assert call.lib.dgs_adam_step(0, None, ref.B1, ref.B2, ref.EPS, call.L.stream_ptr()) == 0
    assert call.run([]) == 0
    assert call.unchanged()
    empty = call.entry(3, null=ROLES)
    empty.numel = 0
    assert call.run([empty]) == 0 and call.unchanged()
    # a null pointer with numel > 0: among the first 40 jobs, and past them (no launch may precede the refusal)
    for bad, role in ((2, "p"), (30, "g"), (60, "m"), (84, "v")):
        table = [call.entry(i, null=role if i == bad else ()) for i in range(85)]
        assert call.run(table) == -1, (bad, role)
        assert b"dgs_adam_step" in call.lib.dgs_last_error()
        assert call.unchanged(), ("a refused call wrote", bad, role)
    assert call.run([call.entry(i) for i in range(85)]) == 0 and call.untouched()  # the same arenas then work
    _, failures = check_tensors(call, ref.B1, ref.B2, ref.EPS, "after the refusals")
    assert not failures, failures[:5]


# ---- (d), (e): step_all through the events of training ----
def torch_adam(groups, **kw):
    return torch.optim.Adam(groups, foreach=False, **kw)


GAUSS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
         ("scaling", "_scaling"), ("rotation", "_rotation"))
GRAD_SCALE = {"xyz": 1e-4, "f_dc": 1e-3, "f_rest": 1e-4, "opacity": 1e-2, "scaling": 1e-3, "rotation": 1e-3}
EXTRA_SHAPES = ((1,), (5,), (7, 3), (2049,), (2048,), (31, 67), (3,), (6000,))


class Track:
    """One copy of the trained state: a GaussianModel, the DeformNetwork's parameters and a third small optimizer, on
    `device` in `dtype`, stepped by `kind` ("hip": deformgs Adam through step_all; "torch": torch.optim.Adam)."""

    def __init__(self, kind, device, dtype, init):
        from deformgs.adam import Adam
        from deformgs.arguments import OptimizationParams
        from deformgs.gaussian_model import GaussianModel
        self.kind, self.device, self.dtype = kind, device, dtype
        cls = Adam if kind == "hip" else torch_adam
        conv = lambda a: a.to(device=device, dtype=dtype).clone()  # noqa: E731
        opt = OptimizationParams()
        self.gs = GaussianModel(3)
        self.gs.from_tensors(*(conv(init["gauss"][name]) for name in ("xyz", "f_dc", "f_rest", "scaling", "rotation",
                                                                     "opacity")))
        if device == "cpu":
            self.gs.row_select = lambda mask, ts: [t[mask] for t in ts]
        self.gs.training_setup(opt, optimizer_cls=cls)
        self.net = [torch.nn.Parameter(conv(w)) for w in init["net"]]
        self.net_opt = cls([{"params": self.net, "lr": opt.position_lr_init * 5, "name": "deform"}], lr=0.0, eps=1e-15)
        self.extra = [torch.nn.Parameter(conv(w)) for w in init["extra"]]
        self.extra_opt = cls([{"params": [p], "lr": 1e-3 * (i + 1), "name": f"extra{i}"}
                              for i, p in enumerate(self.extra)], lr=0.0, eps=1e-15)
        self.bufs = {}
        self.hits = 0

    def optimizers(self, which):
        return [o for o, on in ((self.gs.optimizer, True), (self.net_opt, which == "all"),
                                (self.extra_opt, which == "all")) if on]

    def params(self):
        """{slot: (optimizer, group, parameter)} in a fixed order; slots name the same tensor in every track."""
        out = {}
        for g in self.gs.optimizer.param_groups:
            out[g["name"]] = (self.gs.optimizer, g, g["params"][0])
        for i, p in enumerate(self.net):
            out[f"net{i}"] = (self.net_opt, self.net_opt.param_groups[0], p)
        for i, p in enumerate(self.extra):
            out[f"extra{i}"] = (self.extra_opt, self.extra_opt.param_groups[i], p)
        return out

    def set_grads(self, grads, noncontiguous=()):
        """grads: {slot: fp32 CPU tensor or None}. The gradient of a slot lives in one buffer for as long as the
        parameter object does (the native training step's persistent gradient buffers)."""
        for slot, (_, _, p) in self.params().items():
            g = grads.get(slot)
            if g is None:
                p.grad = None
                continue
            g = g.to(device=self.device, dtype=self.dtype)
            if slot in noncontiguous:
                p.grad = g.transpose(1, 2).contiguous().transpose(1, 2)
                assert not p.grad.is_contiguous()
                continue
            key = (slot, id(p), tuple(p.shape))
            if key not in self.bufs:
                self.bufs = {k: v for k, v in self.bufs.items() if k[0] != slot}
                self.bufs[key] = torch.empty_like(p)
            self.bufs[key].copy_(g)
            p.grad = self.bufs[key]

    def step(self, which):
        opts = self.optimizers(which)
        if self.kind == "hip":
            from deformgs.adam import step_all
            before = getattr(opts[0], "_dgs_fast", None)
            step_all(*opts)
            self.hits += int(before is not None and getattr(opts[0], "_dgs_fast", None) is before)
        else:
            for o in opts:
                o.step()

    def take_hits(self):
        h, self.hits = self.hits, 0
        return h


def initial_state(rows):
    from deformgs.deform_network import DeformNetwork
    from deformgs.synthetic import synth_gaussians
    g = synth_gaussians(rows, seed=2, device="cpu")
    torch.manual_seed(4)
    net = DeformNetwork(is_blender=True, is_6dof=True)
    gen = torch.Generator().manual_seed(5)
    return {"gauss": {"xyz": g["xyz"], "f_dc": g["features_dc"], "f_rest": g["features_rest"], "scaling": g["scaling"],
                      "rotation": g["rotation"], "opacity": g["opacity"]},
            "net": [p.detach().clone().float() for p in net.parameters()],
            "extra": [torch.randn(s, generator=gen) for s in EXTRA_SHAPES]}


class TrainingScript:
    """Drives the three tracks (HIP fp32, torch fp32 on the GPU, torch float64 on the CPU) through the same steps and
    edits, and holds the HIP track's moments to the accumulated bars after every step."""

    def __init__(self, rows, device="cuda"):
        init = initial_state(rows)
        self.hip = Track("hip", device, torch.float32, init)
        self.t32 = Track("torch", device, torch.float32, init)
        self.r64 = Track("torch", "cpu", torch.float64, init)
        self.tracks = (self.hip, self.t32, self.r64)
        assert all(o._hip for o in self.hip.optimizers("all")) == (device == "cuda")
        self.gen = torch.Generator().manual_seed(6)
        self.acc = {}  # slot -> (bar of exp_avg, bar of exp_avg_sq), float64 arrays shaped like the parameter
        self.steps = 0
        self.worst = {"m": 0.0, "v": 0.0}

    def count(self):
        return len(self.hip.params())

    def set_lrs(self):
        """update_learning_rate-style: every group of every optimizer gets a new lr before every step."""
        for tr in self.tracks:
            for slot, (_, group, _) in tr.params().items():
                group.setdefault("lr0", group["lr"])
                group["lr"] = group["lr0"] * 0.97 ** self.steps * (1.0 if self.steps % 2 else 0.9)

    def step(self, which="all", skip=(), noncontiguous=()):
        self.set_lrs()
        ref_params = self.r64.params()
        grads = {}
        for slot, (_, _, p) in ref_params.items():
            if slot in skip or (which == "gauss" and slot not in GRAD_SCALE):
                continue
            scale = GRAD_SCALE.get(slot, 1e-3 if slot.startswith("net") else 1e-2)
            grads[slot] = torch.randn(p.shape, generator=self.gen) * scale  # fp32, drawn on the CPU
        before = {}
        for slot in grads:
            opt, group, p = ref_params[slot]
            st = opt.state.get(p, {})
            before[slot] = tuple(st[k].numpy().copy() if k in st else np.zeros(p.shape) for k in ("exp_avg", "exp_avg_sq"))
        for tr in self.tracks:
            tr.set_grads(grads, noncontiguous)
            tr.step(which)
        self.steps += 1
        torch.cuda.synchronize()
        # step counts, then the moments against the float64 run within the accumulated bars
        hip_params, ref_params = self.hip.params(), self.r64.params()
        for slot, (opt, group, p) in ref_params.items():
            hopt, hgroup, hp = hip_params[slot]
            rst, hst = opt.state.get(p, {}), hopt.state.get(hp, {})
            assert ("step" in rst) == ("step" in hst), (slot, self.steps)
            if "step" in rst:
                assert float(rst["step"]) == float(hst["step"]), (slot, self.steps, float(rst["step"]), float(hst["step"]))
            if slot not in grads:
                continue
            assert hgroup["betas"] == group["betas"] and hgroup["eps"] == group["eps"]
            b1, b2 = group["betas"]
            am, av = self.acc.get(slot, (np.zeros(p.shape), np.zeros(p.shape)))
            m0, v0 = before[slot]
            am, av = ref.accumulate(am, av, grads[slot].numpy(), m0, v0, b1, b2)
            self.acc[slot] = (am, av)
            rm = ref.worst(hst["exp_avg"].cpu().numpy(), rst["exp_avg"].numpy(), am)
            rv = ref.worst(hst["exp_avg_sq"].cpu().numpy(), rst["exp_avg_sq"].numpy(), av)
            self.worst["m"], self.worst["v"] = max(self.worst["m"], rm), max(self.worst["v"], rv)
            assert rm <= 1.0 and rv <= 1.0, (slot, self.steps, rm, rv)

    # the edits: explicit rows and masks, so the fp32 and float64 models make the same decisions
    def densify(self, n_new):
        shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
        new = {k: torch.randn((n_new,) + s, generator=self.gen) * 0.5 for k, s in shapes.items()}
        for tr in self.tracks:
            c = {k: v.to(device=tr.device, dtype=tr.dtype) for k, v in new.items()}
            tr.gs.densification_postfix(c["xyz"], c["f_dc"], c["f_rest"], c["opacity"], c["scaling"], c["rotation"])
        for slot in shapes:
            am, av = self.acc[slot]
            pad = np.zeros((n_new,) + am.shape[1:])
            self.acc[slot] = (np.concatenate([am, pad]), np.concatenate([av, pad]))  # appended rows: zero moments

    def prune(self, frac):
        n = self.r64.gs._xyz.shape[0]
        mask = torch.rand(n, generator=self.gen) < frac
        mask[0], mask[n - 1] = True, False
        for tr in self.tracks:
            tr.gs.prune_points(mask.to(tr.device))
        keep = (~mask).numpy()
        for slot, _ in GAUSS:
            am, av = self.acc[slot]
            self.acc[slot] = (am[keep], av[keep])
        return int(mask.sum())

    def reset_opacity(self):
        for tr in self.tracks:
            tr.gs.reset_opacity()
        am, av = self.acc["opacity"]
        self.acc["opacity"] = (np.zeros_like(am), np.zeros_like(av))  # the moments are zeroed with the new values

    def parameter_errors(self):
        """{slot: (max |hip - f64|, max |torch fp32 - f64|, worst elementwise excess over 2 E32 + ulp)}."""
        out = {}
        hp, tp, rp = self.hip.params(), self.t32.params(), self.r64.params()
        for slot in rp:
            p64 = rp[slot][2].detach().numpy()
            eh = np.abs(hp[slot][2].detach().cpu().numpy().astype(np.float64) - p64)
            et = np.abs(tp[slot][2].detach().cpu().numpy().astype(np.float64) - p64)
            assert eh.shape == p64.shape == et.shape
            out[slot] = (float(eh.max()), float(et.max()), float((eh / (2.0 * et.max() + ref.ulp32(p64))).max()))
        return out

    def finish(self):
        from deformgs.adam import clear_fast_cache
        clear_fast_cache(self.hip.gs.optimizer, self.hip.net_opt, self.hip.extra_opt)


def check_parameters(script, tag, extra):
    """Each parameter's error against float64 at most twice torch fp32's on the same run plus one ulp of the
    parameter (elementwise: |hip - f64| <= 2 max|torch32 - f64| + ulp(p)); both errors go to the parity record."""
    errs = script.parameter_errors()
    for slot, (eh, et, ratio) in errs.items():
        print(f"{tag} {slot}: |hip - f64| {eh:.3e}  |torch fp32 - f64| {et:.3e}  worst / (2 E32 + ulp) {ratio:.3f}")
    write_stats(tag, {"device": torch.cuda.get_device_name(0), "steps": script.steps, "tensors": script.count(),
                      "moment_worst_over_bar": script.worst, **extra,
                      "param_max_err_hip_vs_f64": {s: e[0] for s, e in errs.items()},
                      "param_max_err_torch32_vs_f64": {s: e[1] for s, e in errs.items()},
                      "param_worst_over_bound": {s: e[2] for s, e in errs.items()}})
    bad = {s: e for s, e in errs.items() if e[2] > 1.0}
    assert not bad, bad


def test_step_all_through_training_events():
    """42 tensors (6 Gaussian + 28 DeformNetwork(is_blender, is_6dof) + 8 of a third optimizer), 28 steps."""
    s = TrainingScript(3000)
    assert s.count() == 42 and len(s.hip.net) == 28
    hits = {}
    for _ in range(10):  # warm-up: the Gaussian optimizer alone, the network's parameters have no gradient
        s.step("gauss")
    hits["warm_up"] = s.hip.take_hits()
    assert all(len(s.hip.net_opt.state.get(p, {})) == 0 for p in s.hip.net)
    for _ in range(4):   # both (and the third) in one step_all: step counts 11.. and 1..
        s.step()
    hits["joint"] = s.hip.take_hits()
    s.densify(500)
    assert s.hip.gs._xyz.shape[0] == 3500
    for _ in range(3):
        s.step()
    hits["after_densify"] = s.hip.take_hits()
    pruned = s.prune(0.12)
    assert 300 < pruned < 550 and s.hip.gs._xyz.shape[0] == 3500 - pruned
    for _ in range(3):
        s.step()
    hits["after_prune"] = s.hip.take_hits()
    s.reset_opacity()
    for _ in range(3):
        s.step()
    hits["after_opacity_reset"] = s.hip.take_hits()
    s.step(skip=("f_rest", "net3", "extra2"))  # parameters lacking a gradient: their step counts stay behind
    s.step(noncontiguous=("f_rest",))
    assert s.hip.take_hits() == 0              # neither is cacheable
    for _ in range(3):
        s.step()
    hits["after_irregular_steps"] = s.hip.take_hits()
    print("fast-path steps per segment:", hits, " moments worst / bar:", s.worst)
    # the cached tables were used between all edits: every step of a segment but its first (the warm-up's first
    # builds them, the others follow a changed parameter set)
    assert hits == {"warm_up": 9, "joint": 3, "after_densify": 2, "after_prune": 2, "after_opacity_reset": 2,
                    "after_irregular_steps": 2}, hits
    assert s.steps == 28
    check_parameters(s, "adam_parity", {"fast_path_steps": hits, "rows_end": int(s.hip.gs._xyz.shape[0])})
    s.finish()


def test_group_betas_and_eps_changed_after_caching():
    """torch.optim.Adam reads a group's betas and eps on every step; so must step_all once its tables are cached."""
    s = TrainingScript(300)
    for _ in range(3):
        s.step()
    assert s.hip.take_hits() == 2
    for tr in s.tracks:
        params = tr.params()
        params["xyz"][1]["betas"] = (0.8, 0.99)
        params["opacity"][1]["eps"] = 1e-8
        params["net5"][1]["eps"] = 1e-8  # the whole network group
    for _ in range(2):
        s.step()
    hits_changed = s.hip.take_hits()
    for _ in range(2):
        s.step()
    assert s.hip.take_hits() == 2          # and the new configuration is cached again
    print("moments worst / bar:", s.worst)
    check_parameters(s, "adam_parity_group_change", {"fast_path_steps_after_change": hits_changed})
    s.finish()
