"""The deformation MLP's backward over the active set (csrc/mlp_active.h: dgs_deform_backward_active after
a DGS_MLP_NO_SAVE forward) against the full backward on the same dOut with its zero rows left in place,
against the float64 oracle, and through the native training step (DGS_MLP_ACTIVE_SET).

A row of zeros in dOut adds exactly +0 to every parameter gradient, so the two backwards differ only in
summation order and in the last bits of the recomputed activations (a 16-point tile shares one split
scale): the bar is test_gpu_native_step.py's, rtol 1e-4 and atol 1e-6 of each gradient's max. Against
float64 the bar is test_split_accuracy_matches_fp32's: at most twice the exact-fp32 path's error (+ 1e-6).
Shapes: N = 333 (5.2 blocks of 64, a ragged last one) with M in {0, 1, 16, 17, 64, 65, 129, 333} (the
16-point column tile, the 64-point block and their successors, nothing, everything) and N = 4099 with
M = 2050 (two rounds of dW chunks per workgroup), the active rows a random subset, the last M or the
first M."""
import numpy as np
import pytest
import torch

from helpers import _S_H
from oracle import mlp_ref
from weights import mlp_weights

pytestmark = pytest.mark.gpu

UNIFORM_T, NO_SAVE = 16, 32
NETS = {"blender": (True, False), "6dof": (True, True)}
T0 = 0.61


class _Net:
    """One network, its points and every buffer of the C ABI, allocated once per (name, N)."""

    def __init__(self, name, N):
        from deformgs import _lib
        from deformgs.deform_network import DeformNetworkBaseline
        self.lib, self._l = _lib.load(), _lib
        self.name, self.N = name, N
        self.bl, self.d6 = NETS[name]
        net = DeformNetworkBaseline(is_blender=self.bl, is_6dof=self.d6).cuda()
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        self.w = mlp_weights(shapes, 123)
        net.load_state_dict({k: torch.from_numpy(a) for k, a in self.w.items()})
        self.net = net
        by_id = {id(p): k for k, p in net.named_parameters()}
        self.names = [by_id[id(p)] for p in net.kernel_params()]  # the C ABI's table order
        self.params = [p.detach().contiguous() for p in net.kernel_params()]
        self.flags = net.flags | UNIFORM_T
        lib, fl = self.lib, self.flags
        self.nout = lib.dgs_deform_outputs(fl)
        rng = np.random.default_rng(11 + N)
        self.x_np = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
        self.x = torch.from_numpy(self.x_np).cuda()
        self.t = torch.full((1,), T0, device="cuda")
        e = lambda n: torch.empty(int(n), dtype=torch.float32, device="cuda")  # noqa: E731
        self.packed = e(lib.dgs_deform_packed_floats(fl))
        self.saved = e(lib.dgs_deform_saved_floats(fl, N))
        self.scratch = e(lib.dgs_deform_scratch_floats(fl, N))
        self.active = e(lib.dgs_deform_active_floats(fl, N))
        assert lib.dgs_deform_active_supported(fl, N) == 1
        self.stream = _lib.stream_ptr(self.x.device)

    def _grads(self):
        return [torch.full_like(p, float("nan")) for p in self.params]

    def forward(self, nosave):
        L, lib = self._l, self.lib
        out = torch.full((self.N, self.nout), float("nan"), device="cuda")
        if nosave:
            self.saved.fill_(float("nan"))  # nothing of an earlier saving forward may be used
        L.check(lib.dgs_deform_pack_forward(self.flags | (NO_SAVE if nosave else 0), L.ptr_array(self.params), self.N,
                                            L.ptr(self.x), L.ptr(self.t), L.ptr(self.packed), L.ptr(out),
                                            L.ptr(self.saved), self.stream), "pack_forward")
        return out

    def full(self, G):
        """Today's path: the saving forward, the backward over all N rows of G -> (out, grads, relu' masks)."""
        L, lib = self._l, self.lib
        out = self.forward(False)
        grads = self._grads()
        L.check(lib.dgs_deform_backward(self.flags, self.N, L.ptr(self.packed), L.ptr(self.saved), L.ptr(G),
                                        L.ptr(self.scratch), L.ptr_array(grads), self.stream), "backward")
        Ns = (self.N + 63) // 64 * 64
        sv = self.saved[: 2416 * Ns].view(2416, Ns)[:, :self.N]
        masks = {i: (sv[r:r + 256] > 0).T.cpu().numpy() for i, r in enumerate(_S_H)}
        torch.cuda.synchronize()
        return out, grads, masks

    def act(self, G):
        """The active-set path: the no-save forward, then the recompute backward -> (out, grads, M)."""
        L, lib = self._l, self.lib
        out = self.forward(True)
        self.active.fill_(float("nan"))
        self.scratch.fill_(float("nan"))
        grads = self._grads()
        L.check(lib.dgs_deform_backward_active(self.flags, self.N, L.ptr(self.x), L.ptr(self.packed), L.ptr(self.saved),
                                               L.ptr(G), L.ptr(self.scratch), L.ptr(self.active), None,
                                               L.ptr_array(grads), self.stream), "backward_active")
        torch.cuda.synchronize()
        m = int(self.active[:1].view(torch.int32).item())
        assert lib.dgs_debug_guard_expiries() == 0
        return out, grads, m


_NETS = {}


def _net(name, N):
    if (name, N) not in _NETS:
        _NETS[(name, N)] = _Net(name, N)
    return _NETS[(name, N)]


def _rows(N, M, place, seed=0):
    if place == "first":
        return np.arange(M)
    if place == "last":
        return np.arange(N - M, N)
    return np.sort(np.random.default_rng(1000 * seed + 7 * N + M).permutation(N)[:M])


def _dout(N, nout, rows, seed=5):
    """dOut from a seeded generator (fixed between runs): standard normal on `rows`, zero elsewhere."""
    G = np.zeros((N, nout))
    G[rows] = np.random.default_rng(seed).standard_normal((N, nout))[rows]
    return G


def _close(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a).all(), (what, k)
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * max(float(b.abs().max()), 1e-30),
                                   msg=lambda m: f"{what}, parameter {k}: {m}")


SHAPES = [("blender", 333, M) for M in (0, 1, 16, 17, 64, 65, 129, 333)] + [("blender", 4099, 2050), ("6dof", 333, 129)]


@pytest.mark.parametrize("place", ["random", "last", "first"])
@pytest.mark.parametrize("name,N,M", SHAPES, ids=[f"{n}-{N}-{M}" for n, N, M in SHAPES])
def test_active_matches_full_backward(name, N, M, place):
    net = _net(name, N)
    G = torch.from_numpy(_dout(N, net.nout, _rows(N, M, place))).float().cuda()
    out_f, g_full, _ = net.full(G)
    out_a, g_act, m = net.act(G)
    assert m == M
    assert torch.equal(out_a, out_f)
    if M == 0:
        for k, g in enumerate(g_act):
            assert float(g.abs().max()) == 0.0, k
    _close(g_act, g_full, f"{name} N={N} M={M} {place}")


def test_device_side_tail_split():
    """M just past one round of 64-point blocks per CU (ncu + ncu / 8 blocks): the kernels derive from M,
    on the device, a last round that runs as 16-point blocks (split_blocks: mask slots and first points
    of the tail blocks), which the smaller shapes never reach. Same bar against the full backward; two
    runs bitwise equal."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count - _net("blender", 333).lib.dgs_mlp_reserved_cus()
    M = 64 * (ncu + ncu // 8) - 7
    N = M + 3001
    net = _Net("blender", N)
    G = torch.from_numpy(_dout(N, net.nout, _rows(N, M, "random"))).float().cuda()
    out_f, g_full, _ = net.full(G)
    out_a, g_act, m = net.act(G)
    assert m == M and torch.equal(out_a, out_f)
    _close(g_act, g_full, f"tail N={N} M={M}")
    _, g_again, _ = net.act(G)
    for k, (a, b) in enumerate(zip(g_act, g_again)):
        assert torch.equal(a, b), k


def test_single_tiny_element_makes_a_row_active():
    """A row whose only nonzero element is 1e-30 belongs to the active set (the flag tests the bits, not
    a magnitude); -0.0 rows do not."""
    net = _net("blender", 333)
    rows = _rows(333, 64, "random", seed=3)
    G = _dout(333, net.nout, rows)
    tiny, negz = [i for i in range(333) if i not in set(rows)][:2]
    G[tiny, 4] = 1e-30
    G[negz, :] = -0.0
    Gt = torch.from_numpy(G).float().cuda()
    assert float(Gt[tiny, 4]) > 0.0
    _, g_full, _ = net.full(Gt)
    _, g_act, m = net.act(Gt)
    assert m == 65
    _close(g_act, g_full, "tiny element")


def test_active_is_deterministic():
    net = _net("blender", 4099)
    G = torch.from_numpy(_dout(4099, net.nout, _rows(4099, 2050, "random"))).float().cuda()
    _, g1, m1 = net.act(G)
    _, g2, m2 = net.act(G)
    assert m1 == m2 == 2050
    for k, (a, b) in enumerate(zip(g1, g2)):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("N", [333, 4099])
def test_nosave_forward_is_bitwise_the_saving_forward(N):
    net = _net("blender", N)
    a = net.forward(False)
    b = net.forward(True)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert net.lib.dgs_debug_guard_expiries() == 0


def _raw_grads(G, d6):
    if d6:
        return {"w_raw": G[:, 0:3], "v_raw": G[:, 3:6], "d_rot": G[:, 6:10], "d_scale": G[:, 10:13]}
    return {"d_xyz": G[:, 0:3], "d_rot": G[:, 3:7], "d_scale": G[:, 7:10]}


@pytest.mark.parametrize("name,N,M", [("blender", 4099, 2050), ("6dof", 333, 129)])
def test_active_accuracy_matches_fp32(name, N, M):
    """Against float64 (oracle/mlp_ref.py with the kernel's own relu' masks): the active-set path's max
    error per parameter gradient is at most twice the exact-fp32 path's (+ 1e-6, as
    test_split_accuracy_matches_fp32), on the same seeded dOut."""
    from helpers import mlp_relu_masks
    from deformgs.deform_network import DeformNetworkBaseline
    net = _net(name, N)
    G = _dout(N, net.nout, _rows(N, M, "random"))
    Gt = torch.from_numpy(G).float().cuda()
    t = np.full((N, 1), T0, np.float32)
    out, c = mlp_ref.forward(net.w, net.x_np, t, net.bl, net.d6)
    _, _, masks = net.full(Gt)
    _, g_act, m = net.act(Gt)
    assert m == M
    ref = mlp_ref.backward(net.w, c, out, _raw_grads(G, net.d6), net.bl, net.d6, False, relu_masks=masks)
    exact = DeformNetworkBaseline(is_blender=net.bl, is_6dof=net.d6, exact_fp32=True).cuda()
    exact.load_state_dict({k: torch.from_numpy(a) for k, a in net.w.items()})
    raw = exact.raw(net.x, torch.from_numpy(t).cuda())
    masks_e = mlp_relu_masks(raw, N, net.bl, True)
    (raw * Gt).sum().backward()
    ref_e = mlp_ref.backward(net.w, c, out, _raw_grads(G, net.d6), net.bl, net.d6, False, relu_masks=masks_e)
    got = dict(zip(net.names, g_act))
    checked = 0
    for k, p in exact.named_parameters():
        if k not in ref:
            continue
        err_a = float(np.abs(got[k].cpu().numpy() - ref[k]).max())
        err_e = float(np.abs(p.grad.cpu().numpy() - ref_e[k]).max())
        print(f"{name} N={N} M={M} {k}: active {err_a:.3e} exact {err_e:.3e}")
        assert err_a <= 2.0 * err_e + 1e-6, (k, err_a, err_e)
        checked += 1
    assert checked >= 10


def test_native_step_active_set(monkeypatch):
    """5k Gaussians at 256^2 through dgs_train_step: DGS_MLP_ACTIVE_SET=1 and =0 give the same image and
    loss bit for bit and the same gradients within the native step's tolerance; the step after a forced
    1 reports the active fraction."""
    from test_gpu_native_step import _model, _params
    from deformgs import native_step
    from deformgs.arguments import PipelineParams
    from deformgs.synthetic import synth_camera
    from deformgs.train_step import drop_grads, train_step
    dev = torch.device("cuda", 0)
    cam = synth_camera(256, 256, index=3, fid=0.43, device=dev)
    gt = torch.rand((3, 256, 256), generator=torch.Generator().manual_seed(5)).to(dev)
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DGS_MLP_ACTIVE_SET", mode)
        gs, deform = _model(5000, True, False)
        assert native_step.usable(gs, deform, pipe, gt)
        loss, pkg, redone = train_step(gs, deform, cam, gt, pipe, bg, False)
        torch.cuda.synchronize()
        ns = gs._dgs_native
        assert not redone and ns.active_used == (mode == "1")
        res[mode] = (float(loss), pkg["render"].clone(), [p.grad.clone() for p in _params(gs, deform)])
        if mode == "1":
            drop_grads(gs, deform)
            train_step(gs, deform, cam, gt, pipe, bg, False)
            torch.cuda.synchronize()
            assert ns.active_last is not None and 0.0 < ns.active_last <= 1.0
            assert ns.active_fraction is not None and 0.0 < ns.active_fraction <= 1.0
            print(f"active fraction at 5k / 256^2, camera 3: {ns.active_last:.4f}")
    assert res["0"][0] == res["1"][0]
    assert torch.equal(res["0"][1], res["1"][1])
    _close(res["1"][2], res["0"][2], "native step")
    from deformgs import _lib
    assert _lib.load().dgs_debug_guard_expiries() == 0
