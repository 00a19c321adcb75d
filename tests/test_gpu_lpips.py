"""GPU: dgs_lpips / deformgs.lpips (csrc/lpips.hip) against the float64 restatement of tests/lpips_ref.py, on
seeded random weights (the real weight files are not assumed to exist anywhere this runs).

Sizes, three frames each (the last with img == gt): 16 x 16 (the minimum: the last tap is 1 x 1), 17 x 31 (odd
sides: every pool drops a row or a column), 35 x 45 (ragged against the 16 x 16 pixel tile), 33 x 130 (wider than
one tile row, ragged both ways), 64 x 48 (even throughout).

Bars against the float64 restatement, with e32 = |the same restatement in fp32 torch on the CPU - float64| on the
same inputs (another honest fp32 summation order):
  per tap:   max |gpu - ref| <= max(4 max e32 over that tap, 2^-23 max |tap|)
  per case:  every layer term and the sum: |gpu - ref| <= max(4 E, 2^-23 max |layer term|), E = the largest e32
             over all frames and the five layer terms of the case (a single scalar's fp32 error is too noisy to
             compare one to one).
A wrong border, pool or K padding misses these by orders of magnitude; another summation order does not.
Measured (MI355X, profiles/lpips_parity.jsonl; DESIGN.md section 4 has the table): worst tap error per size 3.1e-6 to
6.0e-6 with fp32 torch at 3.3e-6 to 6.4e-6; worst layer term or sum at 0.2 to 0.6 of the bar, 0.8 with a lin of both
signs. Written to the file DGS_PARITY_OUT names, when it is set.
"""
import functools
import json
import os

import pytest
import torch

import lpips_ref as ref

pytestmark = pytest.mark.gpu

CASES = {"16x16": (16, 16), "17x31": (17, 31), "35x45": (35, 45), "33x130": (33, 130), "64x48": (64, 48)}
ULP = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def weights(negative_lin=False):
    from deformgs.lpips import weights_from_tensors
    w = ref.random_weights(7, negative_lin)
    return w, weights_from_tensors(*w, "cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def reference(img, gt, w, normalize=False):
    """The float64 restatement and the fp32 one: taps of img and (F, 6) layer terms + sum, each."""
    d = {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        tx = ref.taps(img, w[0], w[1], normalize, dtype)
        ty = ref.taps(gt, w[0], w[1], normalize, dtype)
        terms = ref.layer_terms(tx, ty, w[2])
        d[tag] = {"taps": [t.double() for t in tx], "out": torch.cat([terms, terms.sum(1, keepdim=True)], 1).double()}
    return d


def check_terms(got, d, what):
    """got: (F, 6) gpu layer terms + sum against the case's bar; prints the worst of each column first."""
    want = d["f64"]["out"]
    E = (d["f32"]["out"][:, :5] - want[:, :5]).abs().max().item()
    bar = max(4 * E, ULP * want[:, :5].abs().max().item())
    err = (got.double() - want).abs()
    worst = err.max(0).values.tolist()
    print(f"{what}: worst |gpu - ref| per layer term and sum {['%.3e' % e for e in worst]} against bar {bar:.3e} "
          f"(E = {E:.3e})")
    assert (err <= bar).all(), f"{what}: {err.max().item():.3e} > {bar:.3e}"
    return {"term_err_max": worst, "bar": bar, "fp32_torch_err_max": E}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, both restatements and one GPU call of each kind, computed once."""
    from deformgs.lpips import lpips, vgg_taps
    H, W = CASES[name]
    w, gw = weights()
    img, gt = ref.pairs(H, W, seed=H * 1000 + W)
    d = reference(img, gt, w)
    d.update(img=img, gt=gt, a=img.cuda(), b=gt.cuda())
    total, layers = lpips(d["a"], d["b"], gw, return_layers=True)
    d["gpu_out"] = torch.cat([layers, total[:, None]], 1).cpu()
    d["gpu_taps"] = [t.cpu() for t in vgg_taps(d["a"], gw)]
    return d


@pytest.mark.parametrize("name", list(CASES))
def test_taps(name):
    d = case(name)
    H, W = CASES[name]
    report = {"case": name, "taps": []}
    for k, (g, o, s) in enumerate(zip(d["gpu_taps"], d["f64"]["taps"], d["f32"]["taps"])):
        assert tuple(g.shape) == (3, ref.TAP_CHANNELS[k], H >> k, W >> k)
        e32 = (s - o).abs().max().item()
        bar = max(4 * e32, ULP * o.abs().max().item())
        err = (g.double() - o).abs().max().item()
        print(f"tap {k}: max |gpu - ref| {err:.3e} against bar {bar:.3e} (fp32 torch {e32:.3e}, max |tap| "
              f"{o.abs().max().item():.3f}, zeros {(o == 0).double().mean().item():.2f})")
        report["taps"].append({"err_max": err, "bar": bar, "fp32_torch_err_max": e32})
        assert err <= bar, f"tap {k}: {err:.3e} > {bar:.3e}"
    report["terms"] = check_terms(d["gpu_out"], d, f"{name} layer terms")
    if os.environ.get("DGS_PARITY_OUT"):
        with open(os.environ["DGS_PARITY_OUT"], "a") as f:
            f.write(json.dumps(report) + "\n")


@pytest.mark.parametrize("name", list(CASES))
def test_layer_terms_and_exact_properties(name):
    from deformgs.lpips import lpips
    d = case(name)
    _, gw = weights()
    a, b, out = d["a"], d["b"], d["gpu_out"]
    check_terms(out, d, f"{name} layer terms")
    assert (d["f64"]["out"][:2] > 0).all(), "the noisy pairs differ in every layer"
    # the img == gt frame: exactly 0 in every layer
    assert torch.equal(d["img"][2], d["gt"][2]) and (out[2] == 0).all()

    def call(x, y, **kw):
        total, layers = lpips(x, y, gw, return_layers=True, **kw)
        return torch.cat([layers, total[:, None]], 1)
    assert torch.equal(bits(call(a, b)), bits(out)), "two identical calls"
    assert torch.equal(bits(call(b, a)), bits(out)), "lpips(a, b) == lpips(b, a)"
    singles = torch.cat([call(a[i], b[i]) for i in range(3)])
    assert torch.equal(bits(singles), bits(out)), "a frame alone == inside the batch"
    assert torch.equal(bits(call(a, b, scratch_bytes=1)), bits(out)), "one frame per chunk == unchunked"
    as_list = lpips(list(a), [y[None] for y in b], gw)
    assert as_list.shape == (3,) and torch.equal(bits(as_list), bits(out[:, 5]))


def test_normalize():
    """normalize=True on v and normalize=False on the fp32 2v - 1 both meet the bar of the normalised restatement
    (whose fp32 form rounds 2v - 1 the same way)."""
    from deformgs.lpips import lpips
    d = case("17x31")
    w, gw = weights()
    r = reference(d["img"], d["gt"], w, normalize=True)
    for what, (x, y, flag) in {"normalize=True": (d["a"], d["b"], True),
                               "2v - 1 given": (2 * d["a"] - 1, 2 * d["b"] - 1, False)}.items():
        total, layers = lpips(x, y, gw, normalize=flag, return_layers=True)
        check_terms(torch.cat([layers, total[:, None]], 1).cpu(), r, what)
    assert not torch.equal(r["f64"]["out"], d["f64"]["out"])


def test_negative_lin():
    from deformgs.lpips import lpips, weights_from_tensors
    d = case("35x45")
    w, gw = weights(True)
    assert all((l < 0).any() and (l > 0).any() for l in w[2])
    r = reference(d["img"], d["gt"], w)
    total, layers = lpips(d["a"], d["b"], gw, return_layers=True)
    out = torch.cat([layers, total[:, None]], 1).cpu()
    check_terms(out, r, "negative lin")
    assert (out[2] == 0).all()
    # all-negative lin: every term of a differing pair is negative, nothing clamps
    neg = weights_from_tensors(w[0], w[1], [-l.abs() for l in w[2]], "cuda")
    assert (lpips(d["a"][:2], d["b"][:2], neg, return_layers=True)[1] < 0).all()


def test_value_errors_in_both_layers():
    from deformgs import _lib
    from deformgs.lpips import lpips, vgg_taps
    _, gw = weights()
    x = torch.rand(2, 3, 16, 20, device="cuda")
    with pytest.raises(ValueError, match="CPU"):
        lpips(x.cpu(), x.cpu(), gw)
    with pytest.raises(ValueError, match="CPU"):
        lpips(x, x.cpu(), gw)
    with pytest.raises(ValueError, match="3 channels"):
        lpips(x[:, :1], x[:, :1], gw)
    with pytest.raises(ValueError, match="differ in shape"):
        lpips(x, x[:, :, :, :16], gw)
    with pytest.raises(ValueError, match="different sizes"):
        lpips([x[0], x[1, :, :, :16]], [x[0], x[1, :, :, :16]], gw)
    small = torch.rand(1, 3, 40, 15, device="cuda")
    with pytest.raises(ValueError, match="16"):
        lpips(small, small, gw)
    with pytest.raises(ValueError, match="16"):
        vgg_taps(small, gw)
    lib = _lib.load()
    out = torch.full((1, 6), 7.0, device="cuda")
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert lib.dgs_lpips_scratch_bytes(1, 40, 15) == 0 and lib.dgs_lpips_scratch_bytes(0, 40, 40) == 0
    assert lib.dgs_lpips_scratch_bytes(3, 17, 31) == 3 * lib.dgs_lpips_scratch_bytes(1, 17, 31) > 0
    args = (_lib.ptr(small), _lib.ptr(small), _lib.ptr(gw.packed))
    tail = (_lib.ptr(out), None, _lib.ptr(scratch), _lib.stream_ptr())
    assert lib.dgs_lpips(1, 40, 15, *args, 0, *tail) == -1 and b"16" in lib.dgs_last_error()
    assert lib.dgs_lpips(1, 40, 40, *args, 2, *tail) == -1
    assert lib.dgs_lpips(1, 40, 40, _lib.ptr(small), None, _lib.ptr(gw.packed), 0, *tail) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a rejected call launches nothing"


def test_metrics_script_lpips(tmp_path):
    """python -m deformgs.metrics --lpips_vgg --lpips_lin on PNG pairs of two sizes and random weight files."""
    from deformgs import metrics
    from deformgs.lpips import lpips
    from deformgs.png import write_png
    w, gw = weights()
    vgg, lin = ref.state_dicts(*w)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg_lin.pth")
    m = str(tmp_path / "model")
    for sub in ("renders", "gt"):
        os.makedirs(os.path.join(m, "test", "ours_1", sub))
    names, pairs = ["00000.png", "00001.png", "00002.png"], []
    for i, (n, (H, W)) in enumerate(zip(names, ((24, 40), (33, 20), (24, 40)))):
        img, gt = ref.pairs(H, W, seed=90 + i, frames=1, diff=0.0)
        img = (gt + 0.05 * torch.randn(gt.shape, generator=torch.Generator().manual_seed(i))).clamp(0, 1)
        pair = [(t[0].permute(1, 2, 0) * 255).round().to(torch.uint8) for t in (img, gt)]
        write_png(os.path.join(m, "test", "ours_1", "renders", n), pair[0].numpy())
        write_png(os.path.join(m, "test", "ours_1", "gt", n), pair[1].numpy())
        pairs.append([p.permute(2, 0, 1).float().cuda() / 255.0 for p in pair])

    def load():
        with open(os.path.join(m, "results.json")) as f:
            res = f.read()
        with open(os.path.join(m, "per_view.json")) as f:
            return res, f.read()
    metrics.main(["-m", m])
    plain = load()
    assert json.loads(plain[0])["ours_1"]["LPIPS"] is None
    metrics.main(["-m", m, "--lpips_vgg", str(tmp_path / "vgg16.pth"), "--lpips_lin", str(tmp_path / "vgg_lin.pth")])
    res, per = (json.loads(s) for s in load())
    assert set(res["ours_1"]) == {"SSIM", "PSNR", "LPIPS"} == set(per["ours_1"])
    values = [per["ours_1"]["LPIPS"][n] for n in names]
    assert all(isinstance(v, float) and v > 0 and v == v and v != float("inf") for v in values)
    assert isinstance(res["ours_1"]["LPIPS"], float) and res["ours_1"]["LPIPS"] == torch.tensor(values).mean().item()
    for v, (x, y) in zip(values, pairs):
        assert v == lpips(x, y, gw).item()
    for k in ("SSIM", "PSNR"):
        assert res["ours_1"][k] == json.loads(plain[0])["ours_1"][k]
    metrics.main(["-m", m, "--lpips_vgg", str(tmp_path / "vgg16.pth"), "--lpips_lin", str(tmp_path / "vgg_lin.pth"),
                  "--lpips_normalize"])
    assert json.loads(load()[1])["ours_1"]["LPIPS"][names[0]] == lpips(*pairs[0], gw, normalize=True).item()
    metrics.main(["-m", m])
    assert load() == plain, "without the flags both files are what they were"
