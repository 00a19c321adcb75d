"""GPU: dgs_image_metrics / deformgs.image_metrics (csrc/metrics.hip) against the float64 restatement of
tests/ms_ssim_ref.py.

Shapes: 161 x 163 (odd and even pooling at every level: 161 -> 81 -> 41 -> 21 -> 11, 163 -> 82 -> 41 -> 21 -> 11, a
1 x 1 map at level 4, partial tiles everywhere), 200 x 176 (several full tiles in a row, an even side that pools
without padding first) and a single frame. Frame 0 is a seeded smooth pattern + noise (gt) against gt + smaller
noise (img); frame 1 is img against 1 - img (a negative cs, so MS-SSIM is exactly 0); frame 2 is img == gt.

Tolerances, per quantity q against the float64 oracle, with e32(q) = |the same restatement in fp32 torch on the
CPU - oracle| on the same inputs and ulp = one fp32 ulp of 1.0 (2^-23):
  per-level cs / ssim, MS-SSIM:  |gpu - oracle| <= max(4 e32, ulp)     (another summation order; a wider gap is
                                                                        a wrong border or pool)
  SSIM:                          |gpu - oracle| <= 2 |fused_ssim - oracle| + ulp
  PSNR: the bound is set in mse, relative: r = max(4 e32(mse) / mse, ulp). PSNR = -10 log10(mse), so an mse within
        r is a PSNR within (10 / ln 10) r (1 + r); the kernel returns PSNR as an fp32 number, whose own rounding
        (half a spacing of fp32 at that value) is added.
Identical frames: every level exactly 1.0, PSNR +inf. Anti-correlated frame: MS-SSIM exactly 0.0.
Measured errors (MI355X): profiles/image_metrics_parity.jsonl, written when DGS_PARITY_OUT names a file.
"""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import ms_ssim_ref as ref

pytestmark = pytest.mark.gpu

ULP = float(np.finfo(np.float32).eps)
CASES = {"161x163": (3, 161, 163), "200x176": (3, 200, 176), "single": (1, 161, 163)}


def frames(F, H, W):
    img, gt = ref.pattern_pair(H, W, seed=H + W)
    pairs = [(img, gt), (img, 1.0 - img), (gt, gt)][:F]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the float64 oracle, the fp32 restatement and one GPU call with every metric, computed once."""
    from deformgs.image_metrics import image_metrics
    from deformgs.metrics import fused_ssim
    F, H, W = CASES[name]
    img, gt = frames(F, H, W)
    d = {"img": img, "gt": gt}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        ms, levels = ref.ms_ssim(img, gt, dtype)
        p, mse = ref.psnr(img, gt, dtype)
        d[tag] = {"ms_ssim": ms.double(), "levels": levels.double(), "psnr": p.double(), "mse": mse.double(),
                  "ssim": ref.ssim(img, gt, dtype).double()}
    a, b = img.cuda(), gt.cuda()
    out = image_metrics(a, b)
    d["gpu"] = {k: v.cpu().double() for k, v in out.items()}
    d["fused_ssim"] = torch.stack([fused_ssim(a[i:i + 1], b[i:i + 1]) for i in range(F)]).cpu().double()
    report = {"case": name, "F": F, "H": H, "W": W, "device": torch.cuda.get_device_name(0)}
    for q in ("ms_ssim", "levels", "ssim"):
        report[q] = {"gpu_err_max": (d["gpu"][q] - d["f64"][q]).abs().max().item(),
                     "fp32_torch_err_max": (d["f32"][q] - d["f64"][q]).abs().max().item()}
    for lv in range(5):
        report[f"level{lv}"] = {"gpu_err_max": (d["gpu"]["levels"][:, :, lv] - d["f64"]["levels"][:, :, lv]).abs().max().item(),
                                "fp32_torch_err_max": (d["f32"]["levels"][:, :, lv] - d["f64"]["levels"][:, :, lv]).abs().max().item()}
    report["ssim"]["fused_ssim_err_max"] = (d["fused_ssim"] - d["f64"]["ssim"]).abs().max().item()
    fin = torch.isfinite(d["f64"]["psnr"])
    gpu_mse = 10.0 ** (-d["gpu"]["psnr"][fin] / 10.0)
    report["mse_rel"] = {"gpu_err_max_from_fp32_psnr": ((gpu_mse - d["f64"]["mse"][fin]).abs() / d["f64"]["mse"][fin]).max().item(),
                         "fp32_torch_err_max": ((d["f32"]["mse"][fin] - d["f64"]["mse"][fin]).abs() / d["f64"]["mse"][fin]).max().item()}
    report["psnr_abs"] = {"gpu_err_max": (d["gpu"]["psnr"][fin] - d["f64"]["psnr"][fin]).abs().max().item()}
    d["report"] = report
    print(json.dumps(report))
    if os.environ.get("DGS_PARITY_OUT"):
        with open(os.environ["DGS_PARITY_OUT"], "a") as f:
            f.write(json.dumps(report) + "\n")
    return d


def within(got, want, e32, what):
    """|got - want| <= max(4 e32, ulp) element by element; prints the worst before asserting."""
    err, bar = (got - want).abs(), torch.clamp(4 * e32, min=ULP)
    worst = (err / bar).argmax()
    print(f"{what}: worst err {err.flatten()[worst].item():.3e} against bar {bar.flatten()[worst].item():.3e} "
          f"(fp32 torch {e32.flatten()[worst].item():.3e})")
    assert (err <= bar).all(), f"{what}: {err.flatten()[worst].item():.3e} > {bar.flatten()[worst].item():.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_ms_ssim_levels_and_value(name):
    d = case(name)
    g, o, s = d["gpu"], d["f64"], d["f32"]
    within(g["levels"], o["levels"], (s["levels"] - o["levels"]).abs(), "per-level cs / ssim")
    within(g["ms_ssim"], o["ms_ssim"], (s["ms_ssim"] - o["ms_ssim"]).abs(), "MS-SSIM")
    assert (o["levels"][0, 0] > 0).all(), "the noisy pair keeps every level's cs positive"
    if CASES[name][0] == 3:
        assert (o["levels"][1, 0] < 0).any() and g["ms_ssim"][1].item() == 0.0   # anti-correlated
        assert torch.equal(g["levels"][2], torch.ones_like(g["levels"][2]))      # identical
        assert g["ms_ssim"][2].item() == 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_ssim_against_fused(name):
    d = case(name)
    err = (d["gpu"]["ssim"] - d["f64"]["ssim"]).abs()
    fused = (d["fused_ssim"] - d["f64"]["ssim"]).abs()
    print(f"SSIM: batched err {err.tolist()}, fused_ssim err {fused.tolist()}")
    assert (err <= 2 * fused + ULP).all()


@pytest.mark.parametrize("name", list(CASES))
def test_psnr(name):
    d = case(name)
    g, o, s = d["gpu"], d["f64"], d["f32"]
    for i in range(CASES[name][0]):
        if o["mse"][i].item() == 0.0:
            assert g["psnr"][i].item() == math.inf
            continue
        r = max(4 * abs(s["mse"][i].item() - o["mse"][i].item()) / o["mse"][i].item(), ULP)
        bar = 10 / math.log(10) * r * (1 + r) + 0.5 * float(np.spacing(np.float32(o["psnr"][i].item())))
        err = abs(g["psnr"][i].item() - o["psnr"][i].item())
        print(f"PSNR frame {i}: err {err:.3e} dB against bar {bar:.3e} dB (mse bound {r:.3e} relative)")
        assert err <= bar


def test_two_calls_are_bitwise_equal_and_frames_do_not_mix():
    from deformgs.image_metrics import image_metrics
    d = case("161x163")
    a, b = d["img"].cuda(), d["gt"].cuda()

    def call(x, y):
        r = image_metrics(x, y)
        return torch.cat([torch.stack([r["psnr"], r["ssim"], r["ms_ssim"]], 1), r["levels"].flatten(1)], 1).cpu()
    first, second = call(a, b), call(a, b)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(first.view(torch.int32), torch.cat([d["gpu"][k].float().view(3, -1) for k in
                                                           ("psnr", "ssim", "ms_ssim", "levels")], 1).view(torch.int32))
    singles = torch.cat([call(a[i:i + 1], b[i:i + 1]) for i in range(3)])
    assert torch.equal(first.view(torch.int32), singles.view(torch.int32))
    # lists of (C, H, W) and of (1, C, H, W) frames are the same batch
    as_list = image_metrics(list(a), [y[None] for y in b], ("ssim",))["ssim"].cpu()
    assert torch.equal(as_list, first[:, 1])


def test_unrequested_slots_are_nan():
    from deformgs.image_metrics import image_metrics
    d = case("single")
    a, b = d["img"].cuda(), d["gt"].cuda()
    r = image_metrics(a, b, ("psnr",))
    assert set(r) == {"psnr", "levels"} and torch.isnan(r["levels"]).all()
    assert r["psnr"].cpu().double().equal(d["gpu"]["psnr"])
    raw = image_metrics(a, b, ("ms_ssim",))
    base = raw["ms_ssim"]._base if raw["ms_ssim"]._base is not None else raw["ms_ssim"]
    assert torch.isnan(base[:, :2]).all() and not torch.isnan(base[:, 2:]).any()
    assert raw["levels"].cpu().double().equal(d["gpu"]["levels"])
    # small frames: PSNR and SSIM have no size rule
    x = torch.rand(2, 3, 37, 45, device="cuda")
    r = image_metrics(x, x.flip(0), ("psnr", "ssim"))
    assert torch.isfinite(r["psnr"]).all() and torch.isfinite(r["ssim"]).all()


def test_size_rule_in_both_layers():
    from deformgs import _lib
    from deformgs.image_metrics import image_metrics
    lib = _lib.load()
    x = torch.rand(1, 3, 160, 200, device="cuda")
    out = torch.full((1, 33), 7.0, device="cuda")
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    args = (_lib.ptr(x), _lib.ptr(x))
    assert lib.dgs_image_metrics_scratch_bytes(1, 3, 160, 200, 4) == 0
    assert lib.dgs_image_metrics(1, 3, 160, 200, *args, 4, _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr()) == -1
    assert b"160" in lib.dgs_last_error()
    assert lib.dgs_image_metrics(1, 3, 160, 200, *args, 0, _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr()) == -1
    assert lib.dgs_image_metrics(0, 3, 160, 200, *args, 1, _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr()) == -1
    assert lib.dgs_image_metrics(1, 3, 160, 200, None, _lib.ptr(x), 1, _lib.ptr(out), _lib.ptr(scratch),
                                 _lib.stream_ptr()) == -1
    assert lib.dgs_image_metrics(1, 3, 160, 200, *args, 1, _lib.ptr(out), ctypes.c_void_p(None), _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a rejected call launches nothing"
    with pytest.raises(ValueError, match="160"):
        image_metrics(x, x, ("ms_ssim",))
    assert image_metrics(x, x, ("psnr", "ssim"))["psnr"].item() == math.inf


def test_training_report_ms_ssim():
    """--report_ms_ssim: the test entry of a report gains SSIM and MS-SSIM and the log line names them; frames of
    160 pixels or less report SSIM only."""
    from deformgs.arguments import ModelParams, OptimizationParams, PipelineParams
    from deformgs.gaussian_model import GaussianModel
    from deformgs.train import SyntheticScene, training
    opt = OptimizationParams(iterations=2, warm_up=1, sequence_length=4)
    for res, has_ms in (((176, 168), True), ((64, 48), False)):
        scene = SyntheticScene(2000, res[0], res[1], n_train=4, n_test=2, seed=3, device="cuda")
        g = scene.init_gaussians(GaussianModel(3))
        torch.manual_seed(0)
        lines = []
        hist = training(ModelParams(is_blender=True), opt, PipelineParams(), [2], [], scene, g, log=lines.append,
                        report_ms_ssim=True)
        rep = hist["report"][2]
        assert len(rep["test"]) == 4 and len(rep["train"]) == 2
        l1, p, s, ms = rep["test"]
        assert 0 < l1 < 1 and p > 0 and -1 <= s <= 1
        line = [x for x in lines if "Evaluating test" in x][0]
        assert f"PSNR {p} SSIM {s} MS-SSIM {ms}" in line
        assert (0 < ms <= 1) if has_ms else ms is None


def test_metrics_script_ms_ssim(tmp_path):
    """python -m deformgs.metrics --ms_ssim on 176 x 161 PNG pairs: the old key set without the flag, MS-SSIM of the
    decoded bytes and D-SSIM = (1 - MS-SSIM) / 2 with it."""
    from deformgs import metrics
    from deformgs.png import write_png
    m = str(tmp_path)
    names = ["00000.png", "00001.png", "00002.png"]
    for sub in ("renders", "gt"):
        os.makedirs(os.path.join(m, "test", "ours_1", sub))
    pairs = []
    for i, n in enumerate(names):
        img, gt = ref.pattern_pair(161, 176, seed=40 + i)
        pair = [(t.permute(1, 2, 0) * 255).round().to(torch.uint8) for t in (img, gt)]
        write_png(os.path.join(m, "test", "ours_1", "renders", n), pair[0].numpy())
        write_png(os.path.join(m, "test", "ours_1", "gt", n), pair[1].numpy())
        pairs.append([p.permute(2, 0, 1).float() / 255.0 for p in pair])

    def load():
        with open(os.path.join(m, "results.json")) as f:
            res = json.load(f)
        with open(os.path.join(m, "per_view.json")) as f:
            return res, json.load(f)
    metrics.evaluate([m])
    res0, per0 = load()
    assert set(res0["ours_1"]) == {"SSIM", "PSNR", "LPIPS"} and set(per0["ours_1"]) == {"SSIM", "PSNR", "LPIPS"}
    metrics.main(["-m", m, "--ms_ssim"])
    res, per = load()
    assert set(res["ours_1"]) == {"SSIM", "PSNR", "LPIPS", "MS-SSIM", "D-SSIM"} == set(per["ours_1"])
    for k in ("SSIM", "PSNR", "LPIPS"):
        assert res["ours_1"][k] == res0["ours_1"][k] and per["ours_1"][k] == per0["ours_1"][k]
    x, y = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    want, _ = ref.ms_ssim(x, y)
    e32 = (ref.ms_ssim(x, y, torch.float32)[0].double() - want).abs()
    got = torch.tensor([per["ours_1"]["MS-SSIM"][n] for n in names], dtype=torch.float64)
    within(got, want, e32, "metrics --ms_ssim per view")
    assert [per["ours_1"]["D-SSIM"][n] for n in names] == [(1 - v) / 2 for v in got.tolist()]
    assert res["ours_1"]["MS-SSIM"] == torch.tensor(got.tolist()).mean().item()
    assert res["ours_1"]["D-SSIM"] == (1 - res["ours_1"]["MS-SSIM"]) / 2
