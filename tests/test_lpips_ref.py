"""CPU: the float64 LPIPS-VGG restatement (tests/lpips_ref.py) against closed forms, the weight-file loader of
deformgs/lpips.py on both key layouts of both files, and the metrics script's flags."""
import math

import pytest
import torch

import lpips_ref as ref

# float64 sums of a few hundred equal pixel values: n * 2^-53 relative at the very worst, on values near 0.1
TOL = 1e-13


def test_equal_images_score_zero_and_arguments_swap():
    w = ref.random_weights(1)
    img, gt = ref.pairs(17, 31, seed=5)
    total, terms = ref.lpips(img, gt, w)
    assert torch.equal(img[2], gt[2]) and total[2].item() == 0.0 and (terms[2] == 0).all()
    assert (terms[:2] > 0).all() and torch.equal(total, terms.sum(1))
    back, back_terms = ref.lpips(gt, img, w)
    assert torch.equal(back, total) and torch.equal(back_terms, terms)
    taps = ref.taps(img, w[0], w[1])
    assert [tuple(t.shape[1:]) for t in taps] == [(64, 17, 31), (128, 8, 15), (256, 4, 7), (512, 2, 3), (512, 1, 1)]
    for t in taps:  # the random weights keep every tap O(1) and about half of it zero
        assert 0.2 < (t == 0).double().mean().item() < 0.8 and 0.1 < t.abs().max().item() < 100


def test_min_side():
    w = ref.random_weights(1)
    with pytest.raises(ValueError):
        ref.lpips(torch.rand(1, 3, 15, 40), torch.rand(1, 3, 15, 40), w)


def test_hand_computed_first_tap():
    """Centre-tap identity weights carry the scaled red and green planes to tap 1; with constant images and a lin
    that weights only those two channels of tap 1 the score is two terms one can write down."""
    ws = [torch.zeros((co, ci, 3, 3)) for ci, co in ref.CHANNELS]
    bs = [torch.zeros(co) for _, co in ref.CHANNELS]
    ws[0][0, 0, 1, 1] = ws[0][1, 1, 1, 1] = 1.0
    ws[1][0, 0, 1, 1] = ws[1][1, 1, 1, 1] = 1.0
    lins = [torch.zeros((1, c, 1, 1)) for c in ref.TAP_CHANNELS]
    lins[0][0, 0], lins[0][0, 1] = 0.75, 0.25
    x = torch.tensor([0.5, 0.25, 0.9]).view(1, 3, 1, 1).expand(1, 3, 16, 18).contiguous()
    y = torch.tensor([0.125, 0.75, 0.1]).view(1, 3, 1, 1).expand(1, 3, 16, 18).contiguous()
    total, terms = ref.lpips(x, y, (ws, bs, lins))

    def unit(r, g):
        a, b = (r + 0.030) / 0.458, (g + 0.088) / 0.448
        n = math.sqrt(a * a + b * b) + 1e-10
        return a / n, b / n
    (ax, bx), (ay, by) = unit(0.5, 0.25), unit(0.125, 0.75)
    want = 0.75 * (ax - ay) ** 2 + 0.25 * (bx - by) ** 2
    assert abs(terms[0, 0].item() - want) < TOL and (terms[0, 1:] == 0).all()
    assert abs(total.item() - want) < TOL
    # normalize: 2v - 1 first
    (ax, bx), (ay, by) = unit(2 * 0.75 - 1, 2 * 0.625 - 1), unit(2 * 0.875 - 1, 2 * 0.5 - 1)
    x2 = torch.tensor([0.75, 0.625, 0.0]).view(1, 3, 1, 1).expand(1, 3, 16, 16).contiguous()
    y2 = torch.tensor([0.875, 0.5, 1.0]).view(1, 3, 1, 1).expand(1, 3, 16, 16).contiguous()
    want = 0.75 * (ax - ay) ** 2 + 0.25 * (bx - by) ** 2
    assert abs(ref.lpips(x2, y2, (ws, bs, lins), normalize=True)[0].item() - want) < TOL


def test_pool_drops_odd_edge_and_border_is_zero():
    """A 3x3 box filter of ones on a constant plane counts the taps inside the image (4, 6, 9); the pooled map of
    an odd side has floor(side / 2) entries."""
    ws = [torch.zeros((co, ci, 3, 3)) for ci, co in ref.CHANNELS]
    bs = [torch.zeros(co) for _, co in ref.CHANNELS]
    ws[0][0, 0] = 1.0
    ws[1][0, 0, 1, 1] = 1.0
    x = torch.full((1, 3, 17, 19), 0.428)  # red plane: (0.428 + 0.030) / 0.458 = 1
    t = ref.taps(x, ws, bs)
    assert torch.allclose(t[0][0, 0, 0, 0], torch.tensor(4.0, dtype=torch.float64), atol=1e-6)  # x is a float32 0.428
    assert torch.allclose(t[0][0, 0, 0, 5], torch.tensor(6.0, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(t[0][0, 0, 8, 8], torch.tensor(9.0, dtype=torch.float64), atol=1e-6)
    assert t[1].shape[-2:] == (8, 9) and t[4].shape[-2:] == (1, 1)


@pytest.mark.parametrize("vgg_prefix", ["features.", ""])
@pytest.mark.parametrize("lin_style", ["lpips", "renamed"])
def test_loader_accepts_both_layouts(tmp_path, vgg_prefix, lin_style):
    from deformgs import lpips
    ws, bs, lins = ref.random_weights(2)
    vgg, lin = ref.state_dicts(ws, bs, lins, vgg_prefix, lin_style)
    vgg["classifier.0.weight"] = torch.zeros(4, 4)  # other keys are ignored
    torch.save(vgg, tmp_path / "vgg.pth")
    torch.save(lin, tmp_path / "lin.pth")
    got = lpips.load_weights(str(tmp_path / "vgg.pth"), str(tmp_path / "lin.pth"), "cpu")
    want = lpips.weights_from_tensors(ws, bs, lins, "cpu")
    assert torch.equal(got.packed, want.packed)
    # the packed layout of include/dgs.h: conv 0 first, [Cin_p / 16][Cout][tap][16] with zeros past channel 3
    first = want.packed[:64 * 9 * 16].view(64, 9, 16)
    assert torch.equal(first[:, :, :3], ws[0].flatten(2).permute(0, 2, 1)) and (first[:, :, 3:] == 0).all()
    assert torch.equal(want.packed[64 * 9 * 16:64 * 9 * 16 + 64], bs[0])
    second = want.packed[64 * 9 * 16 + 64:][:64 * 64 * 9].view(4, 64, 9, 16)
    assert second[2, 5, 7, 3].item() == ws[1][5, 2 * 16 + 3, 2, 1].item()
    assert torch.equal(want.packed[-512:], lins[4].flatten())


def test_loader_names_missing_key_and_wrong_shape(tmp_path):
    from deformgs import lpips
    ws, bs, lins = ref.random_weights(2)
    vgg, lin = ref.state_dicts(ws, bs, lins)
    paths = str(tmp_path / "vgg.pth"), str(tmp_path / "lin.pth")

    def load(v, l):
        torch.save(v, paths[0])
        torch.save(l, paths[1])
        return lpips.load_weights(*paths, "cpu")
    with pytest.raises(ValueError, match=r"features\.17\.bias"):
        load({k: v for k, v in vgg.items() if k != "features.17.bias"}, lin)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        load(vgg, {k: v for k, v in lin.items() if k != "lin3.model.1.weight"})
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 3, 3\)"):
        load({**vgg, "features.5.weight": torch.zeros(128, 32, 3, 3)}, lin)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight.*\(1, 128, 1, 1\)"):
        load(vgg, {**lin, "lin1.model.1.weight": torch.zeros(1, 64, 1, 1)})
    with pytest.raises(ValueError, match="convolution 2 weight"):
        lpips.weights_from_tensors(ws[:2] + [ws[2][:, :32]] + ws[3:], bs, lins, "cpu")


def test_parser_flags():
    from deformgs import metrics
    a = metrics.parse_args(["-m", "x"])
    assert a.lpips_vgg is None and a.lpips_lin is None and not a.lpips_normalize
    a = metrics.parse_args(["-m", "x", "--lpips_vgg", "v.pth", "--lpips_lin", "l.pth", "--lpips_normalize"])
    assert (a.lpips_vgg, a.lpips_lin, a.lpips_normalize) == ("v.pth", "l.pth", True)
    for bad in (["--lpips_vgg", "v.pth"], ["--lpips_lin", "l.pth"], ["--lpips_normalize"]):
        with pytest.raises(SystemExit) as e:
            metrics.parse_args(["-m", "x"] + bad)
        assert e.value.code == 2


def test_lpips_rejects_cpu_tensors_and_bad_shapes():
    from deformgs import lpips
    w = lpips.weights_from_tensors(*ref.random_weights(2), "cpu")
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(ValueError, match="CPU"):
        lpips.lpips(x, x, w)
    with pytest.raises(ValueError, match="3 channels"):
        lpips.lpips(torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16), w)
    with pytest.raises(ValueError, match="16"):
        lpips.lpips(torch.rand(2, 3, 15, 16), torch.rand(2, 3, 15, 16), w)
    with pytest.raises(ValueError, match="differ in shape"):
        lpips.lpips(x, torch.rand(2, 3, 16, 17), w)


def test_image_metrics_still_rejects_lpips():
    from deformgs.image_metrics import image_metrics
    with pytest.raises(ValueError, match="unknown metrics"):
        image_metrics(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16), ("lpips",))
