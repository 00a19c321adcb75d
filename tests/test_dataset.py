"""CPU: the PNG reader's RGBA / grey + alpha decode, the numpy ingest path against the committed fixture
(tests/golden/dataset_ingest.npz: composite by the reader's float64 formula, resize by the reference's own
PILtoTorch) and against a live PIL where one is installed, malformed input, the D-NeRF directory reader
on tests/golden/dnerf_tiny, and the training script's parser."""
import json
import math
import os

import numpy as np
import pytest

from png_fixtures import encode_png_filtered, filter_scanlines, png_from_scanlines

from deformgs import ingest, png
from deformgs.cameras import blender_c2w_to_RT, focal2fov, fov2focal, getWorld2View2

RESIZE_CASES = [((19, 13), (10, 6)), ((32, 32), (16, 16)), ((24, 40), (12, 20)), ((33, 17), (8, 4)),
                ((16, 16), (16, 8)), ((19, 13), (19, 13))]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "dataset_ingest.npz")))


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return os.path.join(golden_dir, "dnerf_tiny")


def _types(kind, h, rng):
    if kind == "cycle":
        return [y % 5 for y in range(h)]
    if kind == "random":
        return rng.integers(0, 5, h).tolist()
    return [kind] * h


# ---- decode_png ----
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, "cycle", "random"])
@pytest.mark.parametrize("size", [(1, 1), (1, 7), (5, 1), (13, 9)])
def test_decode_round_trip(channels, kind, size):
    w, h = size
    rng = np.random.default_rng(w * 100 + h * 10 + channels)
    px = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    got = png.decode_png(encode_png_filtered(px, _types(kind, h, rng)))
    assert got.dtype == np.uint8
    assert got.shape == ((h, w) if channels == 1 else (h, w, channels))
    assert np.array_equal(got.reshape(h, w, channels), px)


def test_existing_rgb_and_grey_behaviour_unchanged():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (6, 5), dtype=np.uint8)
    assert np.array_equal(png.decode_png(png.encode_png(rgb)), rgb)
    assert np.array_equal(png.decode_png(png.encode_png(grey)), grey)
    assert png.decode_png(png.encode_png(grey)).shape == (6, 5)


def test_inflate_png_returns_filtered_scanlines():
    rng = np.random.default_rng(4)
    px = rng.integers(0, 256, (7, 3, 4), dtype=np.uint8)
    types = [4, 3, 2, 1, 0, 4, 3]
    w, h, ch, raw = png.inflate_png(encode_png_filtered(px, types))
    assert (w, h, ch) == (3, 7, 4) and raw == filter_scanlines(px, types)
    assert np.array_equal(png.unfilter(raw, w, h, ch), px)


# ---- numpy ingest path against the fixture ----
def test_composite_matches_fixture(fx):
    keys = [k for k in fx if k.startswith("rgba_")]
    assert len(keys) == 5
    for k in keys:
        for bg, white in (("black", False), ("white", True)):
            got = ingest.composite_numpy(fx[k], white)
            assert np.array_equal(got, fx[k.replace("rgba_", f"comp_{bg}_")]), (k, bg)


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
@pytest.mark.parametrize("white", [False, True])
def test_ingest_numpy_matches_fixture(fx, case, white):
    (W, H), (w, h) = case
    bg = "white" if white else "black"
    data = encode_png_filtered(fx[f"rgba_{W}x{H}"], [y % 5 for y in range(H)])
    got, got8 = ingest.ingest_images([data], white, size=(w, h), device="cpu", return_uint8=True)
    want = fx[f"resized_{bg}_{W}x{H}_{w}x{h}"]
    assert got.shape == (1, 3, h, w) and got.dtype.is_floating_point and got8.shape == (1, h, w, 3)
    assert np.array_equal(got[0].numpy(), want)
    assert np.array_equal(got8[0].numpy().transpose(2, 0, 1).astype(np.float32) / np.float32(255), want)


@pytest.mark.parametrize("target", [(10, 6), (19, 13)])
def test_ingest_numpy_rgb_skips_composite(fx, target):
    data = encode_png_filtered(fx["rgb_19x13"], [4] * 13)
    for white in (False, True):
        got = ingest.ingest_images([data], white, size=target, device="cpu")
        assert np.array_equal(got[0].numpy(), fx[f"resized_rgb_19x13_{target[0]}x{target[1]}"])


def test_ingest_groups_keep_input_order(fx):
    a, b = fx["rgba_19x13"], fx["rgb_19x13"]
    items = [encode_png_filtered(a, [1] * 13), encode_png_filtered(b, [2] * 13), encode_png_filtered(a[::-1].copy(), [3] * 13)]
    got = ingest.ingest_images(items, False, device="cpu")
    assert got.shape == (3, 3, 13, 19)
    assert np.array_equal(got[1].numpy(), b.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    assert np.array_equal(got[2].numpy(), got[0].numpy()[:, ::-1])
    with pytest.raises(ValueError):
        ingest.ingest_images(items + [encode_png_filtered(fx["rgba_16x16"], [0] * 16)], False, device="cpu")


@pytest.mark.parametrize("case", RESIZE_CASES + [((37, 21), (9, 21)), ((40, 10), (10, 3))],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
def test_resize_numpy_matches_live_pil(case):
    Image = pytest.importorskip("PIL.Image")
    (W, H), (w, h) = case
    a = np.random.default_rng(W * H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(ingest.resize_numpy(a, (w, h)), np.array(Image.fromarray(a, "RGB").resize((w, h))))


# ---- malformed input ----
def test_malformed_input_raises_value_error():
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (4, 3, 4), dtype=np.uint8)
    good = filter_scanlines(px, [0, 1, 2, 3])
    bad_filter = bytearray(good)
    bad_filter[2 * 13] = 5
    cases = {
        "filter byte 5": png_from_scanlines(3, 4, 4, bytes(bad_filter)),
        "short stream": png_from_scanlines(3, 4, 4, good[:-1]),
        "16 bit": png_from_scanlines(3, 4, 4, good + good, depth=16),
        "interlaced": png_from_scanlines(3, 4, 4, good, interlace=1),
    }
    for name, data in cases.items():
        with pytest.raises(ValueError):
            png.decode_png(data)
        with pytest.raises(ValueError):
            ingest.ingest_images([data], False, device="cpu")
    with pytest.raises(ValueError):
        ingest.validate_scanlines(bytes(bad_filter), 3, 4, 4)
    with pytest.raises(ValueError, match="RGBA"):
        png.decode_png(cases["16 bit"])


# ---- the directory reader ----
def _frames(tiny, name):
    with open(os.path.join(tiny, f"transforms_{name}.json")) as f:
        return json.load(f)


def test_read_nerf_synthetic_cameras(tiny):
    from deformgs import dataset
    info = dataset.read_nerf_synthetic(tiny, False, True, init_points=500)
    assert len(info.train_cameras) == 6 and len(info.test_cameras) == 2
    merged = dataset.read_nerf_synthetic(tiny, False, False, init_points=500)
    assert len(merged.train_cameras) == 8 and len(merged.test_cameras) == 0
    assert [c.image_name for c in merged.train_cameras[6:]] == ["r_000", "r_001"]
    meta = _frames(tiny, "train")
    fovx = meta["camera_angle_x"]
    for cam, fr in zip(info.train_cameras, meta["frames"]):
        m = np.linalg.inv(np.array(fr["transform_matrix"]))
        R = -np.transpose(m[:3, :3])
        R[:, 0] = -R[:, 0]
        assert np.allclose(cam.R, R, atol=1e-12) and np.allclose(cam.T, -m[:3, 3], atol=1e-12)
        assert np.array_equal(cam.R, blender_c2w_to_RT(np.array(fr["transform_matrix"]))[0])
        # the reference's naming swap: FovY is camera_angle_x, FovX is derived from it
        assert cam.FovY == fovx and cam.FovX == focal2fov(fov2focal(fovx, 32), 32)
        assert cam.fid == fr["time"] and (cam.width, cam.height) == (32, 32)
    assert [c.fid for c in info.test_cameras] == [fr["time"] for fr in _frames(tiny, "test")["frames"]]
    # getNerfppNorm: 1.1 x the largest distance of a camera centre from their mean; translate = -mean
    centres = np.stack([np.linalg.inv(getWorld2View2(c.R, c.T))[:3, 3] for c in info.train_cameras])
    radius = 1.1 * np.max(np.linalg.norm(centres - centres.mean(0), axis=1))
    assert math.isclose(info.nerf_normalization["radius"], radius, rel_tol=1e-6)
    assert np.allclose(info.nerf_normalization["translate"], -centres.mean(0), atol=1e-6)
    assert 0.5 < radius < 10.0


def test_target_resolution_rules():
    from deformgs.dataset import target_resolution
    assert target_resolution(19, 13, 1) == (19, 13)
    assert target_resolution(19, 13, 2) == (10, 6)  # round(9.5) = 10, round(6.5) = 6: halves go to even
    assert target_resolution(19, 13, 4) == (5, 3)
    assert target_resolution(19, 13, 8) == (2, 2)
    assert target_resolution(19, 13, -1) == (19, 13)
    assert target_resolution(3200, 1600, -1) == (1600, 800)
    assert target_resolution(800, 800, 20) == (20, 20)
    assert target_resolution(19, 13, 20) == (int(19 / (19 / 20)), int(13 / (19 / 20)))
    assert target_resolution(800, 800, 2) == (400, 400)


def _tree(root):
    return sorted((os.path.relpath(os.path.join(d, f), root), os.path.getsize(os.path.join(d, f)))
                  for d, _, fs in os.walk(root) for f in fs)


def test_seeded_point_cloud_and_read_only_source(tiny, tmp_path):
    from deformgs import dataset
    before = _tree(tiny)
    model = str(tmp_path / "model")
    info = dataset.read_nerf_synthetic(tiny, False, True, init_points=700, model_path=model)
    pts, col = np.asarray(info.point_cloud.points), np.asarray(info.point_cloud.colors)
    assert pts.shape == (700, 3) and col.shape == (700, 3)
    assert pts.min() >= -1.3 and pts.max() <= 1.3 and pts.std() > 0.5
    # SH2RGB(U[0, 1) / 255) = 0.5 + C0 * tiny: 127 or 128 of 255 after the file's 8 bits
    assert set(np.unique(np.round(col * 255).astype(int))) <= {127, 128}
    assert info.ply_path == os.path.join(model, "input.ply") and os.path.isfile(info.ply_path)
    again = dataset.read_nerf_synthetic(tiny, False, True, init_points=700)
    assert np.array_equal(np.asarray(again.point_cloud.points), pts)  # same seed, same cloud; float32 as in the file
    assert np.array_equal(np.asarray(again.point_cloud.colors), col)
    assert dataset.read_nerf_synthetic(tiny, False, True).point_cloud.points.shape == (100_000, 3)
    assert _tree(tiny) == before  # nothing is written under SOURCE
    # a dataset that brings its own points3d.ply is read from there
    src = tmp_path / "src"
    os.makedirs(src / "train")
    os.makedirs(src / "test")
    for name in ("train", "test"):
        meta = _frames(tiny, name)
        (src / f"transforms_{name}.json").write_text(json.dumps(meta))
        for fr in meta["frames"]:
            with open(os.path.join(tiny, fr["file_path"] + ".png"), "rb") as f:
                (src / (fr["file_path"] + ".png")).write_bytes(f.read())
    xyz = np.random.default_rng(1).uniform(-1, 1, (9, 3))
    dataset.store_ply(str(src / "points3d.ply"), xyz, np.full((9, 3), 200.7))
    own = dataset.read_nerf_synthetic(str(src), False, True)
    assert np.array_equal(own.point_cloud.points, xyz.astype(np.float32))
    assert np.allclose(own.point_cloud.colors, 200 / 255.0)


def test_camera_json_fields(tiny):
    from deformgs import dataset
    cam = dataset.read_nerf_synthetic(tiny, False, True, init_points=10).train_cameras[2]
    entry = dataset.camera_to_json(7, cam)
    assert set(entry) == {"id", "img_name", "width", "height", "position", "rotation", "fy", "fx"}
    assert entry["id"] == 7 and entry["img_name"] == "r_002" and entry["width"] == 32
    c2w = np.array(_frames(tiny, "train")["frames"][2]["transform_matrix"])
    assert np.allclose(entry["position"], c2w[:3, 3], atol=1e-9)
    json.dumps(entry)


# ---- the training script's parser ----
def test_train_parser_keeps_synthetic_defaults():
    from deformgs.train import build_parser
    a = build_parser().parse_args([])
    assert (a.n, a.res, a.iterations, a.warm_up, a.densify_from, a.densify_interval, a.opacity_reset) == (
        55_000, 800, 3000, None, None, None, None)
    assert (a.sequence_length, a.non_blender, a.six_dof, a.test_every, a.no_deferred) == (30, False, False, 0, False)
    assert a.source_path == "" and a.model_path == "" and not a.eval and a.resolution == -1
    b = build_parser().parse_args(["--n", "100", "--res", "64", "--iterations", "7", "--warm-up", "3", "--non-blender",
                                   "--6dof", "--test-every", "5", "--no-deferred"])
    assert (b.n, b.res, b.iterations, b.warm_up, b.non_blender, b.six_dof, b.test_every, b.no_deferred) == (
        100, 64, 7, 3, True, True, 5, True)
    c = build_parser().parse_args(["-s", "S", "-m", "M", "--eval", "-r", "2", "--white_background", "--init_points", "9",
                                   "--save_iterations", "5", "9", "--test_iterations", "4", "--is_6dof"])
    assert (c.source_path, c.model_path, c.eval, c.resolution, c.white_background, c.init_points) == (
        "S", "M", True, 2, True, 9)
    assert c.save_iterations == [5, 9] and c.test_iterations == [4] and c.is_6dof
