"""CPU: the stdlib PNG writer / reader of the render path (deformgs/png.py) and the C layout of the
dgs_render_frames argument structs."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 1, 3), (72, 100, 3), (7, 13, 3), (1, 1), (9, 1), (72, 100), (3, 17)])
def test_png_round_trip(shape, tmp_path):
    from deformgs.png import decode_png, encode_png, read_png, write_png
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(decode_png(encode_png(img)), img)
    p = tmp_path / "a.png"
    write_png(str(p), img)
    back = read_png(str(p))
    assert back.dtype == np.uint8 and back.shape == img.shape and np.array_equal(back, img)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _filtered_png(img, ft):
    """A PNG of `img` (H, W, 3) whose every row uses filter type ft, built by hand from the PNG
    specification's filter definitions (bytes to the left / above / above-left, 0 outside)."""
    h, w, _ = img.shape
    flat = img.reshape(h, -1).astype(int)
    raw = bytearray()
    for y in range(h):
        raw.append(ft)
        for i in range(w * 3):
            a = flat[y, i - 3] if i >= 3 else 0
            b = flat[y - 1, i] if y > 0 else 0
            c = flat[y - 1, i - 3] if (y > 0 and i >= 3) else 0
            pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[ft]
            raw.append((flat[y, i] - pred) & 255)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b""))


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4])
def test_png_reader_filter_types(ft):
    from deformgs.png import decode_png
    img = np.random.default_rng(ft).integers(0, 256, (6, 9, 3), dtype=np.uint8)
    assert np.array_equal(decode_png(_filtered_png(img, ft)), img)


def test_png_reader_refuses_what_it_cannot_decode():
    from deformgs.png import decode_png, encode_png
    with pytest.raises(ValueError):
        decode_png(b"not a png")
    good = encode_png(np.zeros((2, 2), np.uint8))
    sixteen = good.replace(struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0), struct.pack(">IIBBBBB", 2, 2, 16, 0, 0, 0, 0))
    with pytest.raises(ValueError, match="unsupported"):
        decode_png(sixteen)
    with pytest.raises(ValueError):
        encode_png(np.zeros((2, 2, 4), np.uint8))


STRUCTS = [("dgs_frame", "Frame"), ("dgs_render_frames_args", "RenderFramesArgs")]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_render_frames_structs_match_the_header(tmp_path):
    """sizeof and every offsetof of the ctypes mirrors equal the C compiler's, and the fields come in the
    header's order (as tests/test_struct_layout.py checks the other argument structs)."""
    from deformgs import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "dgs.h"', "int main(void) {"]
    for cname, cls in STRUCTS:
        C = getattr(_lib, cls)
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f, _ in C._fields_:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if line.strip():
            s, f, v = line.split()
            got[(s, f)] = int(v)
    for cname, cls in STRUCTS:
        C = getattr(_lib, cls)
        assert got[(cname, "sizeof")] == ctypes.sizeof(C), cname
        offs = [getattr(C, f).offset for f, _ in C._fields_]
        assert offs == sorted(offs)
        for f, _ in C._fields_:
            assert got[(cname, f)] == getattr(C, f).offset, (cname, f)


@pytest.mark.parametrize("mode", ["render", "time", "view", "all", "pose", "original"])
def test_frame_lists_match_the_golden_paths(mode, golden_dir):
    """Every mode's (R, T, time) list against tests/golden/render_paths.npz (recorded from the reference's
    pose_spherical / render_wander_path and the loops of its render script on four sample views), to 1e-6."""
    import types
    from deformgs.camera_paths import DEFAULT_FRAMES, frame_list
    g = np.load(os.path.join(golden_dir, "render_paths.npz"))
    views = [types.SimpleNamespace(R=g["cams_R"][k], T=g["cams_T"][k], fid=float(g["cams_fid"][k]), FoVy=float(g["FoVy"]),
                                   image_height=int(g["image_height"])) for k in range(len(g["cams_R"]))]
    before = [v.R.copy() for v in views]
    fl = frame_list(mode, views, view_index=int(g["view_index"]))
    assert len(fl) == len(g[mode + "_t"])
    if mode not in ("render", "original"):
        assert len(fl) == DEFAULT_FRAMES[mode]
    assert np.abs(np.stack([f[0] for f in fl]) - g[mode + "_R"]).max() <= 1e-6
    assert np.abs(np.stack([f[1] for f in fl]) - g[mode + "_T"]).max() <= 1e-6
    assert np.abs(np.array([f[2] for f in fl]) - g[mode + "_t"]).max() <= 1e-6
    assert all(np.array_equal(v.R, b) for v, b in zip(views, before))  # the views are left as they were
    short = frame_list(mode, views, view_index=1, frames=5)
    assert len(short) == (len(views) if mode == "render" else 4 if mode == "original" else 5)


def test_metrics_json_layout(tmp_path):
    """results.json / per_view.json in the reference's layout, on two tiny images with a torch-CPU SSIM
    stand-in injected (the fused SSIM kernel needs a GPU)."""
    import json
    import torch
    from deformgs import loss, metrics
    from deformgs.png import write_png
    rng = np.random.default_rng(0)
    base = tmp_path / "model" / "test" / "ours_7"
    imgs = {}
    for sub in ("renders", "gt"):
        (base / sub).mkdir(parents=True)
        for k in range(2):
            a = rng.integers(0, 256, (12, 14, 3), dtype=np.uint8)
            imgs[(sub, k)] = a
            write_png(str(base / sub / f"{k:05d}.png"), a)
    (tmp_path / "model" / "test" / "interpolate_7").mkdir()  # not a method directory: ignored
    stand_in = lambda a, b: loss.ssim(a, b)  # noqa: E731
    m = str(tmp_path / "model")
    res = metrics.evaluate([m], ssim_fn=stand_in, device="cpu")
    with open(os.path.join(m, "results.json")) as f:
        results = json.load(f)
    with open(os.path.join(m, "per_view.json")) as f:
        per_view = json.load(f)
    assert results == res[m] and list(results) == ["ours_7"]
    assert set(results["ours_7"]) == {"SSIM", "PSNR", "LPIPS"} and results["ours_7"]["LPIPS"] is None
    names = ["00000.png", "00001.png"]
    for metric in ("SSIM", "PSNR", "LPIPS"):
        assert list(per_view["ours_7"][metric]) == names
    t = lambda a: (torch.from_numpy(a).permute(2, 0, 1).contiguous().float() / 255.0).unsqueeze(0)  # noqa: E731
    ps = [float(loss.psnr(t(imgs[("renders", k)]), t(imgs[("gt", k)]))) for k in range(2)]
    ss = [float(loss.ssim(t(imgs[("renders", k)]), t(imgs[("gt", k)]))) for k in range(2)]
    assert results["ours_7"]["PSNR"] == torch.tensor(ps).mean().item()
    assert results["ours_7"]["SSIM"] == torch.tensor(ss).mean().item()
    assert [per_view["ours_7"]["PSNR"][n] for n in names] == torch.tensor(ps).tolist()
    assert all(v is None for v in per_view["ours_7"]["LPIPS"].values())
