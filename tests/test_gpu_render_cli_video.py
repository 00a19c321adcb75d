"""GPU: render_cli --video mjpeg on the synthetic scene (2000 Gaussians, 50 x 36: ragged against the MCUs of every
sampling): renders/video.avi holds the PNG frames as the JPEG files the encoder's numpy restatement makes of them, at
the reference's frame rate; without the option nothing changes; mode render writes no video."""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ARGS = ["--synthetic", "2000", "--res", "50", "36", "--skip_train", "--view_index", "1"]


def _listing(base):
    out = {}
    for root, _, files in os.walk(base):
        for n in files:
            with open(os.path.join(root, n), "rb") as f:
                out[os.path.relpath(os.path.join(root, n), base)] = f.read()
    return out


def test_time_mode_video_holds_the_png_frames(tmp_path):
    import jpeg_encode_ref as ref
    from deformgs import jpeg, mjpeg, render_cli
    from deformgs.png import read_png
    m = str(tmp_path / "model")
    # --chunk 3 of 7 frames: the video is put together from more than one encoder call, the last one short
    (out,) = render_cli.main(["-m", m, *ARGS, "--mode", "time", "--frames", "7", "--chunk", "3", "--video", "mjpeg"])
    pngs = sorted(n for n in os.listdir(os.path.join(out, "renders")) if n.endswith(".png"))
    assert pngs == [f"{i:05d}.png" for i in range(7)]
    assert sorted(os.listdir(os.path.join(out, "renders"))) == pngs + ["video.avi"]
    info, frames = mjpeg.read_avi(os.path.join(out, "renders", "video.avi"))
    assert (info["frames"], info["fps"], info["width"], info["height"]) == (7, 30, 50, 36)
    assert len(frames) == 7
    for n, data in zip(pngs, frames):
        want = ref.encode(read_png(os.path.join(out, "renders", n)), 90, "4:2:0")
        assert data == want, n
        assert np.array_equal(jpeg.decode_jpeg(data), jpeg.decode_jpeg(want)), n


def test_pose_mode_is_60_fps_and_the_options_reach_the_encoder(tmp_path):
    import jpeg_encode_ref as ref
    from deformgs import jpeg, mjpeg, render_cli
    from deformgs.png import read_png
    m = str(tmp_path / "model")
    (out,) = render_cli.main(["-m", m, *ARGS, "--mode", "pose", "--frames", "4", "--video", "mjpeg", "--video_quality", "75",
                              "--video_subsampling", "4:4:4"])
    info, frames = mjpeg.read_avi(os.path.join(out, "renders", "video.avi"))
    assert (info["frames"], info["fps"]) == (4, 60)
    for i, data in enumerate(frames):
        want = ref.encode(read_png(os.path.join(out, "renders", f"{i:05d}.png")), 75, "4:4:4")
        assert np.array_equal(jpeg.decode_jpeg(data), jpeg.decode_jpeg(want)), i


def test_without_the_option_nothing_changes(tmp_path):
    """The same command without --video, with --video none and with --video mjpeg: the same files with the same
    bytes, but for video.avi in the last."""
    from deformgs import render_cli
    runs = {}
    for key, extra in (("plain", []), ("none", ["--video", "none"]), ("mjpeg", ["--video", "mjpeg"])):
        (out,) = render_cli.main(["-m", str(tmp_path / key), *ARGS, "--mode", "time", "--frames", "4", *extra])
        runs[key] = _listing(out)
    assert sorted(runs["plain"]) == sorted([f"{sub}/{i:05d}.png" for sub in ("renders", "depth") for i in range(4)])
    assert runs["none"] == runs["plain"]
    video = runs["mjpeg"].pop(os.path.join("renders", "video.avi"))
    assert video[:4] == b"RIFF" and runs["mjpeg"] == runs["plain"]


def test_mode_render_writes_no_video(tmp_path):
    from deformgs import render_cli
    (out,) = render_cli.main(["-m", str(tmp_path / "model"), *ARGS, "--mode", "render", "--video", "mjpeg"])
    names = set(_listing(out))
    assert names and not any(n.endswith(".avi") for n in names)
    assert all(n.endswith(".png") for n in names)


def test_render_set_refuses_an_unknown_video_choice():
    from deformgs import render_cli
    with pytest.raises(ValueError, match="video"):
        render_cli.render_set("unused", "test", 0, "time", [], None, None, None, False, video="mp4")
