"""GPU: render_cli --png gpu against --png zlib on the synthetic scene: every file of renders/, depth/ and gt/
decodes to the same array under both writers, and metrics scores both model directories identically."""
import json
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


def test_both_writers_give_the_same_images_and_scores(tmp_path):
    from deformgs import metrics, render_cli
    from deformgs.png import read_png
    done = {}
    for writer in ("zlib", "gpu"):
        m = str(tmp_path / writer)
        # --chunk 3: the device writer goes through more than one chunk, the last one short
        (done[writer],) = render_cli.main(["-m", m, "--synthetic", "2000", "--res", "64", "64", "--skip_train",
                                           "--chunk", "3", "--png", writer])
    total = 0
    for sub in ("renders", "depth", "gt"):
        names = sorted(os.listdir(os.path.join(done["zlib"], sub)))
        assert names and names == sorted(os.listdir(os.path.join(done["gpu"], sub))), sub
        for n in names:
            a, b = read_png(os.path.join(done["zlib"], sub, n)), read_png(os.path.join(done["gpu"], sub, n))
            assert a.shape == b.shape == ((64, 64) if sub == "depth" else (64, 64, 3)) and np.array_equal(a, b), (sub, n)
        total += len(names)
    assert total >= 3
    metrics.main(["-m", str(tmp_path / "zlib"), str(tmp_path / "gpu")])
    res = []
    for writer in ("zlib", "gpu"):
        with open(os.path.join(str(tmp_path / writer), "results.json")) as f:
            res.append(json.load(f))
    assert res[0] == res[1] and res[0]


def test_metrics_passes_the_writer_through(tmp_path):
    from deformgs import metrics
    from deformgs.png import inflate_png
    m = str(tmp_path / "model")
    metrics.main(["-m", m, "--synthetic", "2000", "--res", "64", "64", "--png", "gpu"])
    d = os.path.join(m, "test", "ours_0", "renders")
    with open(os.path.join(d, sorted(os.listdir(d))[0]), "rb") as f:
        _, h, _, raw = inflate_png(f.read())
    # the host writer filters every row with type 0; the device writer's adaptive choice does not on a rendered frame
    assert any(raw[y * (1 + 64 * 3)] != 0 for y in range(h))
    assert os.path.exists(os.path.join(m, "results.json"))
