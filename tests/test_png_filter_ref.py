"""CPU: deformgs.png.filter_rows, the numpy restatement of the device row filter (csrc/png_encode.hip
k_png_filter): unfilter inverts it, and its choice per row is the brute-force argmin of the sum of |residual as
int8| with ties toward the lower type."""
import numpy as np
import pytest

from deformgs import png
from png_fixtures import disc_image, filtered_variants


def _images():
    rng = np.random.default_rng(11)
    out = {}
    for h, w in ((1, 1), (1, 7), (7, 1), (9, 13), (32, 17)):
        out[f"noise_rgb_{h}x{w}"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out[f"noise_grey_{h}x{w}"] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    smooth = disc_image(45, 31, 0.3)
    out["smooth_rgb"] = np.ascontiguousarray(smooth[:, :, :3])
    out["smooth_grey"] = np.ascontiguousarray(smooth[:, :, 1])
    out["ramp_grey"] = (np.add.outer(np.arange(20), 3 * np.arange(50)) & 255).astype(np.uint8)
    return out


IMAGES = _images()


def _brute_types(img):
    px = img if img.ndim == 3 else img[:, :, None]
    v = filtered_variants(px).astype(np.int64)  # (5, H, W*C)
    types = []
    for y in range(px.shape[0]):
        costs = [int(sum(b if b < 128 else 256 - b for b in v[k, y].tolist())) for k in range(5)]
        types.append(min(range(5), key=lambda k: (costs[k], k)))
    return types, v


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_unfilter_inverts_filter_rows(name):
    img = IMAGES[name]
    h, w = img.shape[:2]
    c = 3 if img.ndim == 3 else 1
    raw = png.filter_rows(img)
    assert isinstance(raw, bytes) and len(raw) == h * (1 + w * c)
    back = png.unfilter(raw, w, h, c)
    assert np.array_equal(back if c == 3 else back[:, :, 0], img)


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_types_are_the_brute_force_argmin(name):
    img = IMAGES[name]
    h, w = img.shape[:2]
    c = 3 if img.ndim == 3 else 1
    lines = np.frombuffer(png.filter_rows(img), np.uint8).reshape(h, 1 + w * c)
    types, v = _brute_types(img)
    assert lines[:, 0].tolist() == types
    for y in range(h):
        assert np.array_equal(lines[y, 1:], v[types[y], y].astype(np.uint8))


def test_ties_go_to_the_lower_type():
    """Row 0 of any image: Up equals None and Paeth equals Sub (zero row above), so every row-0 choice is a tie
    broken downward. A black image ties all five at cost 0 -> None. Rows that repeat the row above tie Up (2) with
    Paeth (4) at cost 0 -> Up."""
    black = np.zeros((3, 5, 3), np.uint8)
    assert np.frombuffer(png.filter_rows(black), np.uint8).reshape(3, 16)[:, 0].tolist() == [0, 0, 0]
    rng = np.random.default_rng(5)
    row = rng.integers(1, 256, (1, 40), dtype=np.uint8)
    rep = np.repeat(row, 4, axis=0)
    types, _ = _brute_types(rep)
    got = np.frombuffer(png.filter_rows(rep), np.uint8).reshape(4, 41)[:, 0].tolist()
    assert got == types and got[1:] == [2, 2, 2] and got[0] in (0, 1)
    # tiny images of small values tie often below row 0 too: every pair of types that ties for the minimum there
    seen = set()
    for _ in range(400):
        img = rng.integers(0, 4, (3, 4), dtype=np.uint8)
        types, v = _brute_types(img)
        cost = np.where(v < 128, v, 256 - v).sum(axis=2)
        assert np.frombuffer(png.filter_rows(img), np.uint8).reshape(3, 5)[:, 0].tolist() == types
        for y in (1, 2):
            tied = np.nonzero(cost[:, y] == cost[:, y].min())[0]
            if len(tied) > 1:
                assert types[y] == tied[0]
                seen.add((int(tied[0]), int(tied[1])))
    assert len(seen) >= 6, seen


def test_refuses_what_encode_png_refuses():
    for bad in (np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4), np.float32), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            png.filter_rows(bad)
