"""Writes tests/golden/jpeg_ingest.npz, tests/golden/colmap_tiny/, tests/golden/colmap_tiny_txt/ and
tests/golden/colmap_tiny.npz (run by hand where a checkout of the reference and PIL exist; the tests only read
the results and never import PIL):

    python tests/golden/make_golden_colmap.py --reference /path/to/Deformable-3D-Gaussians

The goldens in the repository come from Pillow 12.2.0 with libjpeg-turbo 3.1.4. JPEG decoding is pinned to
that library's default decompressor (islow IDCT, fancy upsampling): another libjpeg (IJG 9, say) decodes the
same files to other bytes, and a regenerated jpeg_ingest.npz would then no longer be what deformgs decodes.

jpeg_ingest.npz
  cases                    the names of the decodable cases
  <case>_jpg  uint8 (n,)   the file as PIL wrote it
  <case>_rgb  uint8 (H,W,3)  np.asarray(Image.open(file))
  <case>_half float32 (3,h,w)  the reference's own PILtoTorch (utils/general_utils.py:23-29) at
                           (max(W // 2, 1), max(H // 2, 1)), for the cases of HALVED
  refusals, refuse_<name>_jpg   files that must be refused: progressive, grayscale, cmyk
  pil_version, libjpeg_turbo_version
 The cases (each a place the decoder can go wrong):
  d44x28_420 / _422 / _444   tests/png_fixtures.disc_image, quality 90: ragged against the 16x16 and 16x8 MCU
  d17x17_420, d33x19_420     odd sizes; the chroma context rows cross MCU rows
  d33x19b_420, d33x19c_420   two more 33x19 images (another frame at quality 70, noise at quality 50): with
                             d33x19_420 a group of three whose per-image block count, 36, is no multiple of 32
  n<w>x3_420, n<w>x3_422     w = 1..6 on noise: a downsampled width <= 2 takes plain doubling, 5 is the first
                             fancy width
  d1x1_420
  noise_q100_420, noise_q100_444, noise_q20_420   uniform noise: saturating IDCT outputs, coarse tables
  opt_420                    optimize=True: the file carries its own Huffman tables
  rst_blocks1_420, rst_rows1_420, rst_blocks1_444   restart intervals
  batch0..3_420              44x28 at qualities 30, 60, 85, 95: per-image tables inside one group
  exif_420                   an EXIF orientation tag (6) and an APP1 of about 20 KB

colmap_tiny/: a Colmap directory: sparse/0/{cameras,images,points3D}.bin written with struct.pack, ten 44x28
baseline JPEGs images/<n>.jpg for n in 0..7, 10, 11 (string order differs from numeric order and from the order
in images.bin), one PINHOLE and one SIMPLE_PINHOLE camera, 3..7 2D points per image, 300 points.
colmap_tiny_txt/sparse/0/*.txt: the same model as text (repr() of every float: the same float64 values).

colmap_tiny.npz: the reference's own readColmapSceneInfo (scene/dataset_readers.py:101-220) on a temporary
copy of colmap_tiny/, with eval and without: <split>_name, <split>_R, _T, _FovX, _FovY, _fid, _width, _height,
_uid for split in eval_train, eval_test, all; translate / radius (eval) and translate_all / radius_all;
points (float32), colors: the fetchPly result. scene/dataset_readers.py is imported as in
make_golden_nerfies.py, with empty stand-ins for cv2 and imageio. plyfile, which the Colmap path does call,
is stood in for by the two classes below: they write and read the binary little-endian PLY that plyfile writes
from the structured array the reference builds (the float32 / uint8 conversions are the reference's own, in
that array). half_22x14 float32 (10,3,14,22), in sorted-name order: PILtoTorch at (22, 14): the -r 2 path.
"""
import argparse
import io
import os
import shutil
import struct
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from png_fixtures import disc_image  # noqa: E402

SUB = {"444": 0, "422": 1, "420": 2}
HALVED = ("d44x28_420", "d44x28_422", "d44x28_444", "d33x19_420", "noise_q100_420", "n5x3_420", "batch2_420")
NAMES = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]
FILE_ORDER = [5, 0, 11, 3, 7, 1, 10, 2, 6, 4]  # the order of the records in images.bin


def jpeg_bytes(arr, sub, quality=90, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=quality, subsampling=SUB[sub], **kw)
    return buf.getvalue()


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def disc(w, h, t=0.3):
    return np.ascontiguousarray(disc_image(w, h, t)[:, :, :3])


def ingest_cases():
    from PIL import Image
    cases = {}
    for sub in ("420", "422", "444"):
        cases[f"d44x28_{sub}"] = jpeg_bytes(disc(44, 28), sub)
    cases["d17x17_420"] = jpeg_bytes(disc(17, 17), "420")
    cases["d33x19_420"] = jpeg_bytes(disc(33, 19), "420")
    cases["d33x19b_420"] = jpeg_bytes(disc(33, 19, 0.55), "420", quality=70)
    cases["d33x19c_420"] = jpeg_bytes(noise(33, 19, 5), "420", quality=50)
    for sub in ("420", "422"):
        for w in range(1, 7):
            cases[f"n{w}x3_{sub}"] = jpeg_bytes(noise(w, 3, 100 + w), sub)
    cases["d1x1_420"] = jpeg_bytes(disc(1, 1), "420")
    cases["noise_q100_420"] = jpeg_bytes(noise(44, 28, 1), "420", quality=100)
    cases["noise_q100_444"] = jpeg_bytes(noise(44, 28, 2), "444", quality=100)
    cases["noise_q20_420"] = jpeg_bytes(noise(44, 28, 3), "420", quality=20)
    cases["opt_420"] = jpeg_bytes(disc(44, 28, 0.6), "420", optimize=True)
    cases["rst_blocks1_420"] = jpeg_bytes(disc(44, 28, 0.7), "420", restart_marker_blocks=1)
    cases["rst_rows1_420"] = jpeg_bytes(disc(44, 28, 0.8), "420", restart_marker_rows=1)
    cases["rst_blocks1_444"] = jpeg_bytes(noise(20, 12, 4), "444", restart_marker_blocks=1)
    for k, q in enumerate((30, 60, 85, 95)):
        cases[f"batch{k}_420"] = jpeg_bytes(disc(44, 28, 0.1 + 0.2 * k), "420", quality=q)
    exif = Image.Exif()
    exif[0x0112] = 6
    exif[0x010E] = "x" * 20000
    cases["exif_420"] = jpeg_bytes(disc(44, 28, 0.9), "420", exif=exif)
    refusals = {"progressive": jpeg_bytes(disc(44, 28), "420", progressive=True)}
    buf = io.BytesIO()
    Image.fromarray(disc(44, 28)).convert("L").save(buf, "JPEG", quality=90)
    refusals["grayscale"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(disc(44, 28)).convert("CMYK").save(buf, "JPEG", quality=90)
    refusals["cmyk"] = buf.getvalue()
    return cases, refusals


def write_jpeg_ingest(pil_to_torch):
    import PIL
    from PIL import Image, features
    cases, refusals = ingest_cases()
    out = {"cases": np.array(list(cases)), "refusals": np.array(list(refusals)),
           "pil_version": np.array(PIL.__version__), "libjpeg_turbo_version": np.array(features.version("libjpeg_turbo"))}
    for name, data in cases.items():
        out[f"{name}_jpg"] = np.frombuffer(data, np.uint8)
        rgb = np.asarray(Image.open(io.BytesIO(data)))
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        out[f"{name}_rgb"] = rgb
        if name in HALVED:
            size = (max(rgb.shape[1] // 2, 1), max(rgb.shape[0] // 2, 1))
            out[f"{name}_half"] = pil_to_torch(Image.open(io.BytesIO(data)), size).numpy()
    for name, data in refusals.items():
        out[f"refuse_{name}_jpg"] = np.frombuffer(data, np.uint8)
    np.savez_compressed(os.path.join(HERE, "jpeg_ingest.npz"), **out)
    return len(out)


def orbit_qt(k, n):
    """World-to-camera rotation (as a unit quaternion w, x, y, z) and translation of a camera on a radius-4
    orbit looking at the origin."""
    az, el = 2 * np.pi * k / n, 0.3 + 0.1 * np.sin(1.7 * k)
    pos = 4.0 * np.array([np.cos(el) * np.sin(az), -np.cos(el) * np.cos(az), np.sin(el)])
    fwd = -pos / np.linalg.norm(pos)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])  # world -> camera
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    else:
        q = np.array([0.0, 1.0, 0.0, 0.0])
    q /= np.linalg.norm(q)
    return q, -R @ pos


def write_colmap_tiny(root, root_txt):
    for d in (root, root_txt):
        if os.path.isdir(d):
            shutil.rmtree(d)
    sparse, sparse_txt = os.path.join(root, "sparse", "0"), os.path.join(root_txt, "sparse", "0")
    os.makedirs(sparse)
    os.makedirs(sparse_txt)
    os.makedirs(os.path.join(root, "images"))
    rng = np.random.default_rng(20241020)
    cameras = [(1, 1, "PINHOLE", 44, 28, [40.0, 38.5, 22.0, 14.0]), (2, 0, "SIMPLE_PINHOLE", 44, 28, [41.25, 22.0, 14.0])]
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for cid, mid, _, w, h, params in cameras:
            f.write(struct.pack("<iiQQ", cid, mid, w, h) + struct.pack(f"<{len(params)}d", *params))
    with open(os.path.join(sparse_txt, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, _, model, w, h, params in cameras:
            f.write(f"{cid} {model} {w} {h} " + " ".join(repr(float(p)) for p in params) + "\n")
    records = []
    for k, n in enumerate(NAMES):
        q, t = orbit_qt(k, len(NAMES))
        pts = [(float(rng.uniform(0, 44)), float(rng.uniform(0, 28)), int(rng.integers(-1, 300)))
               for _ in range(int(rng.integers(3, 8)))]
        records.append((k + 1, q, t, 1 + k % 2, f"{n}.jpg", pts))
        with open(os.path.join(root, "images", f"{n}.jpg"), "wb") as f:
            f.write(jpeg_bytes(disc(44, 28, k / (len(NAMES) - 1)), "420" if k % 2 else "444"))
    order = [NAMES.index(n) for n in FILE_ORDER]
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for k in order:
            iid, q, t, cid, name, pts = records[k]
            f.write(struct.pack("<i7di", iid, *q, *t, cid) + name.encode() + b"\0" + struct.pack("<Q", len(pts)))
            for x, y, pid in pts:
                f.write(struct.pack("<ddq", x, y, pid))
    with open(os.path.join(sparse_txt, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for k in order:
            iid, q, t, cid, name, pts = records[k]
            f.write(f"{iid} " + " ".join(repr(float(v)) for v in list(q) + list(t)) + f" {cid} {name}\n")
            f.write(" ".join(f"{x!r} {y!r} {pid}" for x, y, pid in pts) + "\n")
    xyz = rng.normal(0.0, 0.5, (300, 3))
    rgb = rng.integers(0, 256, (300, 3))
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f, open(os.path.join(sparse_txt, "points3D.txt"), "w") as g:
        f.write(struct.pack("<Q", 300))
        g.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for i in range(300):
            err = float(rng.uniform(0, 2))
            track = [(int(rng.integers(1, 11)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(2, 5)))]
            f.write(struct.pack("<Q3d3Bd", i + 1, *xyz[i], *(int(c) for c in rgb[i]), err) + struct.pack("<Q", len(track)))
            for a, b in track:
                f.write(struct.pack("<ii", a, b))
            g.write(f"{i + 1} " + " ".join(repr(float(v)) for v in xyz[i]) + " " + " ".join(str(int(c)) for c in rgb[i]) +
                    f" {err!r} " + " ".join(f"{a} {b}" for a, b in track) + "\n")


class _PlyElement:
    def __init__(self, data, name):
        self.data, self.name = data, name

    @staticmethod
    def describe(data, name):
        return _PlyElement(data, name)

    def __getitem__(self, key):
        return self.data[key]


class _PlyData:
    """What plyfile does for one element of scalar properties, binary little endian."""
    _NAMES = {"f4": "float", "u1": "uchar"}

    def __init__(self, elements):
        self.elements = {e.name: e for e in elements}

    def __getitem__(self, name):
        return self.elements[name]

    def write(self, path):
        (el,) = self.elements.values()
        head = f"ply\nformat binary_little_endian 1.0\nelement {el.name} {len(el.data)}\n"
        head += "".join(f"property {self._NAMES[el.data.dtype[n].str[1:]]} {n}\n" for n in el.data.dtype.names)
        with open(path, "wb") as f:
            f.write((head + "end_header\n").encode("ascii"))
            f.write(el.data.astype(el.data.dtype.newbyteorder("<")).tobytes())

    @staticmethod
    def read(path):
        with open(path, "rb") as f:
            assert f.readline().strip() == b"ply" and b"binary_little_endian" in f.readline()
            name, n = f.readline().split()[1:3]
            fields = []
            while True:
                parts = f.readline().split()
                if parts[0] == b"end_header":
                    break
                fields.append((parts[2].decode(), {"float": "<f4", "uchar": "u1"}[parts[1].decode()]))
            data = np.frombuffer(f.read(), np.dtype(fields), int(n))
        return _PlyData([_PlyElement(data, name.decode())])


def import_reference_reader(reference):
    sys.path.insert(0, reference)
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    ply = types.ModuleType("plyfile")
    ply.PlyData, ply.PlyElement = _PlyData, _PlyElement
    sys.modules["plyfile"] = ply
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(reference, "scene")]
    sys.modules["scene"] = pkg
    from utils.graphics_utils import BasicPointCloud
    gm = types.ModuleType("scene.gaussian_model")
    gm.BasicPointCloud = BasicPointCloud
    sys.modules["scene.gaussian_model"] = gm
    import scene.dataset_readers as readers
    return readers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of preacherwhite/Deformable-3D-Gaussians")
    args = ap.parse_args()
    readers = import_reference_reader(os.path.abspath(args.reference))
    from PIL import Image
    from utils.general_utils import PILtoTorch  # the reference's own function
    n = write_jpeg_ingest(PILtoTorch)
    root, root_txt = os.path.join(HERE, "colmap_tiny"), os.path.join(HERE, "colmap_tiny_txt")
    write_colmap_tiny(root, root_txt)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "colmap_tiny")
        shutil.copytree(root, copy)
        for ev in (True, False):
            info = readers.readColmapSceneInfo(copy, None, ev)
            sets = (("eval_train", info.train_cameras), ("eval_test", info.test_cameras)) if ev else (("all", info.train_cameras),)
            for key, cams in sets:
                out[f"{key}_name"] = np.array([c.image_name for c in cams])
                out[f"{key}_R"] = np.stack([c.R for c in cams])
                out[f"{key}_T"] = np.stack([c.T for c in cams])
                for field in ("FovX", "FovY", "fid"):
                    out[f"{key}_{field}"] = np.array([getattr(c, field) for c in cams], np.float64)
                for field in ("width", "height", "uid"):
                    out[f"{key}_{field}"] = np.array([getattr(c, field) for c in cams], np.int64)
            suffix = "" if ev else "_all"
            out[f"translate{suffix}"] = np.asarray(info.nerf_normalization["translate"])
            out[f"radius{suffix}"] = np.asarray(info.nerf_normalization["radius"])
        out["points"] = np.asarray(info.point_cloud.points)
        out["colors"] = np.asarray(info.point_cloud.colors)
    out["half_22x14"] = np.stack([PILtoTorch(Image.open(os.path.join(root, "images", f"{n}.jpg")), (22, 14)).numpy()
                                  for n in out["all_name"]])
    np.savez_compressed(os.path.join(HERE, "colmap_tiny.npz"), **out)
    print("wrote jpeg_ingest.npz:", n, "arrays; colmap_tiny/, colmap_tiny_txt/, colmap_tiny.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
