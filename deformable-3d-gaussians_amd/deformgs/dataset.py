"""Dataset directories: the counterpart of scene.Scene with the Colmap reader readColmapSceneInfo (a monocular
capture through convert.py), the D-NeRF (Blender-style) reader readNerfSyntheticInfo and the Nerfies-format
reader readNerfiesInfo (NeRF-DS, HyperNeRF vrig / interp / misc).

Mirrors (file:line in the reference):
  scene/dataset_readers.py:223-266  readCamerasFromTransforms: R / T from transform_matrix, fid = frame["time"],
                                    FovY = camera_angle_x and FovX from it (the names are swapped there, and
                                    the swap is kept); transforms_frames parses the file for this reader and
                                    for the render script's (deformgs/render_cli.read_transforms)
  scene/dataset_readers.py:269-306  readNerfSyntheticInfo: test merged into train unless eval; getNerfppNorm;
                                    points3d.ply or 100 000 random points in [-1.3, 1.3]^3
  scene/dataset_readers.py:398-473  readNerfiesCameras: scene.json / metadata.json / dataset.json, the split rule
                                    keyed on the name of SOURCE's parent directory, fid = time_id / max time_id,
                                    one camera/<id>.json per view, rgb/<int(1/ratio)>x/<id>.png
  scene/dataset_readers.py:476-509  readNerfiesInfo: the first train_num cameras train and the rest test with
                                    eval; points3d.ply or points.npy as (xyz - center) * scale
  utils/camera_utils.py:92-112      camera_nerfies_from_JSON: focal_length * ratio, the old `tangential` key
  scene/colmap_loader.py            the binary and text readers of sparse/0/{cameras,images,points3D}, qvec2rotmat
  scene/dataset_readers.py:101-141  readColmapCameras: R = qvec2rotmat(q)^T, T = tvec, the fields of view from the
                                    focal length(s) of a SIMPLE_PINHOLE / PINHOLE camera, the image looked up by
                                    base name, fid = int(image_name) / (number of images - 1)
  scene/dataset_readers.py:172-220  readColmapSceneInfo: cameras sorted by name as strings, every 8th the test
                                    set with eval; points3D.ply, else points3D.bin / .txt converted
  scene/dataset_readers.py:77-98    getNerfppNorm: translate = -mean camera centre, radius = 1.1 x largest
                                    distance from it
  utils/camera_utils.py:21-44       loadCam's resolution rule (target_resolution)
  utils/camera_utils.py:69-89       camera_to_JSON
  scene/__init__.py:23-112          Scene: the format dispatch, input.ply, cameras.json, the camera lists,
                                    create_from_pcd

The images go through deformgs/ingest.py (HIP unfilter + composite + resize on a GPU device), one batch per
camera set; every camera's original_image is a view into that batch. The Nerfies reader needs only what the
reference's needs: JSON, points.npy and 8-bit RGB PNGs, whose size comes from the file header (png_size). A
Colmap directory's images are baseline JPEG (or RGB PNG) files: deformgs/ingest.py decodes both.

Deviation: the reference writes a generated or converted point cloud into the dataset directory (points3d.ply,
sparse/0/points3D.ply). Here SOURCE is read only; the cloud is written as MODEL/input.ply, where the reference
copies it anyway, and a later run builds the same cloud again (the colours from a seeded generator).

Out of scope: the DTU reader (it needs cv2 / imageio behaviour), the plenoptic and Dynamic-360 readers;
gt_alpha_mask (an RGBA image in a Colmap directory is refused) and load2gpu_on_the_fly. Scene names such a
directory in its ValueError.
"""
import json
import os
import struct
from argparse import Namespace
from collections import namedtuple

import numpy as np
import torch

from .cameras import Camera, blender_c2w_to_RT, focal2fov, fov2focal, getWorld2View2
from .ingest import image_header, ingest_images
from .sh import C0

CameraInfo = namedtuple("CameraInfo", "uid R T FovY FovX image_path image_name width height fid")
SceneInfo = namedtuple("SceneInfo", "point_cloud train_cameras test_cameras nerf_normalization ply_path")
BasicPointCloud = namedtuple("BasicPointCloud", "points colors normals")

_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1",
              "char": "i1", "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def _header(path):
    """ingest.image_header of a file: (format, width, height, PNG colour type) from its first 26 bytes."""
    with open(path, "rb") as f:
        return image_header(f.read(26))


def png_size(path):
    """(width, height) from the IHDR of a PNG file (no decode)."""
    fmt, width, height, _ = _header(path)
    if fmt != "png" or width is None:
        raise ValueError(f"{path}: not a PNG file")
    return width, height


def jpeg_size(path):
    """(width, height) from the frame header of a JPEG file (markers only, no decode)."""
    from .jpeg import jpeg_size as size
    return size(path)


def image_size(path):
    """(width, height) of a PNG or JPEG file, told apart by the signature; header only."""
    return jpeg_size(path) if _header(path)[0] == "jpeg" else png_size(path)


def transforms_frames(path, transformsfile, extension=".png"):
    """A D-NeRF transforms_*.json under `path` -> per frame (R, T, camera_angle_x, time or None, image path or
    None): the one parser of that file. Sizes, fields of view and what a missing time or file means are the
    callers'."""
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    fovx = contents["camera_angle_x"]
    return [blender_c2w_to_RT(np.array(frame["transform_matrix"])) +
            (fovx, frame.get("time"), os.path.join(path, frame["file_path"] + extension) if "file_path" in frame else None)
            for frame in contents["frames"]]


def transforms_camera(idx, R, T, fovx, fid, image_path, width, height):
    """The CameraInfo of one transforms frame at a frame size: dataset_readers.py:256-262."""
    fovy = focal2fov(fov2focal(fovx, width), height)
    # :257-259 swaps the names: FovY = fovx, FovX = fovy
    return CameraInfo(uid=idx, R=R, T=T, FovY=fovx, FovX=fovy, image_path=image_path,
                      image_name=os.path.splitext(os.path.basename(image_path))[0] if image_path else None,
                      width=width, height=height, fid=fid)


def read_cameras_from_transforms(path, transformsfile, extension=".png"):
    """dataset_readers.py:223-266 without the image load (the images are ingested per set, in one batch). The size
    is the PNG header's; a frame without file_path or time is a KeyError."""
    infos = []
    for idx, (R, T, fovx, time, image_path) in enumerate(transforms_frames(path, transformsfile, extension)):
        for key, value in (("file_path", image_path), ("time", time)):
            if value is None:
                raise KeyError(key)
        infos.append(transforms_camera(idx, R, T, fovx, time, image_path, *png_size(image_path)))
    return infos


def nerfpp_norm(cam_infos):
    """dataset_readers.py:77-98 getNerfppNorm."""
    centers = np.hstack([np.linalg.inv(getWorld2View2(c.R, c.T))[:3, 3:4] for c in cam_infos])
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


def store_ply(path, xyz, rgb):
    """dataset_readers.py:154-169 storePly: x y z nx ny nz float, red green blue uchar, binary little endian."""
    n = xyz.shape[0]
    el = np.zeros(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                            ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    el["x"], el["y"], el["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rgb8 = np.asarray(rgb).astype(np.uint8)  # truncation, as the structured assignment upstream
    el["red"], el["green"], el["blue"] = rgb8[:, 0], rgb8[:, 1], rgb8[:, 2]
    header = f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n"
    header += "".join(f"property {'uchar' if el.dtype[name].itemsize == 1 else 'float'} {name}\n" for name in el.dtype.names)
    with open(path, "wb") as f:
        f.write((header + "end_header\n").encode("ascii"))
        f.write(el.tobytes())


def fetch_ply(path):
    """dataset_readers.py:144-151 fetchPly for a binary little-endian vertex element of scalar properties."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fields, n, in_vertex = [], None, False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PLY header without end_header")
            parts = line.decode("ascii").split()
            if not parts:
                continue
            if parts[0] == "format" and parts[1] != "binary_little_endian":
                raise ValueError(f"{path}: only binary_little_endian PLY is supported")
            if parts[0] == "element":
                in_vertex = parts[1] == "vertex"
                if in_vertex:
                    n = int(parts[2])
            elif parts[0] == "property" and in_vertex:
                if parts[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: PLY property type {parts[1]}")
                fields.append((parts[-1], _PLY_TYPES[parts[1]]))
            elif parts[0] == "end_header":
                break
        if n is None:
            raise ValueError(f"{path}: PLY without a vertex element")
        dt = np.dtype(fields)
        buf = f.read(n * dt.itemsize)
    if len(buf) != n * dt.itemsize:
        raise ValueError(f"{path}: PLY vertex data is short")
    v = np.frombuffer(buf, dtype=dt, count=n)
    # row-major copies: create_from_pcd turns them into the (contiguous) Gaussian parameters as they are
    points = np.ascontiguousarray(np.vstack([v["x"], v["y"], v["z"]]).T)
    colors = np.ascontiguousarray(np.vstack([v["red"], v["green"], v["blue"]]).T) / 255.0
    names = set(dt.names)
    normals = (np.ascontiguousarray(np.vstack([v["nx"], v["ny"], v["nz"]]).T) if {"nx", "ny", "nz"} <= names
               else np.zeros_like(points))
    return BasicPointCloud(points=points, colors=colors, normals=normals)


def random_point_cloud(num_pts, seed=0):
    """dataset_readers.py:286-293: positions uniform in [-1.3, 1.3]^3, colours SH2RGB(U[0, 1) / 255), from a
    seeded generator (the reference draws from numpy's global state). -> (xyz, rgb in [0, 1])."""
    rng = np.random.default_rng(seed)
    xyz = rng.random((num_pts, 3)) * 2.6 - 1.3
    shs = rng.random((num_pts, 3)) / 255.0
    return xyz, shs * C0 + 0.5


def start_point_cloud(source_ply, make_points, model_path, normals_dtype=np.float64):
    """The start-up cloud of every reader -> (BasicPointCloud, ply_path). SOURCE's own .ply if present; otherwise
    make_points() -> (xyz, rgb on the 0..255 scale), written to MODEL/input.ply when model_path is given (never
    under SOURCE) and read back from there, so the colours carry the file's 8-bit truncation as upstream. Without
    a model_path the same cloud is built in memory and ply_path is None; its zero normals have the dtype the
    reader asks for (the Colmap reader's are float32, the other two's float64)."""
    if os.path.exists(source_ply):
        return fetch_ply(source_ply), source_ply
    xyz, rgb = make_points()
    if model_path:
        os.makedirs(model_path, exist_ok=True)
        ply_path = os.path.join(model_path, "input.ply")
        store_ply(ply_path, xyz, rgb)
        return fetch_ply(ply_path), ply_path
    return BasicPointCloud(points=xyz.astype(np.float32), colors=rgb.astype(np.uint8) / 255.0,
                           normals=np.zeros((xyz.shape[0], 3), normals_dtype)), None


def read_nerf_synthetic(path, white_background, eval, extension=".png", init_points=100_000, model_path=None, seed=0):
    """dataset_readers.py:269-306. white_background is applied when the images are ingested (Scene); it is
    kept in the signature of the reference. The point cloud is SOURCE/points3d.ply if present; otherwise
    `init_points` seeded random points (start_point_cloud)."""
    train = read_cameras_from_transforms(path, "transforms_train.json", extension)
    test = read_cameras_from_transforms(path, "transforms_test.json", extension)
    if not eval:
        train.extend(test)
        test = []
    norm = nerfpp_norm(train)

    def points():
        xyz, rgb = random_point_cloud(init_points, seed)
        return xyz, rgb * 255

    pcd, ply_path = start_point_cloud(os.path.join(path, "points3d.ply"), points, model_path)
    return SceneInfo(point_cloud=pcd, train_cameras=train, test_cameras=test, nerf_normalization=norm, ply_path=ply_path)


NERFIES_KINDS = ("vrig", "nerf", "interp", "other")


def nerfies_kind_of(path):
    """dataset_readers.py:409-430: the split branch from the name of SOURCE's parent directory, taken from the
    absolute, normalised path (a trailing slash or a relative path does not change the answer)."""
    name = os.path.basename(os.path.dirname(os.path.abspath(path)))
    if name.startswith("vrig"):
        return "vrig"
    if name.startswith("NeRF") or name.startswith("nerf"):
        return "nerf"
    if name.startswith("interp") or name.startswith("hyper"):
        return "interp"
    return "other"


def camera_nerfies_from_json(path, scale):
    """camera_utils.py:92-112. Principal point, skew and distortion are read and, as upstream, used nowhere."""
    with open(path) as f:
        camera_json = json.load(f)
    if "tangential" in camera_json:  # old camera JSON
        camera_json["tangential_distortion"] = camera_json["tangential"]
    return dict(orientation=np.array(camera_json["orientation"]), position=np.array(camera_json["position"]),
                focal_length=camera_json["focal_length"] * scale,
                principal_point=np.array(camera_json["principal_point"]) * scale, skew=camera_json["skew"],
                pixel_aspect_ratio=camera_json["pixel_aspect_ratio"],
                radial_distortion=np.array(camera_json["radial_distortion"]),
                tangential_distortion=np.array(camera_json["tangential_distortion"]))


def read_nerfies_cameras(path, nerfies_kind=None):
    """dataset_readers.py:398-473 without the image load. nerfies_kind: one of NERFIES_KINDS to choose the split
    branch explicitly; None applies the directory-name rule. -> (CameraInfos, train then val; train_num; scene
    centre; scene scale)."""
    kind = nerfies_kind or nerfies_kind_of(path)
    if kind not in NERFIES_KINDS:
        raise ValueError(f"nerfies_kind {kind!r}: one of {', '.join(NERFIES_KINDS)}")
    with open(os.path.join(path, "scene.json")) as f:
        scene_json = json.load(f)
    with open(os.path.join(path, "metadata.json")) as f:
        meta_json = json.load(f)
    with open(os.path.join(path, "dataset.json")) as f:
        dataset_json = json.load(f)
    coord_scale = scene_json["scale"]
    scene_center = scene_json["center"]
    if kind in ("vrig", "nerf"):
        train_img = dataset_json["train_ids"]
        all_img = train_img + dataset_json["val_ids"]
        ratio = 0.25 if kind == "vrig" else 1.0
    elif kind == "interp":
        train_img = dataset_json["ids"][::4]
        all_img = train_img + dataset_json["ids"][2::4]
        ratio = 0.5
    else:
        train_img = dataset_json["ids"][::4]
        all_img = train_img
        ratio = 0.5
    max_time = max(meta_json[i]["time_id"] for i in all_img)
    infos = []
    for idx, im in enumerate(all_img):
        camera = camera_nerfies_from_json(os.path.join(path, "camera", f"{im}.json"), ratio)
        position = (camera["position"] - scene_center) * coord_scale
        image_path = os.path.join(path, "rgb", f"{int(1 / ratio)}x", f"{im}.png")
        width, height = png_size(image_path)
        R = camera["orientation"].T
        T = -position @ R
        focal = camera["focal_length"]
        infos.append(CameraInfo(uid=idx, R=R, T=T, FovY=focal2fov(focal, height), FovX=focal2fov(focal, width),
                                image_path=image_path, image_name=os.path.splitext(os.path.basename(image_path))[0],
                                width=width, height=height, fid=meta_json[im]["time_id"] / max_time))
    return infos, len(train_img), scene_center, coord_scale


def read_nerfies(path, eval, model_path=None, nerfies_kind=None, seed=0):
    """dataset_readers.py:476-509. The point cloud is SOURCE/points3d.ply if present; otherwise points.npy as
    (xyz - center) * scale with colours SH2RGB(U[0, 1) / 255) from a seeded generator (start_point_cloud)."""
    cams, train_num, scene_center, scene_scale = read_nerfies_cameras(path, nerfies_kind)
    train, test = (cams[:train_num], cams[train_num:]) if eval else (cams, [])
    norm = nerfpp_norm(train)

    def points():
        npy_path = os.path.join(path, "points.npy")
        if not os.path.exists(npy_path):
            raise ValueError(f"{path}: neither points3d.ply nor points.npy (a Nerfies dataset brings its point cloud)")
        xyz = (np.load(npy_path) - scene_center) * scene_scale
        rgb = np.random.default_rng(seed).random((xyz.shape[0], 3)) / 255.0 * C0 + 0.5
        return xyz, rgb * 255

    pcd, ply_path = start_point_cloud(os.path.join(path, "points3d.ply"), points, model_path)
    return SceneInfo(point_cloud=pcd, train_cameras=train, test_cameras=test, nerf_normalization=norm, ply_path=ply_path)


COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
ColmapCamera = namedtuple("ColmapCamera", "id model width height params")
ColmapImage = namedtuple("ColmapImage", "id qvec tvec camera_id name")


def qvec2rotmat(qvec):
    """Rotation matrix of a unit quaternion (w, x, y, z): colmap_loader.py:43-53, each entry with its operations
    in the reference's order (the golden comparison is bitwise)."""
    w, x, y, z = qvec[0], qvec[1], qvec[2], qvec[3]
    return np.array([[1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


class _Records:
    """Little-endian records of a Colmap .bin file; a short file is a ValueError."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            self.data = f.read()
        self.pos = 0

    def take(self, fmt):
        size = struct.calcsize("<" + fmt)
        if self.pos + size > len(self.data):
            raise ValueError(f"{self.path}: truncated Colmap file")
        out = struct.unpack_from("<" + fmt, self.data, self.pos)
        self.pos += size
        return out

    def skip(self, size):
        if size < 0 or self.pos + size > len(self.data):
            raise ValueError(f"{self.path}: truncated Colmap file")
        self.pos += size

    def cstring(self):
        end = self.data.find(b"\0", self.pos)
        if end < 0:
            raise ValueError(f"{self.path}: truncated Colmap file")
        out = self.data[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return out


def _data_lines(path):
    with open(path) as f:
        return [ln.strip() for ln in f]


def read_colmap_intrinsics(path):
    """colmap_loader.py:209-235 (cameras.bin) / :149-171 (cameras.txt) -> {camera_id: ColmapCamera}."""
    cams = {}
    if path.endswith(".bin"):
        rec = _Records(path)
        for _ in range(rec.take("Q")[0]):
            cid, mid, w, h = rec.take("iiQQ")
            if mid not in COLMAP_MODELS:
                raise ValueError(f"{path}: unknown Colmap camera model id {mid}")
            name, n = COLMAP_MODELS[mid]
            cams[cid] = ColmapCamera(cid, name, w, h, np.array(rec.take("d" * n)))
        return cams
    for ln in _data_lines(path):
        if ln and ln[0] != "#":
            el = ln.split()
            cams[int(el[0])] = ColmapCamera(int(el[0]), el[1], int(el[2]), int(el[3]), np.array(tuple(map(float, el[4:]))))
    return cams


def read_colmap_extrinsics(path):
    """colmap_loader.py:174-206 (images.bin) / :238-264 (images.txt) -> {image_id: ColmapImage} in file order;
    the per-image 2D points (24 bytes each, or the second line of a text record) are skipped."""
    images = {}
    if path.endswith(".bin"):
        rec = _Records(path)
        for _ in range(rec.take("Q")[0]):
            v = rec.take("idddddddi")
            name = rec.cstring()
            rec.skip(24 * rec.take("Q")[0])
            images[v[0]] = ColmapImage(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name)
        return images
    lines = _data_lines(path)
    k = 0
    while k < len(lines):
        ln = lines[k]
        k += 1
        if ln and ln[0] != "#":
            el = ln.split()
            if len(el) < 10:
                raise ValueError(f"{path}: an image line needs 10 fields, got {len(el)}")
            images[int(el[0])] = ColmapImage(int(el[0]), np.array(tuple(map(float, el[1:5]))),
                                             np.array(tuple(map(float, el[5:8]))), int(el[8]), el[9])
            k += 1  # the line of 2D points (it may be empty)
    return images


def read_colmap_points(path):
    """colmap_loader.py:118-146 (points3D.bin) / :87-115 (points3D.txt) -> xyz (n, 3), rgb (n, 3) float64."""
    if path.endswith(".bin"):
        rec = _Records(path)
        n = rec.take("Q")[0]
        if 43 * n > len(rec.data):
            raise ValueError(f"{path}: truncated Colmap file")
        xyz, rgb = np.empty((n, 3)), np.empty((n, 3))
        for i in range(n):
            v = rec.take("QdddBBBd")
            xyz[i], rgb[i] = v[1:4], v[4:7]
            rec.skip(8 * rec.take("Q")[0])
        return xyz, rgb
    xyz, rgb = [], []
    for ln in _data_lines(path):
        if ln and ln[0] != "#":
            el = ln.split()
            xyz.append(tuple(map(float, el[1:4])))
            rgb.append(tuple(map(int, el[4:7])))
    return np.array(xyz, np.float64).reshape(-1, 3), np.array(rgb, np.float64).reshape(-1, 3)


def colmap_model_files(path):
    """(images file, cameras file) of sparse/0: the .bin pair, else the .txt pair, else None."""
    for ext in (".bin", ".txt"):
        pair = [os.path.join(path, "sparse", "0", n + ext) for n in ("images", "cameras")]
        if all(os.path.isfile(p) for p in pair):
            return pair
    return None


def read_colmap_cameras(path, images=None):
    """dataset_readers.py:101-141 without the image load, in the order of the images file. images: the
    directory of the image files under SOURCE (default "images")."""
    pair = colmap_model_files(path)
    if pair is None:
        raise ValueError(f"{path}: a Colmap dataset without sparse/0/{{images,cameras}}.{{bin,txt}}: that layout is unsupported")
    extrinsics, intrinsics = read_colmap_extrinsics(pair[0]), read_colmap_intrinsics(pair[1])
    folder = os.path.join(path, "images" if images is None else images)
    num_frames = len(extrinsics)
    if num_frames < 2:
        raise ValueError(f"{path}: a Colmap model of {num_frames} image(s): the frame time is int(name) / (images - 1), "
                         "which needs at least two")
    infos = []
    for extr in extrinsics.values():
        if extr.camera_id not in intrinsics:
            raise ValueError(f"{pair[0]}: image {extr.name} refers to camera {extr.camera_id}, which {pair[1]} does not hold")
        intr = intrinsics[extr.camera_id]
        R = np.transpose(qvec2rotmat(extr.qvec))
        T = np.array(extr.tvec)
        if intr.model == "SIMPLE_PINHOLE":
            fovy, fovx = focal2fov(intr.params[0], intr.height), focal2fov(intr.params[0], intr.width)
        elif intr.model == "PINHOLE":
            fovy, fovx = focal2fov(intr.params[1], intr.height), focal2fov(intr.params[0], intr.width)
        else:
            raise ValueError(f"{pair[1]}: camera model {intr.model}: Colmap camera model not handled: only undistorted "
                             "datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!")
        image_path = os.path.join(folder, os.path.basename(extr.name))
        image_name = os.path.basename(image_path).split(".")[0]
        try:
            number = int(image_name)
        except ValueError:
            raise ValueError(f"{pair[0]}: image name {extr.name!r}: a Colmap image must be named by its frame number "
                             "(the frame time is int(name) / (images - 1))") from None
        fmt, _, _, colour_type = _header(image_path)
        if fmt == "png" and colour_type in (4, 6):
            raise ValueError(f"{image_path}: an image with an alpha channel in a Colmap directory (gt_alpha_mask) is unsupported")
        infos.append(CameraInfo(uid=intr.id, R=R, T=T, FovY=fovy, FovX=fovx, image_path=image_path, image_name=image_name,
                                width=intr.width, height=intr.height, fid=number / (num_frames - 1)))
    return infos


def read_colmap(path, eval, images=None, model_path=None, llffhold=8):
    """dataset_readers.py:172-220. The point cloud is sparse/0/points3D.ply if present; otherwise points3D.bin,
    else points3D.txt (start_point_cloud; the reference writes the converted cloud to sparse/0/points3D.ply)."""
    cams = sorted(read_colmap_cameras(path, images), key=lambda c: c.image_name)  # as strings: "10" < "2"
    if eval:
        train = [c for i, c in enumerate(cams) if i % llffhold != 0]
        test = [c for i, c in enumerate(cams) if i % llffhold == 0]
    else:
        train, test = cams, []
    norm = nerfpp_norm(train)
    sparse = os.path.join(path, "sparse", "0")

    def points():
        for name in ("points3D.bin", "points3D.txt"):
            if os.path.isfile(os.path.join(sparse, name)):
                return read_colmap_points(os.path.join(sparse, name))
        raise ValueError(f"{path}: no sparse/0/points3D.ply, .bin or .txt (a Colmap dataset brings its point cloud)")

    pcd, ply_path = start_point_cloud(os.path.join(sparse, "points3D.ply"), points, model_path, np.float32)
    return SceneInfo(point_cloud=pcd, train_cameras=train, test_cameras=test, nerf_normalization=norm, ply_path=ply_path)


# scene/__init__.py:45-63 in its order: marker file or directory -> the format it announces
_FORMAT_MARKERS = (("sparse", "Colmap"), ("transforms_train.json", "D-NeRF"), ("cameras_sphere.npz", "DTU"),
                   ("dataset.json", "Nerfies"), ("poses_bounds.npy", "plenoptic video (Neu3D)"),
                   ("transforms.json", "Dynamic-360"))


def dataset_format(source_path):
    """"Colmap", "D-NeRF" or "Nerfies" by the reference's dispatch order; ValueError for the formats it also
    knows but this package does not read, for a sparse/ without a readable sparse/0 model, and for a directory
    it would not recognise either."""
    for marker, name in _FORMAT_MARKERS:
        if os.path.exists(os.path.join(source_path, marker)):
            if name in ("D-NeRF", "Nerfies"):
                return name
            if name == "Colmap":
                if colmap_model_files(source_path) is not None:
                    return name
                raise ValueError(f"{source_path}: found {marker}, a Colmap dataset without "
                                 "sparse/0/{images,cameras}.{bin,txt}: that layout is unsupported")
            raise ValueError(f"{source_path}: found {marker}, a {name} dataset: that format is unsupported "
                             "(D-NeRF and Nerfies directories are read)")
    raise ValueError(f"{source_path}: could not recognise the scene type (no transforms_train.json of a D-NeRF "
                     "directory and no dataset.json of a Nerfies one)")


def render_format(source_path):
    """The render script's reader of SOURCE, on the same markers: "Colmap" where sparse/ exists (with
    dataset_format's refusal of an unreadable sparse/0), "Nerfies" for a dataset.json without a
    transforms_train.json, and "D-NeRF", the transforms reader, for everything else. The two rules differ where
    training refuses: a DTU, plenoptic or Dynamic-360 marker, or no marker at all (one transforms_test.json, an
    empty directory), is a ValueError of dataset_format and the transforms reader here, which takes whichever of
    the two transforms files exist and yields empty sets for the others."""
    found = {name for marker, name in _FORMAT_MARKERS if os.path.exists(os.path.join(source_path, marker))}
    if "Colmap" in found:
        return dataset_format(source_path)  # sparse is the first marker: "Colmap", or the refusal
    return "Nerfies" if "Nerfies" in found and "D-NeRF" not in found else "D-NeRF"


def read_scene_info(source_path, white_background, eval, init_points=100_000, model_path=None, nerfies_kind=None,
                    images=None):
    """The reader of the directory's format (dataset_format). init_points only applies to D-NeRF directories:
    a Nerfies or a Colmap one starts from its own point cloud. images: the image directory of a Colmap one."""
    fmt = dataset_format(source_path)
    if fmt == "Colmap":
        return read_colmap(source_path, eval, images=images, model_path=model_path)
    if fmt == "Nerfies":
        return read_nerfies(source_path, eval, model_path=model_path, nerfies_kind=nerfies_kind)
    return read_nerf_synthetic(source_path, white_background, eval, init_points=init_points, model_path=model_path)


def target_resolution(orig_w, orig_h, resolution):
    """camera_utils.py:24-42 at resolution_scale 1: -r in {1, 2, 4, 8} -> round(orig / r) per axis (Python's
    round: halves go to even); -1 -> full size unless wider than 1600; anything else is a target width."""
    if resolution in (1, 2, 4, 8):
        return round(orig_w / resolution), round(orig_h / resolution)
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down)
    return int(orig_w / scale), int(orig_h / scale)


def camera_to_json(id, cam):
    """camera_utils.py:69-89 on a CameraInfo."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = cam.R.transpose()
    Rt[:3, 3] = cam.T
    Rt[3, 3] = 1.0
    W2C = np.linalg.inv(Rt)
    return {"id": id, "img_name": cam.image_name, "width": cam.width, "height": cam.height,
            "position": W2C[:3, 3].tolist(), "rotation": [x.tolist() for x in W2C[:3, :3]],
            "fy": fov2focal(cam.FovY, cam.height), "fx": fov2focal(cam.FovX, cam.width)}


def load_cameras(cam_infos, resolution, white_background, device, size=None):
    """camera_utils.py:60-66 cameraList_from_camInfos: one ingest batch for the set, one Camera per view.
    size None: the -r rule (target_resolution) on the files' own size; every view has its image. size (W, H),
    the render script's forced frame size: views whose image file exists carry it resized to that (byte / 255,
    which an 8-bit write maps back to the same byte), the others stay without original_image."""
    if not cam_infos:
        return []
    have = [i for i, c in enumerate(cam_infos) if size is None or (c.image_path and os.path.isfile(c.image_path))]
    if have:
        images = ingest_images([cam_infos[i].image_path for i in have], white_background, device=device,
                               size=size or (lambda w, h: target_resolution(w, h, resolution)))
    width, height = size or (images.shape[3], images.shape[2])
    cams = []
    for i, c in enumerate(cam_infos):
        cam = Camera(c.R, c.T, FoVx=c.FovX, FoVy=c.FovY, width=width, height=height, fid=c.fid, uid=i, data_device=device)
        cam.image_name = c.image_name
        cams.append(cam)
    for k, i in enumerate(have):
        cams[i].original_image = images[k]
    return cams


class Scene:
    """scene/__init__.py:23-112 for a Colmap, a D-NeRF or a Nerfies directory (dataset_format). args: source_path,
    model_path, white_background, eval, resolution (default -1), init_points (default 100 000; D-NeRF only),
    nerfies_kind (default None: the directory-name rule), images (default "images": the image directory of a
    Colmap SOURCE), data_device (default "cuda"). white_background has no effect on images without alpha
    (Nerfies and Colmap captures)."""

    def __init__(self, args, gaussians, load_iteration=None):
        from .deform_model import searchForMaxIteration
        self.model_path = args.model_path
        self.gaussians = gaussians
        self.loaded_iter = None
        if load_iteration is not None:
            self.loaded_iter = (searchForMaxIteration(os.path.join(self.model_path, "point_cloud"))
                                if load_iteration == -1 else load_iteration)
        self.format = dataset_format(args.source_path)  # raises on what is not read, before MODEL is created
        device = torch.device(getattr(args, "data_device", "cuda"))
        os.makedirs(self.model_path, exist_ok=True)
        info = read_scene_info(args.source_path, args.white_background, args.eval,
                               init_points=getattr(args, "init_points", 100_000),
                               model_path=None if self.loaded_iter else self.model_path,
                               nerfies_kind=getattr(args, "nerfies_kind", None),
                               images=getattr(args, "images", None))
        if not self.loaded_iter:
            dest = os.path.join(self.model_path, "input.ply")
            if info.ply_path != dest:  # SOURCE/points3d.ply: copied, as upstream
                with open(info.ply_path, "rb") as src, open(dest, "wb") as dst:
                    dst.write(src.read())
            camlist = list(info.test_cameras) + list(info.train_cameras)
            with open(os.path.join(self.model_path, "cameras.json"), "w") as f:
                json.dump([camera_to_json(i, c) for i, c in enumerate(camlist)], f)
            with open(os.path.join(self.model_path, "cfg_args"), "w") as f:
                f.write(str(Namespace(**{k: v for k, v in sorted(vars(args).items())})))
        self.cameras_extent = float(info.nerf_normalization["radius"])
        resolution = getattr(args, "resolution", -1)
        self.train_cameras = load_cameras(info.train_cameras, resolution, args.white_background, device)
        self.test_cameras = load_cameras(info.test_cameras, resolution, args.white_background, device)
        if self.loaded_iter:
            self.gaussians.load_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{self.loaded_iter}",
                                                 "point_cloud.ply"), device=device)
        else:
            self.gaussians.create_from_pcd(info.point_cloud, self.cameras_extent, device=device)

    def save(self, iteration):
        self.gaussians.save_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{iteration}", "point_cloud.ply"))

    def getTrainCameras(self):
        return self.train_cameras

    def getTestCameras(self):
        return self.test_cameras
