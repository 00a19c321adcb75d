"""Frame lists of the render script's modes: which (camera R, T, time) every output frame has.

Host-side mirror (numpy, no GPU) of the loops of render_baseline.py and the camera paths of
utils/pose_utils.py in preacherwhite/Deformable-3D-Gaussians:
  render    render_baseline.py:29-55    every view with its own fid
  time      :76-105  interpolate_time   one view, t = i / (frames - 1), 150 frames
  view      :108-154 interpolate_view   one view's wander path (utils/pose_utils.py:66-100), its fid, 60 frames
  all       :157-198 interpolate_all    pose_spherical(angle, -30, 4) over [-180, 180), t = i / (frames - 1), 150 frames
  pose      :201-245 interpolate_poses  linear R / T from the first to the last view, one view's fid, 520 frames
  original  :248-297 interpolate_view_original  piecewise-linear R / T through all views, t = i / (frames - 1), 1000 frames
A frame is (R (3,3) float64, T (3,) float64, time float): what Camera(R, T, ...) / reset_extrinsic take.
Pinned by tests/golden/render_paths.npz.
"""
import numpy as np

from .cameras import fov2focal

MODES = ("render", "time", "view", "all", "pose", "original")
DEFAULT_FRAMES = {"time": 150, "view": 60, "all": 150, "pose": 520, "original": 1000}
# output directory of every mode under <model>/<train|test>/
DIR_NAMES = {"render": "ours", "time": "interpolate", "view": "interpolate_view", "all": "interpolate_all",
             "pose": "interpolate_pose", "original": "interpolate_hyper_view"}


def pose_spherical(theta, phi, radius):
    """utils/pose_utils.py:58-63: camera-to-world of a camera on a sphere (degrees), float32 like the reference."""
    f = np.float32
    ph, th = phi / 180.0 * np.pi, theta / 180.0 * np.pi
    trans = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]], f)
    rot_phi = np.array([[1, 0, 0, 0], [0, np.cos(ph), -np.sin(ph), 0], [0, np.sin(ph), np.cos(ph), 0], [0, 0, 0, 1]], f)
    rot_theta = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]], f)
    flip = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], f)
    return flip @ (rot_theta @ (rot_phi @ trans))


def pose_to_RT(pose):
    """A camera-to-world pose -> the (R, T) Camera takes (render_baseline.py:128-131, dataset_readers.py:235-238)."""
    m = np.linalg.inv(np.array(pose))
    R = -np.transpose(m[:3, :3])
    R[:, 0] = -R[:, 0]
    return R, -m[:3, 3]


def render_wander_path(R, T, FoVy, image_height, num_frames=60, max_disp=5000.0):
    """utils/pose_utils.py:66-100: the view's pose displaced on a small closed loop; float32 4x4 poses.
    (The reference flips the view's own R in place while building the path; here R is copied.)"""
    focal = fov2focal(FoVy, image_height)
    R = np.array(R, np.float64)
    R[:, 1] = -R[:, 1]
    R[:, 2] = -R[:, 2]
    pose = np.concatenate([R, -np.asarray(T, np.float64).reshape(-1, 1)], -1)
    ref_pose = np.concatenate([pose, np.array([[0.0, 0.0, 0.0, 1.0]])], 0)
    max_trans = max_disp / focal
    out = []
    for i in range(num_frames):
        a = 2.0 * np.pi * float(i) / float(num_frames)
        shift = np.eye(4)
        shift[:3, 3] = [max_trans * np.sin(a), max_trans * np.cos(a) / 3.0, max_trans * np.cos(a) / 3.0]
        out.append(np.float32(ref_pose @ np.linalg.inv(shift)))
    return out


def frame_list(mode, views, view_index=0, frames=None):
    """views: objects with R, T, fid (and FoVy, image_height for mode "view"). -> list of (R, T, time)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    fid = lambda v: float(v.fid)  # noqa: E731
    if mode == "render":
        return [(np.array(v.R, np.float64), np.array(v.T, np.float64), fid(v)) for v in views]
    n = DEFAULT_FRAMES[mode] if frames is None else int(frames)
    view = views[view_index]
    tn = lambda i: i / (n - 1) if n > 1 else 0.0  # noqa: E731
    if mode == "time":
        return [(np.array(view.R, np.float64), np.array(view.T, np.float64), tn(i)) for i in range(n)]
    if mode == "view":
        return [pose_to_RT(p) + (fid(view),) for p in render_wander_path(view.R, view.T, view.FoVy, view.image_height, n)]
    if mode == "all":
        angles = np.linspace(-180, 180, n + 1)[:-1]
        return [pose_to_RT(pose_spherical(a, -30.0, 4.0)) + (tn(i),) for i, a in enumerate(angles)]
    lerp = lambda a, b, r: (1 - r) * np.asarray(a, np.float64) + r * np.asarray(b, np.float64)  # noqa: E731
    if mode == "pose":
        b, e = views[0], views[-1]
        return [(lerp(b.R, e.R, tn(i)), lerp(b.T, e.T, tn(i)), fid(view)) for i in range(n)]
    out = []  # original: stops where the upper neighbour would be past the last view
    for i in range(n):
        q = i / n * len(views)
        lo, hi = int(np.floor(q)), int(np.ceil(q))
        if hi == len(views):
            break
        out.append((lerp(views[lo].R, views[hi].R, q - lo), lerp(views[lo].T, views[hi].T, q - lo), tn(i)))
    return out
