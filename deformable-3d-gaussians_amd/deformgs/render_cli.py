"""python -m deformgs.render_cli -m MODEL --mode {render,time,view,all,pose,original} — the counterpart of
render_baseline.py:299-350 on render_frames.

Loads MODEL/point_cloud/iteration_k/point_cloud.ply and MODEL/deform/iteration_k/deform.pth, builds the
mode's frame list (deformgs/camera_paths.py), renders it with render_frames (8-bit colour and depth straight
from the blend kernel) and writes <MODEL>/<train|test>/<mode dir>_<k>/renders/%05d.png, depth/%05d.png and,
for mode render, gt/%05d.png — the reference's directory names — with the stdlib PNG writer (--png zlib, the
default) or the device encoder of deformgs/png_gpu.py (--png gpu: the same pixels, smaller files). Prints the
reference's FPS line for every set (frames / elapsed of the render_frames call between two device
synchronisations). --video mjpeg writes, in the five interpolation modes, renders/video.avi beside the PNGs: the
reference's imageio video (render_baseline.py: fps 30 for time / view / all, 60 for pose / original) as Motion-JPEG
in an AVI container (deformgs/mjpeg.py), its frames encoded on the device chunk by chunk from the same rgb8 frames
(deformgs/jpeg_gpu.py; --video_quality, --video_subsampling). Mode render writes no video, as the reference writes
none there. MP4 / H.264 is out of scope (it needs an encoder library).

Cameras: --synthetic N takes the synthetic scene of deformgs/train.py (N Gaussians, --res W H); when MODEL
holds no saved model yet, the scene's own initial Gaussians and a fresh network (heads at 1/100 scale) are
saved there as iteration 0 first, so the script runs with no dataset. -s SOURCE reads a D-NeRF style
transforms_train.json / transforms_test.json (camera_angle_x, per frame transform_matrix and time;
dataset_readers.py:222-262) for the cameras; a view whose image file exists carries it as ground truth (composited
over the chosen background and resized to --res by deformgs/ingest.py), and gt/ is written for those views.
-s SOURCE at a Nerfies directory (dataset.json: NeRF-DS / HyperNeRF) takes both sets from the training reader
(deformgs/dataset.read_nerfies_cameras: train ids, then val ids as the test set): cameras, frame times and
ground-truth images from the files; without --res the frame size is the dataset's own after -r, the training
size. -s SOURCE at a Colmap directory (sparse/0) does the same through deformgs/dataset.read_colmap: cameras
sorted by name, every 8th the test set, images from -i / --images (default images).
"""
import argparse
import os
import time

import torch

from .camera_paths import DIR_NAMES, MODES, frame_list
from .cameras import Camera
from .png import write_png


class _Set:
    def __init__(self, train, test):
        self.train, self.test = train, test


def read_transforms(source, width, height, device, white_background=False, extension=".png"):
    """D-NeRF transforms_{train,test}.json -> _Set of Cameras (dataset_readers.py:222-262) at the given frame
    size; a missing file is an empty set, a frame without `time` takes k / (n - 1), and a view carries its
    ground-truth image (composited over the background) when the frame's file exists under `source`."""
    from .dataset import load_cameras, transforms_camera, transforms_frames
    sets = []
    for name in ("transforms_train.json", "transforms_test.json"):
        frames = transforms_frames(source, name, extension) if os.path.exists(os.path.join(source, name)) else []
        infos = [transforms_camera(k, R, T, float(fovx), k / max(len(frames) - 1, 1) if t is None else float(t),
                                   image_path, width, height) for k, (R, T, fovx, t, image_path) in enumerate(frames)]
        sets.append(load_cameras(infos, None, white_background, device, size=(width, height)))
    return _Set(*sets)


def read_dataset_sets(source, fmt, res, resolution, device, nerfies_kind=None, images=None):
    """A "Nerfies" or "Colmap" directory -> _Set of Cameras with their ground truth, split as the training reader
    splits it with --eval (Nerfies: train ids, then val ids; Colmap: every 8th camera by name is the test set).
    res None: the files' size after the -r rule; (W, H): that frame size (dataset.load_cameras)."""
    from .dataset import load_cameras, read_colmap, read_nerfies_cameras
    if fmt == "Colmap":
        info = read_colmap(source, True, images=images)
        parts = info.train_cameras, info.test_cameras
    else:
        infos, train_num, _, _ = read_nerfies_cameras(source, nerfies_kind)
        parts = infos[:train_num], infos[train_num:]
    return _Set(*(load_cameras(part, resolution, False, device, size=res) for part in parts))


def _iteration(model_path, iteration):
    from .deform_model import searchForMaxIteration
    if iteration >= 0:
        return iteration
    return searchForMaxIteration(os.path.join(model_path, "point_cloud"))


def load_scene(args, device="cuda"):
    """-> (gaussians, deform, camera sets, background, iteration) for the parsed arguments."""
    from .deform_model import DeformModelBaseline
    from .gaussian_model import GaussianModel
    dev = torch.device(device)
    W, H = args.res or (800, 800)
    if args.synthetic:
        from .train import SyntheticScene
        scene = SyntheticScene(args.synthetic, W, H, device=dev, white_background=args.white_background)
        cams = _Set(scene.getTrainCameras(), scene.getTestCameras())
        if not os.path.isdir(os.path.join(args.model_path, "point_cloud")):
            g0 = scene.init_gaussians(GaussianModel(3))
            g0.save_ply(os.path.join(args.model_path, "point_cloud", "iteration_0", "point_cloud.ply"))
            torch.manual_seed(0)
            d0 = DeformModelBaseline(not args.non_blender, args.is_6dof, device=dev)
            net = d0.deform
            heads = (net.branch_w, net.branch_v) if args.is_6dof else (net.gaussian_warp,)
            with torch.no_grad():
                for head in heads + (net.gaussian_rotation, net.gaussian_scaling):
                    head.weight.mul_(0.01)
                    head.bias.mul_(0.01)
            d0.save_weights(args.model_path, 0)
    elif args.source_path:
        from .dataset import render_format
        fmt = render_format(args.source_path)
        if fmt == "D-NeRF":
            cams = read_transforms(args.source_path, W, H, dev, white_background=args.white_background)
        else:
            cams = read_dataset_sets(args.source_path, fmt, args.res, args.resolution, dev, args.nerfies_kind, args.images)
    else:
        raise SystemExit("render_cli: give the cameras with --synthetic N or -s SOURCE (transforms_*.json)")
    it = _iteration(args.model_path, args.iteration)
    gaussians = GaussianModel(args.sh_degree)
    gaussians.load_ply(os.path.join(args.model_path, "point_cloud", f"iteration_{it}", "point_cloud.ply"), device=dev)
    deform = DeformModelBaseline(not args.non_blender, args.is_6dof, device=dev)
    deform.load_weights(args.model_path, iteration=it)
    bg = torch.tensor([1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0], device=dev)
    return gaussians, deform, cams, bg, it


def frame_cameras(mode, views, view_index=0, frames=None):
    """The mode's frames as (Cameras, times): mode render keeps the views themselves."""
    if mode == "render":
        return list(views), [float(v.fid) for v in views]
    v0 = views[view_index]
    fl = frame_list(mode, views, view_index, frames)
    cams = [Camera(R, T, v0.FoVx, v0.FoVy, v0.image_width, v0.image_height, fid=t, trans=v0.trans, scale=v0.scale,
                   data_device=v0.data_device) for R, T, t in fl]
    return cams, [t for _, _, t in fl]


VIDEO_FPS = {"time": 30, "view": 30, "all": 30, "pose": 60, "original": 60}  # render_baseline.py's mimwrite calls


def _write_video(path, rgb, fps, chunk, quality, subsampling):
    """renders/video.avi from the rgb8 frames: JPEG on the device in chunks of frames, the container on the host."""
    from .jpeg_gpu import encode_frames
    from .mjpeg import write_avi
    from .render_frames import default_chunk
    n = int(chunk) if chunk else default_chunk(rgb.shape[1], rgb.shape[2], ("rgb8", "depth8"))
    jpegs = []
    for k in range(0, rgb.shape[0], n):
        jpegs += encode_frames(rgb[k:k + n], quality=quality, subsampling=subsampling)
    write_avi(path, jpegs, rgb.shape[2], rgb.shape[1], fps)


def _gt8(cams):
    """The views' ground truth as the bytes gt/ holds: uint8 (n, H, W, 3) on the images' device."""
    gt = torch.stack([c.original_image[0:3] for c in cams])
    return (255 * gt.clamp(0, 1)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _write_gpu(out, cams, dirs, chunk):
    """--png gpu: renders, depth and the 8-bit ground truth go through deformgs.png_gpu in chunks of frames; only
    compressed bytes reach the host."""
    from .png_gpu import write_frames
    from .render_frames import default_chunk
    rgb, dep = out["rgb8"], out["depth8"]
    n = int(chunk) if chunk else default_chunk(rgb.shape[1], rgb.shape[2], ("rgb8", "depth8"))
    for k in range(0, len(cams), n):
        idx = range(k, min(k + n, len(cams)))
        write_frames([os.path.join(dirs["renders"], f"{i:05d}.png") for i in idx], rgb[k:k + n])
        write_frames([os.path.join(dirs["depth"], f"{i:05d}.png") for i in idx], dep[k:k + n])
        if "gt" in dirs:
            have = [i for i in idx if getattr(cams[i], "original_image", None) is not None]
            if have:
                write_frames([os.path.join(dirs["gt"], f"{i:05d}.png") for i in have], _gt8([cams[i] for i in have]))


def render_set(model_path, name, iteration, mode, views, gaussians, deform, background, is_6dof, view_index=0,
               frames=None, chunk=None, png="zlib", video="none", video_quality=90, video_subsampling="4:2:0"):
    """Renders one camera set for `mode`, writes the PNGs, prints the FPS line. -> the output directory.
    png: "zlib" writes with deformgs.png.write_png from host copies of the frames, "gpu" with deformgs.png_gpu.
    video: "mjpeg" also writes renders/video.avi in an interpolation mode (nothing in mode render); "none" writes
    what was written before the option existed."""
    from .render_frames import render_frames
    if png not in ("zlib", "gpu"):
        raise ValueError(f"render_set: png must be 'zlib' or 'gpu', got {png!r}")
    if video not in ("none", "mjpeg"):
        raise ValueError(f"render_set: video must be 'none' or 'mjpeg', got {video!r}")
    base = os.path.join(model_path, name, f"{DIR_NAMES[mode]}_{iteration}")
    dirs = {k: os.path.join(base, k) for k in (("renders", "depth", "gt") if mode == "render" else ("renders", "depth"))}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    cams, times = frame_cameras(mode, views, view_index, frames)
    torch.cuda.synchronize()
    t0 = time.time()
    out = render_frames(cams, gaussians, deform, background, times=times, is_6dof=is_6dof, outputs=("rgb8", "depth8"),
                        chunk=chunk)
    torch.cuda.synchronize()
    dt = time.time() - t0
    if png == "gpu":
        if cams:
            _write_gpu(out, cams, dirs, chunk)
    else:
        rgb, dep = out["rgb8"].cpu().numpy(), out["depth8"].cpu().numpy()
        for i in range(len(cams)):
            write_png(os.path.join(dirs["renders"], f"{i:05d}.png"), rgb[i])
            write_png(os.path.join(dirs["depth"], f"{i:05d}.png"), dep[i])
            if mode == "render" and getattr(cams[i], "original_image", None) is not None:
                write_png(os.path.join(dirs["gt"], f"{i:05d}.png"), _gt8([cams[i]])[0].cpu().numpy())
    if video == "mjpeg" and mode in VIDEO_FPS and cams:
        _write_video(os.path.join(dirs["renders"], "video.avi"), out["rgb8"], VIDEO_FPS[mode], chunk, video_quality,
                     video_subsampling)
    fps = len(cams) / dt if dt > 0 and cams else 0.0
    print(f"Test FPS: \033[1;35m{fps:.5f}\033[0m, Num. of GS: {gaussians.get_xyz.shape[0]}", flush=True)
    return base


def build_parser():
    ap = argparse.ArgumentParser(description="Render a trained deformable-Gaussian model (render_baseline.py counterpart)")
    ap.add_argument("--model_path", "-m", required=True)
    ap.add_argument("--source_path", "-s", default="")
    ap.add_argument("--mode", default="render", choices=list(MODES))
    ap.add_argument("--iteration", default=-1, type=int)
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_test", action="store_true")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    ap.add_argument("--res", type=int, nargs=2, default=None, metavar=("W", "H"),
                    help="frame size (default 800 800; for a Nerfies or Colmap SOURCE the dataset's own size after -r)")
    ap.add_argument("--resolution", "-r", type=int, default=-1, help="the training script's -r (Nerfies or Colmap SOURCE)")
    ap.add_argument("--images", "-i", default="images", help="image directory of a Colmap SOURCE (under SOURCE)")
    ap.add_argument("--nerfies_kind", choices=["vrig", "nerf", "interp", "other"], default=None)
    ap.add_argument("--frames", type=int, default=None, help="frames of an interpolation mode (default: the reference's)")
    ap.add_argument("--view_index", type=int, default=-1, help="the fixed view of time / view / all / pose (-1: random)")
    ap.add_argument("--sh_degree", type=int, default=3)
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--is_6dof", action="store_true")
    ap.add_argument("--non_blender", action="store_true")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--png", choices=["zlib", "gpu"], default="zlib",
                    help="the PNG writer: zlib on the host (filter 0, level 6) or the device encoder (adaptive filters, "
                         "run matches; only compressed bytes leave the GPU)")
    ap.add_argument("--video", choices=["none", "mjpeg"], default="none",
                    help="mjpeg: the interpolation modes also write renders/video.avi (Motion-JPEG, frames encoded on the "
                         "device; 30 fps for time / view / all, 60 for pose / original)")
    ap.add_argument("--video_quality", type=int, default=90, help="JPEG quality of the video's frames, 1..100")
    ap.add_argument("--video_subsampling", choices=["4:4:4", "4:2:2", "4:2:0"], default="4:2:0")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print("Rendering " + args.model_path)
    with torch.no_grad():
        gaussians, deform, cams, bg, it = load_scene(args)
        done = []
        for name, views, skip in (("train", cams.train, args.skip_train), ("test", cams.test, args.skip_test)):
            if skip or not views:
                continue
            idx = args.view_index if args.view_index >= 0 else int(torch.randint(0, len(views), (1,)).item())
            done.append(render_set(args.model_path, name, it, args.mode, views, gaussians, deform, bg, args.is_6dof,
                                   view_index=idx, frames=args.frames, chunk=args.chunk, png=args.png,
                                   video=args.video, video_quality=args.video_quality,
                                   video_subsampling=args.video_subsampling))
    return done


if __name__ == "__main__":
    main()
