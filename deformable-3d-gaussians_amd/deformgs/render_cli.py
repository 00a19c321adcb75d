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
import json
import math
import os
import time

import numpy as np
import torch

from .camera_paths import DIR_NAMES, MODES, frame_list
from .cameras import Camera, blender_c2w_to_RT, focal2fov, fov2focal
from .png import write_png


class _Set:
    def __init__(self, train, test):
        self.train, self.test = train, test


def attach_images(cams, paths, white_background, width, height, device):
    """Views whose image file exists get original_image: composited over the background and resized to the
    render size by deformgs/ingest.py (byte / 255, which render_set's 8-bit gt/ write maps back to the same
    byte). The others stay without one."""
    from .ingest import ingest_images
    have = [i for i, p in enumerate(paths) if p and os.path.isfile(p)]
    if not have:
        return
    images = ingest_images([paths[i] for i in have], white_background, size=(width, height), device=device)
    for k, i in enumerate(have):
        cams[i].original_image = images[k]


def read_transforms(source, width, height, device, white_background=False, extension=".png"):
    """D-NeRF transforms_{train,test}.json -> _Set of Cameras (dataset_readers.py:222-262); a view carries its
    ground-truth image when the frame's file exists under `source`."""
    sets = {}
    for name in ("train", "test"):
        path = os.path.join(source, f"transforms_{name}.json")
        cams, files = [], []
        if os.path.exists(path):
            with open(path) as f:
                meta = json.load(f)
            fovx = float(meta["camera_angle_x"])
            frames = meta["frames"]
            for k, fr in enumerate(frames):
                R, T = blender_c2w_to_RT(np.array(fr["transform_matrix"]))
                fovy = focal2fov(fov2focal(fovx, width), height)
                fid = float(fr["time"]) if "time" in fr else k / max(len(frames) - 1, 1)
                # dataset_readers.py:260-262 swaps the names: FovY = fovx, FovX = fovy
                cams.append(Camera(R, T, FoVx=fovy, FoVy=fovx, width=width, height=height, fid=fid, uid=k,
                                   data_device=device))
                files.append(os.path.join(source, fr["file_path"] + extension) if "file_path" in fr else None)
            attach_images(cams, files, white_background, width, height, device)
        sets[name] = cams
    return _Set(sets["train"], sets["test"])


def read_nerfies_sets(source, res, resolution, device, nerfies_kind=None):
    """A Nerfies directory -> _Set of Cameras with their ground truth, split as the training reader splits it with
    --eval. res None: the files' size after the -r rule (dataset.load_cameras); (W, H): that frame size."""
    from .dataset import load_cameras, read_nerfies_cameras
    infos, train_num, _, _ = read_nerfies_cameras(source, nerfies_kind)
    sets = []
    for part in (infos[:train_num], infos[train_num:]):
        if res is None:
            sets.append(load_cameras(part, resolution, False, device))
            continue
        cams = [Camera(c.R, c.T, FoVx=c.FovX, FoVy=c.FovY, width=res[0], height=res[1], fid=c.fid, uid=k,
                       data_device=device) for k, c in enumerate(part)]
        attach_images(cams, [c.image_path for c in part], False, res[0], res[1], device)
        sets.append(cams)
    return _Set(*sets)


def read_colmap_sets(source, res, resolution, device, images=None):
    """A Colmap directory -> _Set of Cameras with their ground truth, split as the training reader splits it with
    --eval (every 8th camera by name is the test set). res as for read_nerfies_sets."""
    from .dataset import load_cameras, read_colmap
    info = read_colmap(source, True, images=images)
    sets = []
    for part in (info.train_cameras, info.test_cameras):
        if res is None:
            sets.append(load_cameras(part, resolution, False, device))
            continue
        cams = [Camera(c.R, c.T, FoVx=c.FovX, FoVy=c.FovY, width=res[0], height=res[1], fid=c.fid, uid=k,
                       data_device=device) for k, c in enumerate(part)]
        attach_images(cams, [c.image_path for c in part], False, res[0], res[1], device)
        sets.append(cams)
    return _Set(*sets)


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
    elif args.source_path and os.path.exists(os.path.join(args.source_path, "sparse")):
        from .dataset import dataset_format
        dataset_format(args.source_path)  # raises on a sparse/ without a readable sparse/0 model
        cams = read_colmap_sets(args.source_path, args.res, args.resolution, dev, args.images)
    elif args.source_path and os.path.exists(os.path.join(args.source_path, "dataset.json")) and not os.path.exists(
            os.path.join(args.source_path, "transforms_train.json")):
        cams = read_nerfies_sets(args.source_path, args.res, args.resolution, dev, args.nerfies_kind)
    elif args.source_path:
        cams = read_transforms(args.source_path, W, H, dev, white_background=args.white_background)
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
                gt = torch.stack([cams[i].original_image[0:3] for i in have])
                gt8 = (255 * gt.clamp(0, 1)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
                write_frames([os.path.join(dirs["gt"], f"{i:05d}.png") for i in have], gt8)


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
                gt = cams[i].original_image[0:3]
                gt8 = (255 * gt.clamp(0, 1)).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
                write_png(os.path.join(dirs["gt"], f"{i:05d}.png"), gt8)
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
