"""The small scene of the render_frames tests: 3000 Gaussians drawn as synth-100k draws them but with
_scaling = log(SCALE), a 100 x 72 image (7 x 5 tiles, ragged right and bottom), 6 cameras on a circle with
distinct times, a network with the heads scaled as the bench scales them (x 0.01)."""
import math

import torch

N, H, W, F = 3000, 72, 100, 6
SCALE = 0.08


def gaussians(n=N, sh_degree=3, scale=SCALE, device="cuda"):
    from deformgs.gaussian_model import GaussianModel
    from deformgs.synthetic import synth_gaussians
    g = synth_gaussians(n, seed=0, device=device)
    gm = GaussianModel(3)
    gm.from_tensors(g["xyz"], g["features_dc"], g["features_rest"], torch.full_like(g["scaling"], math.log(scale)),
                    g["rotation"], g["opacity"], active_sh_degree=sh_degree)
    return gm


def cameras(n=F, width=W, height=H, device="cuda"):
    from deformgs.synthetic import synth_camera
    return [synth_camera(width, height, az=2.0 * math.pi * k / n, el=0.1 + 0.05 * k, fid=(k + 0.5) / n, device=device)
            for k in range(n)]


def network(is_blender=True, is_6dof=False, device="cuda"):
    from deformgs.deform_model import DeformModelBaseline
    torch.manual_seed(0)
    deform = DeformModelBaseline(is_blender=is_blender, is_6dof=is_6dof, device=device)
    net = deform.deform
    heads = (net.branch_w, net.branch_v) if is_6dof else (net.gaussian_warp,)
    with torch.no_grad():
        for head in heads + (net.gaussian_rotation, net.gaussian_scaling):
            head.weight.mul_(0.01)
            head.bias.mul_(0.01)
    return deform
