"""How many of the rect binning's (tile, Gaussian) pairs could binning itself drop (CPU, oracle geometry).

The reference bins every Gaussian into each tile of its 3-sigma square (getRect); the blend kernels
skip, at staging, the pairs whose alpha >= 1/255 ellipse misses every pixel centre of the tile
(raster_blend.h tile_reach). This counts, on the bench scene (synth-100k @ 800x800, camera 0, fid 0.5,
normalized rotations), the pairs that (a) the exact ellipse-vs-tile test and (b) the ellipse's
axis-aligned bounding box would keep. (b) is the only variant that keeps k_rect_place's rank trick
(ranks are popcounts over per-row x per-column lane masks, i.e. rectangles).
usage: python tests/diag/cull_estimate.py [N] [res]
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deformable-3d-gaussians_amd")]

from deformgs.synthetic import synth_camera, synth_gaussians  # noqa: E402
from oracle import raster as orr  # noqa: E402


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    res = int(sys.argv[2]) if len(sys.argv) > 2 else 800
    cpu = torch.device("cpu")
    g = synth_gaussians(N, seed=0, device=cpu)
    cam = synth_camera(res, res, index=0, fid=0.5, device=cpu)
    s = orr.make_settings(res, res, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), np.zeros(3, np.float32), 1.0,
                          cam.world_view_transform.numpy(), cam.full_proj_transform.numpy(), 3,
                          cam.camera_center.numpy())
    shs = torch.cat([g["features_dc"], g["features_rest"]], 1).numpy()
    o = orr.OracleRaster(s, g["xyz"].numpy(), shs=shs, opacities=torch.sigmoid(g["opacity"]).numpy(),
                         scales=torch.exp(g["scaling"]).numpy(),
                         rotations=torch.nn.functional.normalize(g["rotation"]).numpy())
    geo = o.geometry()
    xy, co, rad = geo["xy"].astype(np.float64), geo["conic_opacity"].astype(np.float64), o.radii
    gx, gy = (res + 15) // 16, (res + 15) // 16
    rect = exact = bbox = 0
    for i in np.nonzero(rad > 0)[0]:
        x, y = xy[i]
        R = rad[i]
        x0, x1 = min(gx, max(0, int((x - R) // 16))), min(gx, max(0, int((x + R + 15) // 16)))
        y0, y1 = min(gy, max(0, int((y - R) // 16))), min(gy, max(0, int((y + R + 15) // 16)))
        if x1 <= x0 or y1 <= y0:
            continue
        rect += (x1 - x0) * (y1 - y0)
        a, b, c, op = co[i]
        if op < 1.0 / 255.0:
            continue
        thr = 2.0 * math.log(255.0 * op)
        det = a * c - b * b
        hx, hy = math.sqrt(thr * c / det), math.sqrt(thr * a / det)  # the ellipse's half extents
        bx0, bx1 = max(x0, int(math.floor((x - hx) / 16))), min(x1, int(math.floor((x + hx) / 16)) + 1)
        by0, by1 = max(y0, int(math.floor((y - hy) / 16))), min(y1, int(math.floor((y + hy) / 16)) + 1)
        bbox += max(0, bx1 - bx0) * max(0, by1 - by0)
        X, Y = np.meshgrid(np.arange(x0 * 16, x1 * 16) - x, np.arange(y0 * 16, y1 * 16) - y)
        reach = (a * X * X + 2 * b * X * Y + c * Y * Y) <= thr
        exact += int(reach.reshape(y1 - y0, 16, x1 - x0, 16).any(axis=(1, 3)).sum())
    print(f"num_rendered {o.num_rendered}: rect pairs {rect}, exact ellipse-tile {exact} ({exact / rect:.3f}), "
          f"ellipse bbox {bbox} ({bbox / rect:.3f})")


if __name__ == "__main__":
    main()
