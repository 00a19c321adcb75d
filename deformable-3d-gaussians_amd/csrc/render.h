// The rasterizer side of dgs_render_frames (render.hip), implemented in raster.hip next to the binning
// driver it shares with the training forward (the kernels: raster_preprocess.h, raster_bin.h, raster_blend.h).
#pragma once
#include "dgs_common.h"

namespace dgs {

struct RenderWs;  // per-device forward-only workspace (geometry, binning, pair-count slots, depth maxima)

struct RenderRasterIn {
    int P, H, W, sh_degree;
    float scale_modifier, tanfovx, tanfovy;
    const float *means3D, *f_dc, *f_rest, *opacities, *scales, *rotations;
    const float *bg, *viewmatrix, *projmatrix, *campos;
    // this frame's outputs (any may be null)
    float *color, *depth, *alpha;
    uint8_t *rgb8, *depth8;
};

// Takes the device's workspace for one dgs_render_frames call of F frames (held until render_ws_release;
// calls on one device serialise), with F count slots and an H x W depth scratch (the per-Gaussian buffers
// are sized by render_raster_frame); `stream` is ordered after the workspace's previous user. need_depth:
// depth8 is wanted without a float depth output.
int render_ws_acquire(int F, int H, int W, bool need_depth, hipStream_t stream, RenderWs **ws);
void render_ws_release(RenderWs *ws, hipStream_t stream);
// Enqueues frame f: preprocess, pair count (into the frame's host slot), binning, k_blend_img, k_depth8.
// known_count < 0: bin for the learned capacity (without one: wait for this frame's count and bin at the
// exact size); >= 0: a redo at that exact size (no host wait, the host slot is left alone).
int render_raster_frame(RenderWs *ws, const RenderRasterIn &in, int f, int known_count, hipStream_t stream);
// The call's one host wait: returns once every enqueued frame's pair count is in its slot.
int render_wait_counts(RenderWs *ws, hipStream_t stream);
int render_frame_count(const RenderWs *ws, int f);  // after render_wait_counts
int render_frame_cap(const RenderWs *ws, int f);    // the capacity frame f was binned with
// feeds frame f's count to the learned capacity (pair_cap_observe) unless its synchronous wait already did
void render_observe_count(const RenderWs *ws, int f, int nr);

}  // namespace dgs
