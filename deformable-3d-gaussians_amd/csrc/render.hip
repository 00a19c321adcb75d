// F frames of one model in one C call, forward only: dgs_render_frames (include/dgs.h).
//
// The counterpart of render_baseline.py's render loops (render_set and the interpolate_* variants,
// render_baseline.py:57-66 per frame: deform.step(xyz, fid) -> render()): per frame the deformation
// network's inference forward, the render-input glue and the forward-only rasterizer (raster.hip's
// render_raster_frame: raster_preprocess.h k_preprocess<., true>, the training forward's binning,
// raster_blend.h k_blend_img and k_depth8), all enqueued on one
// stream without a host wait in between.
//
// Host waits per call: one, for the last frame's pair count at the end (render_wait_counts), plus one
// for the first frame when the device has no learned pair capacity yet. A frame whose count exceeded the
// capacity it was binned with rendered from truncated tile lists; its scratch (network output, render
// inputs, geometry) has been reused by the frames after it, so it is redone from the deformation on, at
// its exact size, after the wait.
#include <hip/hip_runtime.h>

#include "dgs_common.h"
#include "render.h"

namespace dgs {
namespace {

__global__ void k_fill_time(int n, const float *__restrict__ v, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v[0];
}

constexpr int M_REST = 15;

int bad(const char *msg) {
    set_error(std::string("dgs_render_frames: ") + msg);
    return DGS_ERR_ARGS;
}

// one frame: deformation -> input glue -> forward-only rasterizer
int frame(const dgs_render_frames_args *a, RenderWs *ws, int f, int known_count, hipStream_t stream) {
    const int P = a->P;
    const bool warm = a->deform != 0;
    const bool six = (a->mlp_flags & DGS_MLP_6DOF) != 0;
    const int nout = dgs_deform_outputs(a->mlp_flags);
    const size_t HW = (size_t)a->H * a->W;
    if (P > 0) {
        if (warm) {
            // the flags DeformNetwork.raw passes for a stride-0 expanded t under no_grad; the split path of a
            // blender network reads t[0] only (k_timenet), every other kernel a column of P values
            const float *t = a->t + f;
            if (!(a->mlp_flags & DGS_MLP_BLENDER) || (a->mlp_flags & DGS_MLP_EXACT_FP32)) {
                hipLaunchKernelGGL(k_fill_time, dim3(div_up(P, 256)), dim3(256), 0, stream, P, t, a->t_full);
                DGS_LAUNCH_CHECK("k_fill_time", false, stream);
                t = a->t_full;
            }
            if (int rc = dgs_deform_forward(a->mlp_flags | DGS_MLP_UNIFORM_T, P, a->xyz, t, a->mlp_packed, a->mlp_out,
                                            nullptr, stream))
                return rc;
        }
        const float *rows = warm ? a->mlp_out : nullptr;
        const int rc = warm && six
                           ? dgs_gaussian_inputs_se3_forward(P, M_REST, a->xyz, a->f_dc, a->f_rest, a->scaling,
                                                             a->rotation, a->opacity, rows, nout, a->means3D, nullptr,
                                                             a->scales, a->rotations, a->opacities, stream)
                           : dgs_gaussian_inputs_forward(P, M_REST, a->xyz, a->f_dc, a->f_rest, a->scaling, a->rotation,
                                                         a->opacity, rows, warm ? nout : 0, a->means3D, nullptr,
                                                         a->scales, a->rotations, a->opacities, stream);
        if (rc) return rc;
    }
    const dgs_frame &fr = a->frames[f];
    RenderRasterIn in{};
    in.P = P; in.H = a->H; in.W = a->W; in.sh_degree = a->sh_degree;
    in.scale_modifier = a->scale_modifier; in.tanfovx = fr.tanfovx; in.tanfovy = fr.tanfovy;
    in.means3D = a->means3D; in.f_dc = a->f_dc; in.f_rest = a->f_rest; in.opacities = a->opacities;
    in.scales = a->scales; in.rotations = a->rotations;
    in.bg = a->bg; in.viewmatrix = fr.viewmatrix; in.projmatrix = fr.projmatrix; in.campos = fr.campos;
    in.color = a->out_color ? a->out_color + 3 * HW * f : nullptr;
    in.depth = a->out_depth ? a->out_depth + HW * f : nullptr;
    in.alpha = a->out_alpha ? a->out_alpha + HW * f : nullptr;
    in.rgb8 = a->out_rgb8 ? a->out_rgb8 + 3 * HW * f : nullptr;
    in.depth8 = a->out_depth8 ? a->out_depth8 + HW * f : nullptr;
    return render_raster_frame(ws, in, f, known_count, stream);
}

}  // namespace
}  // namespace dgs

extern "C" int dgs_render_frames(const dgs_render_frames_args *a, int *redone_frames, void *stream_) {
    using namespace dgs;
    hipStream_t stream = (hipStream_t)stream_;
    if (redone_frames) *redone_frames = 0;
    if (!a) return bad("null argument block");
    if (a->P < 0 || a->F < 0) return bad("negative P or F");
    if (a->H <= 0 || a->W <= 0) return bad("empty image");
    if (!a->out_color && !a->out_depth && !a->out_alpha && !a->out_rgb8 && !a->out_depth8)
        return bad("no output requested (every out_* pointer is NULL)");
    if (a->sh_degree < 0 || a->sh_degree > 3) return bad("SH degree unsupported (0..3)");
    if (a->F > 0 && (!a->frames || !a->bg)) return bad("frames / bg missing");
    for (int f = 0; f < a->F; f++)
        if (!a->frames[f].viewmatrix || !a->frames[f].projmatrix || !a->frames[f].campos)
            return bad("a frame's camera pointer is NULL");
    if (a->P > 0) {
        if (!a->xyz || !a->f_dc || !a->f_rest || !a->scaling || !a->rotation || !a->opacity || !a->means3D ||
            !a->scales || !a->rotations || !a->opacities)
            return bad("null Gaussian parameter or render-input scratch pointer");
        if ((reinterpret_cast<uintptr_t>(a->f_dc) | reinterpret_cast<uintptr_t>(a->f_rest)) & 15)
            return bad("features_dc / features_rest must be 16-byte aligned");
        if (a->deform) {
            if (!a->mlp_packed || !a->mlp_out || !a->t)
                return bad("the deformation network needs mlp_packed, mlp_out and t");
            if ((!(a->mlp_flags & DGS_MLP_BLENDER) || (a->mlp_flags & DGS_MLP_EXACT_FP32)) && !a->t_full)
                return bad("t_full (P floats) is needed by this network's kernels");
            if (a->mlp_flags & DGS_MLP_NO_ROTSCALE)
                return bad("the network without rotation / scaling heads is not covered by the fused input glue");
        }
    }
    if (a->F == 0) return DGS_OK;
    RenderWs *ws = nullptr;
    if (int rc = render_ws_acquire(a->F, a->H, a->W, a->out_depth8 && !a->out_depth, stream, &ws)) return rc;
    int rc = DGS_OK, redone = 0;
    for (int f = 0; f < a->F && !rc; f++) rc = frame(a, ws, f, -1, stream);
    // the call's one host wait; after a failure too (result ignored), so that no enqueued frame can still be
    // about to write its host count word once the workspace is released
    if (rc)
        (void)render_wait_counts(ws, stream);
    else
        rc = render_wait_counts(ws, stream);
    if (!rc) {
        for (int f = 0; f < a->F && !rc; f++) {
            const int nr = a->P > 0 ? render_frame_count(ws, f) : 0;
            if (a->num_rendered) a->num_rendered[f] = nr;
            if (a->P == 0) continue;
            render_observe_count(ws, f, nr);
            if (nr > render_frame_cap(ws, f)) {
                redone++;
                rc = frame(a, ws, f, nr, stream);
            }
        }
    }
    render_ws_release(ws, stream);
    if (redone_frames) *redone_frames = redone;
    return rc;
}
