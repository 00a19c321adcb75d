// Fused deformation MLP, fixed-order reduction of the dW slabs into the parameter gradients
// (k_dw_reduce, launch_dw_reduce): shared by the fp32 k_dw and the f16-split k_dws. Included by
// mlp.hip's translation unit only, which thereby defines mlp_shared.h's launch_dw_reduce.
#pragma once
#include <hip/hip_runtime.h>

#include "dgs_common.h"
#include "mlp_shared.h"

namespace dgs {
namespace mlpc {

struct RJob {
    float *dst;        // parameter gradient (rows x cols) or bias (rows)
    int rows, cols;    // cols == 0 -> bias
    int rowpad0;       // padded output row of source row 0 (head stacking)
    int nseg;
    Seg seg[3];        // source col <-> padded feature
    int block0[2];     // first slab of the layer's k-tile 0 / 1 (padded features [0,k1) / [k1,..))
    int nsplit[2];
    int k1;            // padded feature where k-tile 1 starts (WPlan::layer_k1)
};

constexpr int MAXR = 28;
struct RJobs {
    RJob j[MAXR];
    int begin[MAXR + 1];  // element prefix
    int n;
};

// one thread per gradient element of every parameter; sums the splits in a fixed order
// sum of one element over ns slabs in slab order (deterministic): RU loads issued before the adds
// that consume them (one HBM round trip per RU slabs; adding the predicated 0.f is exact)
#ifndef DGS_REDUCE_U
#define DGS_REDUCE_U 8
#endif
__device__ __forceinline__ float slab_sum(const float *sl, int ns) {
    constexpr int RU = DGS_REDUCE_U;
    float s = 0.f;
    for (int b = 0; b < ns; b += RU) {
        float v[RU];
#pragma unroll
        for (int k = 0; k < RU; k++) v[k] = b + k < ns ? sl[(size_t)(b + k) * SLAB] : 0.f;
#pragma unroll
        for (int k = 0; k < RU; k++) s += v[k];
    }
    return s;
}

__global__ __launch_bounds__(256) void k_dw_reduce(RJobs R, const float *__restrict__ slabs) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R.begin[R.n]) return;
    int q = 0;
    while (idx >= R.begin[q + 1]) q++;
    const RJob &J = R.j[q];
    idx -= R.begin[q];
    int r = J.cols ? idx / J.cols : idx;
    int n = J.rowpad0 + r;
    float s = 0.f;
    if (J.cols) {
        int c = idx % J.cols;
        int f = -1;
        for (int k = 0; k < J.nseg; k++)
            if (c >= J.seg[k].s0 && c < J.seg[k].s0 + J.seg[k].len) f = J.seg[k].p0 + (c - J.seg[k].s0);
        if (f < 0) return;  // a folded t_emb column: written by k_tgrad
        const int kt = f >= J.k1 ? 1 : 0, kl = f - (kt ? J.k1 : 0);
        const float *sl = slabs + (size_t)J.block0[kt] * SLAB + n * WT + kl;
        s = slab_sum(sl, J.nsplit[kt]);
    } else {
        const float *sl = slabs + (size_t)J.block0[0] * SLAB + WT * WT + n;
        s = slab_sum(sl, J.nsplit[0]);
    }
    J.dst[idx] = s;
}

int launch_dw_reduce(const Flags &F, const WPlan &W, const float *slabs, float *const *grads, hipStream_t stream) {
    const Params P = make_params(F);
    RJobs R{};
    int total = 0;
    auto add = [&](int pidx, int rowpad0, int ns, const Seg *sg, int layer, bool bias) {
        int r, c;
        param_shape(F, P, pidx, r, c);
        RJob &J = R.j[R.n];
        J.dst = grads[pidx]; J.rows = r; J.cols = bias ? 0 : c; J.rowpad0 = rowpad0; J.nseg = ns;
        for (int q = 0; q < ns; q++) J.seg[q] = sg[q];
        for (int kt = 0; kt < 2; kt++) {
            int jq = W.layer_job[layer][kt];
            J.block0[kt] = jq >= 0 ? W.jobs.j[jq].block0 : 0;
            J.nsplit[kt] = jq >= 0 ? W.jobs.j[jq].nsplit : 0;
        }
        J.k1 = W.layer_k1[layer];
        R.begin[R.n] = total;
        total += bias ? r : r * c;
        R.n++;
    };
    for (int i = 0; i < 8; i++) {
        Seg sg[3];
        int ns = layer_in_segs(F, i, sg);
        add(P.pLw[i], 0, ns, sg, i, false);
        add(P.pLb[i], 0, ns, sg, i, true);
    }
    {
        Seg full = seg(0, 256, 0);
        int r0 = 0;
        for (int hh = 0; hh < P.nheads; hh++) {
            add(P.pHw[hh], r0, 1, &full, 8, false);
            add(P.pHb[hh], r0, 1, &full, 8, true);
            r0 += P.hrows[hh];
        }
        if (F.blender && !F.uniform_t) {  // uniform t: written by the split path's k_tgrad
            Seg st = seg(0, F.tin, 0);
            add(P.pT0w, 0, 1, &st, 9, false);
            add(P.pT0b, 0, 1, &st, 9, true);
            add(P.pT2w, 0, 1, &full, 10, false);
            add(P.pT2b, 0, 1, &full, 10, true);
        }
    }
    R.begin[R.n] = total;
    {
        ScopedTimer tm("mlp_dw_reduce", stream);
        hipLaunchKernelGGL(k_dw_reduce, dim3(div_up(total, 256)), dim3(256), 0, stream, R, slabs);
    }
    DGS_LAUNCH_CHECK("k_dw_reduce", false, stream);
    return DGS_OK;
}

}  // namespace mlpc
}  // namespace dgs
