// Fused deformation MLP (positional encoding + timenet + 8x256 trunk with skip + heads) on fp32
// MFMA (v_mfma_f32_32x32x2_f32: exact fp32 fma chains) for MI355X / gfx950.
//
// Replaces DeformNetworkBaseline.forward and its autograd backward (utils/time_utils.py:56-127;
// DeformNetwork :129-201 via DGS_MLP_NO_ROTSCALE; 6-DoF heads :114-121 emitted raw, exp_se3 stays
// in the host glue). Default and only supported shape: D=8, W=256, multires=10, skips=[4]
// (arguments/__init__.py:65-68 and every arguments/*.py config).
//
// Layout ("transposed" formulation, Y^T = W X^T): features on MFMA rows, points on MFMA columns.
// One workgroup = 32 points x 8 waves; wave w owns output rows 32w..32w+31 of every 256-wide layer,
// so every weight fragment is read once per workgroup. 78 KiB of LDS: two workgroups share a CU.
//  * Activations live in LDS as [feature/4][32 points][4] (16-byte units; a group = 4 features x 32
//    points = 512 B): the B operand of a k-step is one ds_read_b128 per lane, and the 32x32
//    accumulator rows (8j + 4h + 0..3) of a layer are exactly one ds_write_b128 into the next
//    layer's input image (no shuffles).
//    LDS groups (mlp_fp32_core.h): XE 0-15 | TE 16-23 | H 24-87 | TIN 88-91 | PART 92-155 (8 K-part
//    slots of 8 groups), G_TOTAL = 156; XE|TE|H contiguous makes cat(x_emb, t_emb) and
//    cat(x_emb, t_emb, h) plain ranges.
//  * Weights are re-packed every call (they change every optimizer step) into MFMA A-fragment
//    order [n-tile][8-feature chunk][64 lanes][4] so each wave-load is 1 KiB contiguous.
//  * Narrow layers (timenet.2, heads, and the t_emb slices of the backward) split K over the 8
//    waves and sum their partials in a fixed order (deterministic, no LDS atomics).
//  * Forward saves every layer's input activations feature-major [F][Ns] (coalesced from the
//    accumulator layout); backward dX saves every dZ the same way; dW = dZ X^T is a separate
//    split-N MFMA GEMM + fixed-order slab reduction (deterministic).
//
// Files. This is the only translation unit: it holds the host side (packing plan and map, pack,
// forward, backward, the size functions, dw_fp32) and k_pack_map; the device code is in
//   mlp_fp32_core.h   LDS map, gemm<NCH>, the prologue / stash hooks, narrow-layer pieces
//   mlp_fp32_fwd.h    k_timenet, k_mlp_fwd<SAVE>
//   mlp_fp32_bwd.h    k_mlp_bwd (dX chain)
//   mlp_dw_fp32.h     k_dw (also the f16-split path's dW fallback)
//   mlp_dw_reduce.h   k_dw_reduce, launch_dw_reduce (namespace mlpc: every training step of both paths)
// and mlp_shared.h holds what the f16-split path (mlp_split.hip) shares.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "dgs_common.h"
#include "mlp_shared.h"
#include "mlp_fp32_core.h"
#include "mlp_fp32_fwd.h"
#include "mlp_fp32_bwd.h"
#include "mlp_dw_fp32.h"
#include "mlp_dw_reduce.h"

namespace dgs {
namespace mlp {

// ------------------------------------------------------------------------------------------------
// packing plan (host): which A-operand images exist and where
// ------------------------------------------------------------------------------------------------
struct PackJob {
    int src;            // parameter index (weight)
    int transpose;      // 0: A[n][f] = W[n][f]; 1: A[n][f] = W[f][n] (n over input features)
    int ntiles, nchunks;
    int nseg_n, nseg_f;
    Seg segn[3], segf[3];
    int off;            // float offset in packed buffer
};
struct BiasJob {
    int src;            // parameter index (bias)
    int npad;
    int nseg;
    Seg seg[3];
    int off;
};

struct Plan : Params {
    Flags F;
    std::vector<PackJob> jobs;
    std::vector<BiasJob> biases;
    FwdOffsets fwd;  // forward A images and padded biases
    BwdOffsets bwd;  // backward A images (transposed)
    int total;
};

Plan make_plan(int flags) {
    Plan P;
    P.F = make_flags(flags);
    const Flags &F = P.F;
    static_cast<Params &>(P) = make_params(F);
    int off = 0;
    auto add_job = [&](int src, int tr, int ntiles, int nchunks, int nsn, const Seg *sn, int nsf, const Seg *sf) {
        PackJob j{};
        j.src = src; j.transpose = tr; j.ntiles = ntiles; j.nchunks = nchunks;
        j.nseg_n = nsn; j.nseg_f = nsf;
        for (int q = 0; q < nsn; q++) j.segn[q] = sn[q];
        for (int q = 0; q < nsf; q++) j.segf[q] = sf[q];
        j.off = off;
        off += ntiles * nchunks * 256;
        P.jobs.push_back(j);
        return j.off;
    };
    auto add_bias = [&](int src, int npad, int ns, const Seg *s) {
        BiasJob b{};
        b.src = src; b.npad = npad; b.nseg = ns;
        for (int q = 0; q < ns; q++) b.seg[q] = s[q];
        b.off = off;
        off += npad;
        P.biases.push_back(b);
        return b.off;
    };
    Seg full256 = seg(0, 256, 0);
    if (F.blender) {
        Seg sf = seg(0, F.tin, 0);
        P.fwd.fT1 = add_job(P.pT0w, 0, 8, 2, 1, &full256, 1, &sf);
        Seg sn = seg(0, 30, 0);
        P.fwd.fT2 = add_job(P.pT2w, 0, 1, 32, 1, &sn, 1, &full256);
        P.fwd.bT1 = add_bias(P.pT0b, 256, 1, &full256);
        P.fwd.bT2 = add_bias(P.pT2b, 32, 1, &sn);
        // backward: A[n = TH feature][f = TE feature] = W_T2[f][n]
        P.bwd.tT2 = add_job(P.pT2w, 1, 8, 4, 1, &full256, 1, &sn);
    } else {
        P.fwd.fT1 = P.fwd.fT2 = P.fwd.bT1 = P.fwd.bT2 = P.bwd.tT2 = -1;
    }
    for (int i = 0; i < 8; i++) {
        Seg s[3];
        int ns = layer_in_segs(F, i, s);
        int kp = layer_kpad(i);
        P.fwd.fL[i] = add_job(P.pLw[i], 0, 8, kp / 8, 1, &full256, ns, s);
        P.fwd.bL[i] = add_bias(P.pLb[i], 256, 1, &full256);
        // backward image: rows = padded input features (kp), contraction over the 256 outputs
        P.bwd.tL[i] = add_job(P.pLw[i], 1, kp / 32, 32, ns, s, 1, &full256);
    }
    // heads: rows stacked in output order
    {
        // one job per head linear writing into row ranges of one 32-row tile: emulate by segments
        // on n with distinct sources is not expressible (different src params) -> pack per head.
        int base = off;
        off += 1 * 32 * 256;  // forward image, 1 n-tile x 32 chunks
        int tbase = off;
        off += 8 * 4 * 256;   // transposed image, 8 tiles x 4 chunks
        int bbase = off;
        off += 32;
        int r0 = 0;
        for (int h = 0; h < P.nheads; h++) {
            PackJob j{};
            j.src = P.pHw[h]; j.transpose = 0; j.ntiles = 1; j.nchunks = 32;
            j.nseg_n = 1; j.segn[0] = seg(r0, P.hrows[h], 0);
            j.nseg_f = 1; j.segf[0] = full256;
            j.off = base;
            P.jobs.push_back(j);
            PackJob t{};
            t.src = P.pHw[h]; t.transpose = 1; t.ntiles = 8; t.nchunks = 4;
            t.nseg_n = 1; t.segn[0] = full256;
            t.nseg_f = 1; t.segf[0] = seg(r0, P.hrows[h], 0);
            t.off = tbase;
            P.jobs.push_back(t);
            BiasJob b{};
            b.src = P.pHb[h]; b.npad = 32; b.nseg = 1; b.seg[0] = seg(r0, P.hrows[h], 0);
            b.off = bbase;
            P.biases.push_back(b);
            r0 += P.hrows[h];
        }
        P.fwd.fHd = base;
        P.bwd.tHd = tbase;
        P.fwd.bHd = bbase;
    }
    P.total = off;
    return P;
}

// Packing is one gather launch: map[i] = (parameter << 22) | element for packed float i, or -1 for
// zero padding. The map depends only on the flags (built once on the host, cached on the device).
constexpr int PACK_MAXP = 32;
constexpr int PACK_SHIFT = 22;
struct PackPtrs {
    const float *p[PACK_MAXP];
};

__global__ __launch_bounds__(256) void k_pack_map(const int *__restrict__ map, PackPtrs src, float *__restrict__ packed,
                                                  int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = map[i];
    packed[i] = c < 0 ? 0.f : src.p[c >> PACK_SHIFT][c & ((1 << PACK_SHIFT) - 1)];
}

// fp32 dW split plan: per-chunk cost units calibrated with tools/dw_phase.cpp (full 256 x 256 tile
// 16 + 1.5 units ~ 18.9k cycles, narrow 6 + 1.5 ~ 8.3k, 32-row jobs ~ 4.2k); one 8-wave workgroup per
// CU (LDS 147 KiB)
static WPlan fp32_wplan(const Flags &F) { return make_wplan(F, 256, 1.5, 4.0); }

static size_t padded_points(int N) { return (size_t)div_up(N, BM) * BM; }

size_t packed_floats(int flags) { return (size_t)make_plan(flags).total; }
// saved activations [nsaved][Ns] floats, then the relu' bits [Ns / 32 blocks][nmask] u32 words, then
// the frame-uniform timenet values (TC_FLOATS)
size_t saved_floats(int flags, int N) {
    const Flags F = make_flags(flags);
    return (size_t)F.nsaved * padded_points(N) + (size_t)F.nmask * (padded_points(N) / BM) + TC_FLOATS;
}

size_t scratch_floats(int flags, int N) {
    Flags F = make_flags(flags);
    WPlan W = fp32_wplan(F);
    return (size_t)F.nz * padded_points(N) + (size_t)W.nblocks * SLAB;
}

// host emulation of the packed-image layout (forward A images, transposed backward images, biases)
static std::vector<int> build_pack_map(const Plan &P) {
    std::vector<int> map((size_t)P.total, -1);
    for (const PackJob &j : P.jobs) {
        int r, c;
        param_shape(P.F, P, j.src, r, c);
        const bool head = (j.off == P.fwd.fHd || j.off == P.bwd.tHd);  // head images are shared by several jobs
        const int total = j.ntiles * j.nchunks * 256;
        for (int idx = 0; idx < total; idx++) {
            int t = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8;
            int chunk = rest % j.nchunks, ntile = rest / j.nchunks;
            int n = ntile * 32 + (lane & 31);
            int f = chunk * 8 + 4 * (lane >> 5) + t;
            int sn = seg_lookup(j.segn, j.nseg_n, n);
            int sf = seg_lookup(j.segf, j.nseg_f, f);
            bool mine = j.transpose ? (sf >= 0) : (sn >= 0);
            int code = -1;
            if (sn >= 0 && sf >= 0) code = (j.src << PACK_SHIFT) | (j.transpose ? sf * c + sn : sn * c + sf);
            if (mine || !head) map[(size_t)j.off + idx] = code;
        }
    }
    for (const BiasJob &b : P.biases)
        for (int n = 0; n < b.npad; n++) {
            int sidx = seg_lookup(b.seg, b.nseg, n);
            if (sidx >= 0) map[(size_t)b.off + n] = (b.src << PACK_SHIFT) | sidx;
            else if (b.off != P.fwd.bHd) map[(size_t)b.off + n] = -1;
        }
    return map;
}

static std::mutex g_map_mu;
static std::map<std::pair<int, int>, int *> g_pack_maps;  // (device, flags) -> device map

static int *pack_map_for(const Plan &P, int flags) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_map_mu);
    auto it = g_pack_maps.find({dev, flags});
    if (it != g_pack_maps.end()) return it->second;
    std::vector<int> h = build_pack_map(P);
    int *d = nullptr;
    if (hipMalloc(&d, h.size() * sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    g_pack_maps[{dev, flags}] = d;
    return d;
}

int pack(int flags, const float *const *params, float *packed, hipStream_t stream) {
    Plan P = make_plan(flags);
    if (P.nparams > PACK_MAXP) {
        set_error("dgs_deform_pack: too many parameters");
        return DGS_ERR_ARGS;
    }
    PackPtrs src{};
    for (int k = 0; k < P.nparams; k++) {
        if (!params[k]) {
            set_error("dgs_deform_pack: null parameter pointer");
            return DGS_ERR_ARGS;
        }
        src.p[k] = params[k];
    }
    const int *map = pack_map_for(P, flags);
    if (!map) {
        set_error("dgs_deform_pack: could not allocate the pack map");
        return DGS_ERR_HIP;
    }
    hipLaunchKernelGGL(k_pack_map, dim3(div_up(P.total, 256)), dim3(256), 0, stream, map, src, packed, P.total);
    DGS_LAUNCH_CHECK("k_pack_map", false, stream);
    return DGS_OK;
}

int forward(int flags, int N, const float *xyz, const float *t, const float *packed, float *out, float *saved,
            hipStream_t stream) {
    if (N < 0 || (N > 0 && (!xyz || !t || !packed || !out))) {
        set_error("dgs_deform_forward: null argument");
        return DGS_ERR_ARGS;
    }
    if (N == 0) return DGS_OK;
    Plan P = make_plan(flags);
    FwdArgs a{};
    a.N = N;
    a.Ns = padded_points(N);
    a.xyz = xyz; a.t = t; a.packed = packed; a.out = out; a.saved = saved;
    a.mask = saved ? reinterpret_cast<uint32_t *>(saved + (size_t)P.F.nsaved * a.Ns) : nullptr;
    a.o = P.fwd;
    a.flags = flags;
    {
        ScopedTimer tm("mlp_fwd", stream);
        if (saved && P.F.blender) {
            a.tc = saved + (size_t)P.F.nsaved * a.Ns + (size_t)P.F.nmask * (a.Ns / BM);
            hipLaunchKernelGGL(k_timenet, dim3(1), dim3(256), 0, stream, a);
        }
        hipLaunchKernelGGL(saved ? k_mlp_fwd<true> : k_mlp_fwd<false>, dim3(div_up(N, BM)), dim3(NTHR), 0, stream, a);
    }
    DGS_LAUNCH_CHECK("k_mlp_fwd", false, stream);
    return DGS_OK;
}

int backward(int flags, int N, const float *packed, const float *saved, const float *dout, float *scratch,
             float *const *grads, hipStream_t stream) {
    if (N < 0 || (N > 0 && (!packed || !saved || !dout || !scratch || !grads))) {
        set_error("dgs_deform_backward: null argument");
        return DGS_ERR_ARGS;
    }
    Plan P = make_plan(flags);
    const Flags &F = P.F;
    if (N == 0) {
        for (int k = 0; k < P.nparams; k++) {
            int r, c;
            param_shape(F, P, k, r, c);
            DGS_HIP_CHECK(hipMemsetAsync(grads[k], 0, sizeof(float) * r * (c ? c : 1), stream));
        }
        return DGS_OK;
    }
    const size_t Ns = padded_points(N);
    float *dz = scratch;
    float *slabs = scratch + (size_t)F.nz * Ns;
    BwdArgs b{};
    b.N = N; b.Ns = Ns; b.packed = packed; b.saved = saved; b.dout = dout; b.dz = dz;
    b.mask = reinterpret_cast<const uint32_t *>(saved + (size_t)F.nsaved * Ns);
    b.o = P.bwd;
    b.flags = flags;
    {
        ScopedTimer tm("mlp_bwd", stream);
        hipLaunchKernelGGL(k_mlp_bwd, dim3(div_up(N, BM)), dim3(NTHR), 0, stream, b);
    }
    DGS_LAUNCH_CHECK("k_mlp_bwd", false, stream);
    return dw_fp32(F, Ns, dz, saved, slabs, grads, stream);
}

// dW on fp32-input MFMA (k_dw) + the fixed-order slab reduction; shared with the f16-split path,
// whose dZ / saved-activation arrays have the same [rows][Ns] layout (Ns a multiple of 32)
size_t dw_fp32_slab_floats(int flags) { return (size_t)fp32_wplan(make_flags(flags)).nblocks * SLAB; }

int dw_fp32(const Flags &F, size_t Ns, const float *dz, const float *saved, float *slabs, float *const *grads,
            hipStream_t stream) {
    WPlan W = fp32_wplan(F);
    {
        const size_t lds_bytes = sizeof(float) * 2 * 2 * WT * LDA;
        // 147 KiB dynamic LDS: the attribute is per device, set once per (kernel, device)
        if (int rc = ensure_dynamic_lds((const void *)k_dw, (int)lds_bytes)) return rc;
        ScopedTimer tm("mlp_dw", stream);
        hipLaunchKernelGGL(k_dw, dim3(W.nblocks), dim3(DW_THREADS), lds_bytes, stream, W.jobs, Ns, dz, saved, slabs);
    }
    DGS_LAUNCH_CHECK("k_dw", false, stream);
    return launch_dw_reduce(F, W, slabs, grads, stream);
}

}  // namespace mlp
}  // namespace dgs

#ifdef DGS_MLP_PROFILE
extern "C" void dgs_mlp_set_prof(unsigned long long *p) {
    (void)hipMemcpyToSymbol(HIP_SYMBOL(dgs::mlp::dgs_mlp_prof), &p, sizeof(p));
}
#endif
