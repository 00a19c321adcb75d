// Fused deformation MLP, dW on fp32-input MFMA (device code of mlp.hip's translation unit): k_dw.
// The exact path's dW and the f16-split path's fallback (mlp::dw_fp32).
#pragma once
#include "mlp_fp32_core.h"

namespace dgs {
namespace mlp {

// dW = dZ X^T over all points: one 256x256 tile per layer (L5: 256 + 96 input columns), split over
// the point axis in proportion to each tile's work so ~one workgroup per CU finishes together;
// fixed-order slab reduction (mlp_dw_reduce.h; deterministic).
constexpr int PC = 32;             // points per LDS chunk
constexpr int LDA = PC + 4;        // padded LDS row (floats)
constexpr int DW_THREADS = 512;    // 8 waves: 2 (n) x 4 (k), 128 x 64 per wave

#ifdef DGS_MLP_PROFILE  // diagnostic build only (tools/dw_phase.cpp): per-chunk s_memtime stamps of k_dw
__device__ unsigned long long *dgs_mlp_prof;
#endif

// component-wise select (a select of the float4 struct itself can be lowered through scratch)
__device__ inline float4 zsel4(float4 v, bool ok) {
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// Staging of one operand (256 rows x 32 points) by the 512 threads: thread -> row srow + 64 j
// (j < 4), float4 column scol. o[j] = float offset of that row from the operand's base, or -1 for a
// row past the job's extent.
//   Rows past the extent load row 0 (always valid) and are zeroed at the LDS store (after the chunk's
// MFMAs, so the loads stay in flight across them): an unconditional global_load keeps hipcc from
// turning `ok ? *p : 0` into a flat load of a pointer select between global memory and a
// scratch-held zero.
//   32-bit byte offsets from a uniform base -> global_load with an SGPR base (saddr) and one offset
// VGPR per load instead of a 64-bit address pair.
__device__ __forceinline__ void dw_offsets(int (&o)[4], uint32_t (&u)[4], int lim, int srow, int scol, int ns) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        o[j] = srow + 64 * j < lim ? (srow + 64 * j) * ns + scol : -1;
        u[j] = (uint32_t)((o[j] >= 0 ? o[j] : scol) * 4);
    }
}

__device__ __forceinline__ void dw_gload(float4 (&r)[4], const float *base, const uint32_t (&u)[4], int po) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        r[j] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(base) + (uint32_t)(u[j] + (uint32_t)po * 4u));
}

__device__ __forceinline__ void dw_lstore(float *dst, const float4 (&r)[4], const int (&o)[4], int srow, int scol) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        *reinterpret_cast<float4 *>(dst + (srow + 64 * j) * LDA + scol) = zsel4(r[j], o[j] >= 0);
}

// one 32 x 32 accumulator tile -> slab rows nb.., columns kb..
__device__ __forceinline__ void slab_store(float *slab, const f32x16 &acc, int nb, int kb, int h, int i) {
#pragma unroll
    for (int r = 0; r < 16; r++) slab[(nb + 8 * (r >> 2) + 4 * h + (r & 3)) * WT + kb + i] = acc[r];
}

// bias row sums of rows nb..nb + 31 (lanes l and l + 32 hold the same row) -> the slab's last row
__device__ __forceinline__ void bias_sum_store(float *slab, float bs, int nb, int h, int i) {
    const float v = bs + __shfl_xor(bs, 32);
    if (h == 0) slab[WT * WT + nb + i] = v;
}

template <bool NARROW>
__device__ __forceinline__ void dw_tile(const WJob &J, size_t Ns, const float *__restrict__ dz,
                                        const float *__restrict__ saved, float *__restrict__ slabs,
                                        float *ldsf) {
    const int split = blockIdx.x - J.block0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (scalar branches)
    const int wn = wave >> 2, wk = wave & 3;  // wide wave tile: rows [128 wn, +128), cols [64 wk, +64)
    const int h = lane >> 5, i = lane & 31;
    const int nch = (int)(Ns / PC);
    const int per = div_up(nch, J.nsplit);
    const int c0 = split * per;
    const int c1 = min(nch, c0 + per);
    const float *baseA = dz + (size_t)J.zrow * Ns;
    const float *baseB = saved + (size_t)J.xrow * Ns;
    const int ns = (int)Ns;  // 256 rows x Ns < 2^31
    const int srow = tid >> 3, scol = (tid & 7) * 4;
    int oA[4], oB[4];
    uint32_t uA[4], uB[4];
    dw_offsets(oA, uA, J.nrows, srow, scol, ns);
    dw_offsets(oB, uB, J.krows, srow, scol, ns);
    float4 ra[4], rb[4];
    auto gload = [&](int c) { dw_gload(ra, baseA, uA, c * PC), dw_gload(rb, baseB, uB, c * PC); };
    auto lstore = [&](int buf) {
        dw_lstore(ldsf + buf * (2 * WT * LDA), ra, oA, srow, scol);
        dw_lstore(ldsf + buf * (2 * WT * LDA) + WT * LDA, rb, oB, srow, scol);
    };
    // this wave's active sub-tiles (wave-uniform). wide: rows 128 wn + 32 t, cols 64 wk + 32 u
    // (acc[t][u]); narrow: rows 32 wave, cols 32 v (acc[v >> 1][v & 1], v < 4)
    constexpr bool narrow = NARROW;
    const int nact_r = narrow ? (32 * wave < J.nrows ? 1 : 0) : min(4, max(0, div_up(J.nrows - 128 * wn, 32)));
    const int nact_c = narrow ? min(4, div_up(J.krows, 32)) : min(2, max(0, div_up(J.krows - 64 * wk, 32)));
    const bool any = nact_r > 0 && nact_c > 0;
    f32x16 acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        acc[t][0] = zero16();
        acc[t][1] = zero16();
    }
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 < c1) {
        gload(c0);
        lstore(0);
    }
    __syncthreads();
    for (int c = c0; c < c1; c++) {
        const int buf = (c - c0) & 1;
        const bool more = c + 1 < c1;
        if (more) gload(c + 1);
        const float *A = ldsf + buf * (2 * WT * LDA);
        const float *B = A + WT * LDA;
        if (any && narrow) {
#pragma unroll
            for (int g = 0; g < PC / 8; g++) {
                const int o = 8 * g + 4 * h;
                const float4 a0 = *reinterpret_cast<const float4 *>(A + (32 * wave + i) * LDA + o);
                float4 bb[4];
#pragma unroll
                for (int v = 0; v < 4; v++) bb[v] = *reinterpret_cast<const float4 *>(B + (32 * v + i) * LDA + o);
                bs[0] += (a0.x + a0.y) + (a0.z + a0.w);
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    if (v >= nact_c) continue;
                    mfma4(acc[v >> 1][v & 1], a0, bb[v]);
                }
            }
        } else if (any) {
#pragma unroll
            for (int g = 0; g < PC / 8; g++) {
                const int o = 8 * g + 4 * h;
                float4 a[4], bb[2];
#pragma unroll
                for (int t = 0; t < 4; t++) a[t] = *reinterpret_cast<const float4 *>(A + (128 * wn + 32 * t + i) * LDA + o);
#pragma unroll
                for (int u = 0; u < 2; u++) bb[u] = *reinterpret_cast<const float4 *>(B + (64 * wk + 32 * u + i) * LDA + o);
                if (wk == 0) {
#pragma unroll
                    for (int t = 0; t < 4; t++) bs[t] += (a[t].x + a[t].y) + (a[t].z + a[t].w);
                }
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (t >= nact_r) continue;
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        if (u >= nact_c) continue;
                        mfma4(acc[t][u], a[t], bb[u]);
                    }
                }
            }
        }
#ifdef DGS_MLP_PROFILE
        if ((c - c0) >= 4 && (c - c0) < 8 && (tid & 63) == 0)
            dgs_mlp_prof[blockIdx.x * 256 + 64 + ((c - c0) - 4) * 16 + wave] = __builtin_amdgcn_s_memtime();
#endif
        if (more) lstore(buf ^ 1);
        __syncthreads();
#ifdef DGS_MLP_PROFILE
        if ((c - c0) >= 3 && (c - c0) < 8 && tid == 0)
            dgs_mlp_prof[blockIdx.x * 256 + 160 + ((c - c0) - 3)] = __builtin_amdgcn_s_memtime();
#endif
    }
    // rows past nrows / cols past krows hold zeros or partial garbage that k_dw_reduce never reads
    float *slab = slabs + (size_t)blockIdx.x * SLAB;
    if (narrow) {
#pragma unroll
        for (int v = 0; v < 4; v++) slab_store(slab, acc[v >> 1][v & 1], 32 * wave, 32 * v, h, i);
        bias_sum_store(slab, bs[0], 32 * wave, h, i);
        return;
    }
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int u = 0; u < 2; u++) slab_store(slab, acc[t][u], 128 * wn + 32 * t, 64 * wk + 32 * u, h, i);
    if (wk == 0) {
#pragma unroll
        for (int t = 0; t < 4; t++) bias_sum_store(slab, bs[t], 128 * wn + 32 * t, h, i);
    }
}

__global__ __launch_bounds__(DW_THREADS) void k_dw(WJobs JT, size_t Ns, const float *__restrict__ dz,
                                                   const float *__restrict__ saved, float *__restrict__ slabs) {
    extern __shared__ float4 dw_lds[];
    // job of this workgroup: static-index selects over the kernel-argument table (no scratch copy)
    WJob J = JT.j[0];
#pragma unroll
    for (int q = 1; q < MAXJ; q++)
        if (q < JT.n && (int)blockIdx.x >= JT.j[q].block0) J = JT.j[q];
#ifdef DGS_MLP_PROFILE
    if (threadIdx.x == 0) dgs_mlp_prof[blockIdx.x * 256 + 200] = __builtin_amdgcn_s_memtime();
#endif
    // the two wave layouts are separate code regions (a runtime switch inside one loop makes the
    // register allocator spill the accumulators)
    if (J.narrow)
        dw_tile<true>(J, Ns, dz, saved, slabs, reinterpret_cast<float *>(dw_lds));
    else
        dw_tile<false>(J, Ns, dz, saved, slabs, reinterpret_cast<float *>(dw_lds));
#ifdef DGS_MLP_PROFILE
    __syncthreads();
    if (threadIdx.x == 0) {
        dgs_mlp_prof[blockIdx.x * 256 + 201] = __builtin_amdgcn_s_memtime();
        dgs_mlp_prof[blockIdx.x * 256 + 202] = (unsigned long long)(J.zrow * 10000 + J.xrow);
        dgs_mlp_prof[blockIdx.x * 256 + 203] = (unsigned long long)J.nsplit;
    }
#endif
}

}  // namespace mlp
}  // namespace dgs
