// Fused deformation MLP on fp32 MFMA, shared device core (device code of mlp.hip's translation
// unit): LDS map, the GEMM, the stash / prologue hooks and the narrow-layer pieces.
#pragma once
#include <hip/hip_runtime.h>

#include "dgs_common.h"
#include "mlp_shared.h"

namespace dgs {
namespace mlp {

using namespace mlpc;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 32;          // points per workgroup
constexpr int NWAVE = 8;
constexpr int NTHR = NWAVE * 64;
// LDS group offsets (1 group = 32 points x 4 features = 512 B): XE 0-15 | TE 16-23 | H 24-87 |
// TIN 88-91 | PART 92-155 = 8 K-part slots of 8 groups
constexpr int G_XE = 0, G_TE = 16, G_H = 24, G_TIN = 88, G_PART = 92, G_TOTAL = 156;

__device__ inline f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; i++) z[i] = 0.f;
    return z;
}

// acc += the four k-steps of one A fragment against one B fragment (v_mfma_f32_32x32x2_f32, in k order)
__device__ __forceinline__ void mfma4(f32x16 &acc, const float4 &a, const float4 &b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

struct NoPre { __device__ void operator()() const {} };

// The previous layer's output tile of this wave (rows n0 + 8(r>>2) + 4h + (r&3), point m), kept in
// registers and written to a feature-major [rows][Ns] array during the first two chunks of the
// next GEMM: 8 plain coalesced stores per chunk, issued after that GEMM's prologue loads so no
// A-fragment wait depends on them, with no LDS read and no index arithmetic.
struct NoStash { __device__ void store(int) const {} };

struct Stash1 {
    f32x16 t;
    TileAddr d;
    __device__ void store(int k) const {
#pragma unroll
        for (int j = 0; j < 8; j++) d.st(8 * k + j, t[8 * k + j]);
    }
    __device__ void store_all() const { store(0), store(1); }
};

// acc += A . X over NCH chunks starting at chunk c0 of the A image and of the LDS image at group g0
// (chunk c = groups g0 + 2c + h). Fully unrolled straight-line schedule: per chunk the A fragment 4
// chunks ahead (4-deep ring) and the next chunk's B (double-buffered ds_read_b128) are issued
// before this chunk's 4 MFMAs (sched_barrier keeps that order; the scheduler otherwise sinks the
// loads next to their use; the dependent MFMA chain is covered by the SIMD's other 3 waves), and
// the stash stores in chunks 0-1. pre() runs after the A prologue (its loads are younger than the
// first fragments).
template <int NCH, class Pre = NoPre, class Stash = NoStash>
__device__ inline void gemm(const float4 *__restrict__ Apk, int c0, const float4 *lds, int g0, int lane, f32x16 &acc,
                            Pre pre = Pre(), const Stash stash = Stash()) {
    static_assert(NCH >= 1, "empty GEMM");
    const int h = lane >> 5, m = lane & 31;
    const float4 *Ap = Apk + c0 * 64 + lane;
    const float4 *Bp = lds + (g0 + 2 * c0 + h) * BM + m;
    float4 ring[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < NCH) ring[k] = Ap[k * 64];
    pre();
    float4 bx[2];
    bx[0] = Bp[0];
#pragma unroll
    for (int k = 0; k < NCH; k++) {
        const float4 a = ring[k & 3];
        if (k + 4 < NCH) ring[k & 3] = Ap[(k + 4) * 64];
        if (k + 1 < NCH) bx[(k + 1) & 1] = Bp[2 * (k + 1) * BM];
        __builtin_amdgcn_sched_barrier(0);
        mfma4(acc, a, bx[k & 1]);
        if (k < 2) stash.store(k);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// timenet layer 0 (2 chunks) with its A fragments loaded by the caller (before the PE phase)
__device__ inline void gemm_t1(const float4 a0, const float4 a1, const float4 *lds, int g0, int lane, f32x16 &acc) {
    const int h = lane >> 5, m = lane & 31;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        mfma4(acc, c ? a1 : a0, lds[(g0 + 2 * c + h) * BM + m]);
    }
}

// accumulator (n-tile base n0) -> LDS groups starting at gout
__device__ inline void acc_to_lds(const f32x16 &acc, float4 *lds, int gout, int n0, int lane) {
    const int h = lane >> 5, m = lane & 31;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int f = n0 + 8 * j + 4 * h;
        lds[(gout + f / 4) * BM + m] = make_float4(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]);
    }
}

// bias of this lane's accumulator rows (n0 + 8j + 4h .. +3, j < 4), loaded ahead of the GEMM
struct Bias4 {
    float4 v[4];
};

__device__ inline Bias4 load_bias(const float *bias, int n0, int lane) {
    const int h = lane >> 5;
    Bias4 b;
#pragma unroll
    for (int j = 0; j < 4; j++) b.v[j] = *reinterpret_cast<const float4 *>(bias + n0 + 8 * j + 4 * h);
    return b;
}

// acc = relu(acc + bias) in place (the values kept for the deferred store). v < 0 ? 0 : v, not fmaxf(v, 0):
// a NaN stays a NaN as in torch.relu (fmaxf returns the other operand), so a point whose encodings are
// not finite (|xyz| = inf, or 2^9 |xyz| overflows) comes out non-finite, not as finite garbage
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ inline void bias_relu(f32x16 &acc, const Bias4 &b) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        acc[4 * j] = relu_nan(acc[4 * j] + b.v[j].x);
        acc[4 * j + 1] = relu_nan(acc[4 * j + 1] + b.v[j].y);
        acc[4 * j + 2] = relu_nan(acc[4 * j + 2] + b.v[j].z);
        acc[4 * j + 3] = relu_nan(acc[4 * j + 3] + b.v[j].w);
    }
}

// LDS groups [g0, g0+ng) (features 4*ng) -> global rows [row0, row0 + 4ng) of a [rows][Ns] array
__device__ inline void lds_to_global(const float4 *lds, int g0, int ng, float *__restrict__ dst, int row0, size_t Ns,
                                     int p0, int tid) {
    // thread -> (feature, point): consecutive threads = consecutive points (coalesced)
    for (int e = tid; e < ng * 4 * BM; e += NTHR) {
        int m = e % BM;
        int f = e / BM;
        const float *src = reinterpret_cast<const float *>(lds + (g0 + f / 4) * BM + m);
        dst[(size_t)(row0 + f) * Ns + p0 + m] = src[f & 3];
    }
}

// 8 K-part partials (PART slots) -> sum in a fixed order (+bias) -> LDS groups gout..gout+7
__device__ inline void sum_parts(float4 *lds, int gout, const float *bias, int tid, bool accumulate) {
    for (int e = tid; e < 8 * BM; e += NTHR) {
        const int gi = e / BM, m = e % BM;
        float4 r = lds[(G_PART + gi) * BM + m];
#pragma unroll
        for (int q = 1; q < NWAVE; q++) {
            const float4 v = lds[(G_PART + 8 * q + gi) * BM + m];
            r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
        }
        if (bias) {
            const float4 b = *reinterpret_cast<const float4 *>(bias + 4 * gi);
            r.x += b.x; r.y += b.y; r.z += b.z; r.w += b.w;
        }
        float4 &d = lds[(gout + gi) * BM + m];
        if (accumulate) {
            d.x += r.x; d.y += r.y; d.z += r.z; d.w += r.w;
        } else {
            d = r;
        }
    }
}

// narrow layer (32 output rows): K (32 chunks) split over the 8 waves, 4 chunks each, partials
// summed in a fixed order (+bias) into LDS groups gout..gout+7
template <class Stash = NoStash>
__device__ inline void narrow_layer(const float4 *Apk, float4 *lds, int g0, int gout, const float *bias, int wave,
                                    int lane, int tid, const Stash stash = Stash()) {
    f32x16 acc = zero16();
    gemm<4>(Apk, wave * 4, lds, g0, lane, acc, NoPre(), stash);
    acc_to_lds(acc, lds, G_PART + 8 * wave, 0, lane);
    lds_barrier();
    sum_parts(lds, gout, bias, tid, false);
    lds_barrier();
}

}  // namespace mlp
}  // namespace dgs
