// Fused deformation MLP on split f16 (device code of mlp_split.hip's translation unit; the map of the
// whole path, numerics and layout, is at the top of mlp_split.hip). What every stage shares: constants,
// the scaled two-piece split, the per-block scale state, the stamp macros of the diagnostic builds, the
// LDS hand-off, the GEMM, the tile helpers and the block queue of the persistent launches.
#pragma once
#include <hip/hip_runtime.h>

#include "dgs_common.h"
#include "mlp_shared.h"

namespace dgs {
namespace mlps {

using namespace mlpc;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

constexpr int BM = 64;            // points per workgroup
constexpr int NQ = 4;             // 16-point column tiles per workgroup
constexpr int NWAVE = 16;         // one 16-row n-tile of a 256-wide layer per wave
constexpr int NTHR = NWAVE * 64;
constexpr int NTHR8 = NTHR / 2;   // k_fwd8 / k_bwd8: 8 waves of two n-tiles each
constexpr int NSPLIT = 2;         // hi, lo
constexpr int PACK_MAXK = 11;     // k-slots of the widest A-image n-tile (linear.5's forward image: 352 / 32)
constexpr int UG = NSPLIT * BM;   // 16-B units per 8-feature group (all splits, all points)
constexpr int KSLOT = 3 * 64;     // units per (n-tile, k-step) of an A image: hi, lo, inverse scale
constexpr int KG = 4;             // 8-feature groups per k-step (32 features)
// forward LDS groups: XE (64 features) | TE (32) | H (256) | TIN (16 + 16 zero: one k-step)
constexpr int G_XE = 0, G_TE = 8, G_H = 12, G_TIN = 44, G_FWD = 48;
// backward LDS groups: H (dZ, 256) | G (dOut / dTE, 32)
constexpr int G_BH = 0, G_BG = 32, G_BWD = 36;
// fp32 staging rows (inside the H region): XE 0..63 | TE 64..95 | TIN 96..111
constexpr int ST_TE = 64, ST_TIN = 96;
// relu' masks per 64-point block (2 * nmask u32 words): the trunk's as [layer pair][row / 16][64 lanes]
// u32 (layer 2l in the low, 2l + 1 in the high 16 bits: one dword store per two layers), then the
// timenet TH tiles as [row / 16][64 lanes] u16 at tile MR_TH
constexpr int MR_TH = M_TH / 16;

static_assert(G_TE == G_XE + 8 && G_H == G_TE + 4, "XE|TE|H must be contiguous");
static_assert(G_FWD * UG * 16 + (8 * 256 + 16) * 4 + NTHR * 4 + 512 <= 160 * 1024 && G_BWD * UG * 16 <= 160 * 1024,
              "LDS (k_fwd: + trunk biases, pending relu' bits, hand-off counters, scales)");
static_assert(112 * BM * 4 <= 32 * UG * 16, "fp32 staging must fit the H region");

// ------------------------------------------------------------------------------------------------
// scaled two-piece f16 split
// ------------------------------------------------------------------------------------------------
// 2^e as a float (e in [-126, 127])
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
// the power-of-two scale S that brings a bound m >= max |x| into [2^14, 2^15), and 1 / S; exponents
// clamped to +-60 (a zero or tiny bound keeps S = 2^74, an infinite one 2^-46)
struct Scale {
    float s, inv;
};
__device__ __forceinline__ Scale scale_for(float m) {
    int e = (int)((__float_as_uint(m) >> 23) & 255u) - 127;
    e = min(max(e, -60), 60);
    return Scale{pow2f(14 - e), pow2f(e - 14)};
}

// A bound the split cannot carry: exponent above scale_for's clamp (>= 2^61: the scaled values would
// overflow f16), an infinity or a NaN (bounds are maxima of float BITS, so a NaN input arrives as the
// largest). The forward tests the bounds of the inputs it stages (xyz, the t encodings) and poisons such a
// column tile: all 16 points' outputs are NaN (fwd_block), not the finite values a clamped scale would give
// the tile's in-range points.
__device__ __forceinline__ uint32_t bound_bad(float m) { return ((__float_as_uint(m) >> 23) & 255u) > 127u + 60u; }

// hi = f16(a), lo = f16(a - hi) of two (already scaled) values, pairwise: v_cvt_pk_f16_f32, two
// f16 -> f32, a packed subtraction, v_cvt_pk_f16_f32 (5 VALU per two values)
__device__ __forceinline__ void hsplit2(float a, float b, uint32_t &h, uint32_t &l) {
    const h16x2 hv = __builtin_convertvector((f32x2){a, b}, h16x2);
    const f32x2 hf = __builtin_convertvector(hv, f32x2);
    const h16x2 lv = __builtin_convertvector((f32x2){a - hf[0], b - hf[1]}, h16x2);
    h = __builtin_bit_cast(uint32_t, hv);
    l = __builtin_bit_cast(uint32_t, lv);
}

struct Split4 {
    h16x4 h, l;
};

// four values times the scale S -> their hi / lo halves of a unit
__device__ inline Split4 split4(float a, float b, float c, float d, float S) {
    uint32_t h0, l0, h1, l1;
    hsplit2(a * S, b * S, h0, l0);
    hsplit2(c * S, d * S, h1, l1);
    return Split4{__builtin_bit_cast(h16x4, make_uint2(h0, h1)), __builtin_bit_cast(h16x4, make_uint2(l0, l1))};
}

// 8 consecutive features of one point -> the two 16-B units of group g (LDS image [g][split][BM])
__device__ inline void put_unit8(h16x8 *lds, int g, int m, const float (&v)[8], float S) {
    const Split4 a = split4(v[0], v[1], v[2], v[3], S);
    const Split4 b = split4(v[4], v[5], v[6], v[7], S);
    h16x8 *u = lds + g * UG + m;
    u[0] = __builtin_shufflevector(a.h, b.h, 0, 1, 2, 3, 4, 5, 6, 7);
    u[BM] = __builtin_shufflevector(a.l, b.l, 0, 1, 2, 3, 4, 5, 6, 7);
}

// max over the wave of non-negative floats (as u32: the same order), in every lane: DPP row shifts,
// the row broadcasts into lane 63, then readlane
__device__ __forceinline__ float wave_max(float v) {
    uint32_t x = __float_as_uint(v);
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));
    return __uint_as_float(__builtin_amdgcn_readlane(x, 63));
}

// max |v| over this lane's tiles
template <int NQ_>
__device__ inline float tiles_absmax(const f32x4 (&v)[NQ_]) {
    float m = 0.f;
#pragma unroll
    for (int q = 0; q < NQ_; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) m = fmaxf(m, fabsf(v[q][i]));
    return m;
}

// LDS max of non-negative floats (ds_max_u32 on the bits)
__device__ __forceinline__ void lds_fmax(uint32_t *p, float v) {
    __hip_atomic_fetch_max(p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Per-block scale state in LDS. Every B-operand scale is per 16-point column tile q (the MFMA's column
// block), so a point's arithmetic does not depend on which other points share its workgroup (the tail
// decomposition, block_split, stays bitwise equal to 64-point blocks):
//  ksc[k][q]: inverse scale of k-step k of the LDS image, column tile q (every writer of a k-step stores
//             the same value)
//  amax[par][w][q]: actual max |output| of writer wave w in the layer (chain step) of parity par
//  ain[i][q]: maxima of the staged inputs: [0] x_emb (forward) / dOut (backward), [1] t_emb
//  bsync[i][q]: block-wide maxima gathered behind a workgroup barrier (staging, narrow timenet tiles)
//  bmax[L]: max |bias| of trunk layer L (8: heads), from the launch-constant bias table
//  wstat[L]: max row abs sum of the layer's A image (k_pack's tile statistics; [8]: heads^T)
//  bad[q]: a staged input bound of column tile q is out of range (bound_bad; forward)
struct alignas(16) ScaleLDS {
    float ksc[12][4];
    float amax[2][16][4];
    float ain[2][4];
    uint32_t bsync[8][4];
    uint32_t bmax[10];
    uint32_t wstat[10];
    uint32_t bad[4];
};
// block-sync slots
constexpr int BS_XE = 0, BS_TE = 1, BS_TIN = 2, BS_TH = 3, BS_TET = 4, BS_G = 5, BS_GTE = 6;

// max over the nw writer waves of their published maxima, all four column tiles (one 16-B read per wave)
__device__ inline float4 amax_of4(const ScaleLDS *sc, int par, int nw) {
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int w = 0; w < nw; w++) {
        const float4 v = *reinterpret_cast<const float4 *>(sc->amax[par][w]);
        m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
    }
    return m;
}
__device__ __forceinline__ float f4get(const float4 &v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

// ------------------------------------------------------------------------------------------------
// GEMM pieces. 16x16x32 lane maps (cdna_hip_programming.md §3): lane l (kq = l >> 4, col = l & 15)
// holds A[row col][k = 8 kq + j] and B[k = 8 kq + j][col col]; C/D element i is row 4 kq + i, col col.
// ------------------------------------------------------------------------------------------------
#define MF16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

struct AFrag {  // one operand fragment in its two split parts
    h16x8 h, l;
};

__device__ inline AFrag load_a(const h16x8 *p) { return AFrag{p[0], p[64]}; }

// B fragment of column tile q from the LDS image (p: this lane's unit of split 0, column tile 0)
__device__ inline AFrag load_b(const h16x8 *p, int q) { return AFrag{p[16 * q], p[BM + 16 * q]}; }

__device__ inline f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// The three split products of one k-step: hh into the running accumulator, the two corrections
// (|.| <= 2^-11 |hh|) into their own accumulator, added in fp32 once per GEMM
__device__ inline void mma3(const AFrag &a, const AFrag &b, f32x4 &acc, f32x4 &lo) {
    lo = MF16(a.l, b.h, lo);
    lo = MF16(a.h, b.l, lo);
    acc = MF16(a.h, b.h, acc);
}

// inverse scale of an A image's n-tile: the float after its first k-slot's two planes
__device__ __forceinline__ float a_inv(const h16x8 *tile_slot0) {
    return reinterpret_cast<const float *>(tile_slot0 + 128)[0];
}

#ifdef DGS_MLP_PROFILE  // diagnostic build only (tools/mlp_phase.py): per-phase s_memtime stamps
__device__ unsigned long long *dgs_mlps_prof;
// only the workgroup's first block (launched while every CU is busy) is stamped: p0 == blockIdx.x * BM
#define DGS_STAMP(k)                                                                                   \
    do {                                                                                               \
        if (threadIdx.x == 0 && p0 == (int)blockIdx.x * BM)                                            \
            dgs_mlps_prof[blockIdx.x * 64 + (k)] = __builtin_amdgcn_s_memtime();                       \
    } while (0)
#define DGS_WSTAMP(k, L)                                                                               \
    do {                                                                                               \
        if (L == 3 && (threadIdx.x & 63) == 0 && p0 == (int)blockIdx.x * BM)                           \
            dgs_mlps_prof[blockIdx.x * 64 + (k) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
// k_fwd8 (8 waves): layer DGS_PROF_LAYER of the workgroup's first block, stamp k + wave
#ifndef DGS_PROF_LAYER
#define DGS_PROF_LAYER 3
#endif
#define DGS_WSTAMP8(k, L)                                                                              \
    do {                                                                                               \
        if (L == DGS_PROF_LAYER && (threadIdx.x & 63) == 0 && p0 == (int)blockIdx.x * BM)              \
            dgs_mlps_prof[blockIdx.x * 64 + (k) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
#else
#define DGS_WSTAMP8(k, L) \
    do {                  \
    } while (0)
#define DGS_WSTAMP(k, L) \
    do {                 \
    } while (0)
#define DGS_STAMP(k) \
    do {             \
    } while (0)
#endif

struct NoPre {
    __device__ void operator()() const {}
};

// LDS hand-off between the waves of a workgroup without a workgroup barrier: monotonically growing
// per-k-step counters, a relaxed LDS load spun on (wave-uniform), a relaxed LDS add from one lane.
// A wave executes its LDS operations in issue order, so data written before a signal is visible to
// a wave that has seen the signal; the empty asm keeps the compiler from moving LDS accesses across.
// The spin is bounded so a wrong count can never hang the GPU; an expired bound is not silent: it
// counts into dgs_mlps_guard_expired (a global atomic from one lane), which the host reads with
// dgs_debug_guard_expiries() and every GPU test checks to be 0 (outputs after an expiry are invalid).
__device__ uint32_t dgs_mlps_guard_expired;

#ifdef DGS_CLOCK_STAMPS
// Diagnostic build only (tools/mlp_clock.py): per-workgroup in-kernel clock of k_fwd / k_bwd / k_dws
// (MI355X_MICROARCH 'DVFS give-back' item 6): shader-clock and 100 MHz real-time stamps of wave 0 at
// block start and end, into a buffer no kernel reads. The product build has no stamps.
constexpr int CLK_BLOCKS = 2048;
__device__ unsigned long long dgs_clk[3][CLK_BLOCKS][6];
struct ClkStamp {
    unsigned long long t, r;
    __device__ ClkStamp() : t(__builtin_amdgcn_s_memtime()), r(__builtin_amdgcn_s_memrealtime()) {}
    __device__ void end(int k) const {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0 && blockIdx.x < CLK_BLOCKS) {
            unsigned long long *p = dgs_clk[k][blockIdx.x];
            p[0] = t; p[1] = t1; p[2] = r; p[3] = r1;
            // HW_ID (CU / SH / SE fields) and XCC_ID: which CU ran the workgroup
            p[4] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                   ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
        }
    }
};
#define CLK_BEGIN() const ClkStamp clk_
#define CLK_END(k) clk_.end(k)
#else
#define CLK_BEGIN()
#define CLK_END(k)
#endif
#ifndef DGS_SPIN_SLEEP
#define DGS_SPIN_SLEEP 1  // s_sleep units (64 clocks) between polls of a hand-off counter
#endif
__device__ __forceinline__ uint32_t lds_peek(const uint32_t *f) {
    return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// The first test of `seen` (peeked earlier, usually already satisfied) sits outside the spin loop:
// as the loop's header it merged with the loop's own fresh peek, so the compiler waited for EVERY
// outstanding LDS read there (lgkmcnt(0)) — the next tile's just-issued B fragment reads included —
// once per k-step of every GEMM; outside it, the wait covers the peek only.
__device__ __forceinline__ void lds_wait_ge(const uint32_t *f, uint32_t target, uint32_t seen) {
    if (__builtin_amdgcn_readfirstlane(seen) < target) {
        int guard = 0;
#pragma clang loop unroll(disable)
        do {
            __builtin_amdgcn_s_sleep(DGS_SPIN_SLEEP);
            seen = lds_peek(f);
        } while (__builtin_amdgcn_readfirstlane(seen) < target && ++guard < (1 << 20));
        if (guard == (1 << 20) && (threadIdx.x & 63) == 0)
            __hip_atomic_fetch_add(&dgs_mlps_guard_expired, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void lds_signal(uint32_t *f, int lane) {
    asm volatile("" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct NoGate {
    __device__ uint32_t peek(int) const { return 0; }
    __device__ void need(int, uint32_t) const {}
    __device__ void done(int) const {}
};

// Trunk gate: the H k-steps (GEMM k-steps k0..) may be read once both writer waves of the previous
// layer have signalled wr[j] (wr[j] >= wt), and each wave signals rd[j] once its reads of H k-step
// j are consumed (the next layer's writers wait for all 16)
struct HGate {
    uint32_t *wr, *rd;
    int k0;
    uint32_t wt;
    bool sig;
    int lane;
    __device__ uint32_t peek(int k) const { return k < k0 ? 0xffffffffu : lds_peek(wr + (k - k0)); }
    __device__ void need(int k, uint32_t seen) const {
        if (k >= k0) lds_wait_ge(wr + (k - k0), wt, seen);
    }
    __device__ void done(int k) const {
        if (sig && k >= k0) lds_signal(rd + (k - k0), lane);
    }
};

// f(0) .. f(NT - 1) written out, not a loop: the GEMM's per-n-tile loads and MFMAs reach the optimizer as
// the straight-line statements they were in the two-n-tile copy of the GEMM (a loop over t, unrolled
// later, moved the allocation of k_fwd8 / k_bwd8: profiles/mlp_split_core_resources.txt)
template <int NT, class F>
__device__ __forceinline__ void each_ntile(F f) {
    static_assert(NT == 1 || NT == 2, "n-tiles per wave");
    f(0);
    if constexpr (NT == 2) f(1);
}

// acc[t][q] += A_t . X for the NT n-tiles of this wave (n-tile t's A image at Aw + t * astride units, Aw:
// unit pointer of n-tile 0 at k-step 0) and the column tiles q0 .. q0 + NQ_ - 1, over NK k-steps of the A
// images and of the LDS image from group g0 (k-step c = groups g0 + 4c + kq). NT = 1: the 16-wave
// kernels and the narrow tiles; NT = 2 (the 8-wave k_fwd8 / k_bwd8): every B fragment read from LDS
// feeds both n-tiles' MFMAs, so the activation image is read by 8 waves per layer instead of 16; each
// (n-tile, column tile) accumulator sees the same MFMA sequence either way. Fully unrolled; per k-step:
// each column tile's three MFMAs per n-tile followed by its B fragment for the next k-step into the same
// registers, then the A fragments RING k-steps ahead (register ring: the A stream comes from L2).
// sched_barrier keeps that order per k-step; the other waves of the SIMD cover the B reload latency.
// pre() runs after the A prologue. SKIP: k-steps >= SKIP read the LDS image one k-step further on
// (linear.5 with t_emb folded: x_emb | h, past t_emb).
// Scales: ksc[g / 4][q] is the inverse scale of the image k-step at group g, column tile q (read once
// its writers have signalled). BND: bit k set = k-step k starts a new scale group (x_emb | t_emb | h);
// there the accumulators are brought to the new group's scale (one multiply by a power of two). ib[q]:
// the inverse scale of the last group: the result is acc[t][q] * (A_t's inverse scale) * ib[q].
template <int NT, int NK, int NQ_, class Pre = NoPre, class Gate = NoGate, int SKIP = (1 << 20), unsigned BND = 0u>
__device__ inline void gemm(const h16x8 *__restrict__ Aw, int astride, const h16x8 *lds, int g0, int q0, int lane,
                            f32x4 (&acc)[NT][NQ_], float (&ib)[NQ_], const float (*ksc)[4], Pre pre = Pre(),
                            Gate gate = Gate()) {
    static_assert(NK >= 1, "empty GEMM");
    const int kq = lane >> 4, col = lane & 15;
    const h16x8 *Ap[NT];
    each_ntile<NT>([&](int t) __attribute__((always_inline)) { Ap[t] = Aw + t * astride + lane; });
    const int bunit = (g0 + kq) * UG + 16 * q0 + col;  // this lane's B unit at k-step 0
    constexpr int AK = KSLOT;
    constexpr int BK = KG * UG;
    auto bofs = [](int k) { return (k + (k >= SKIP ? 1 : 0)) * BK; };  // compile-time per unrolled k
    auto kidx = [&](int k) { return (g0 >> 2) + k + (k >= SKIP ? 1 : 0); };
    // the B fragments of k-step k from a base formed once per k-step (the unit index is opaque to the
    // compiler): the image spans > 64 KB, so a single base would need one address add per ds_read
    // (a DS immediate offset is 16 bits); from the k-step base every fragment is an immediate offset
    auto kbase = [&](int k) {
        int u = bunit + bofs(k);
        asm volatile("" : "+v"(u));
        return lds + u;
    };
    constexpr int RING = 2;
    AFrag ring[RING][NT];
#pragma unroll
    for (int k = 0; k < RING; k++)
        if (k < NK) each_ntile<NT>([&](int t) __attribute__((always_inline)) { ring[k][t] = load_a(Ap[t] + k * AK); });
    pre();
    gate.need(0, gate.peek(0));
    float cur[NQ_], nxt[NQ_];
#pragma unroll
    for (int q = 0; q < NQ_; q++) nxt[q] = cur[q] = ksc[kidx(0)][q0 + q];
    const h16x8 *Bk = kbase(0);
    AFrag b = load_b(Bk, 0);
    f32x4 lo[NT][NQ_];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < NQ_; q++) lo[t][q] = zero4();
#pragma unroll
    for (int k = 0; k < NK; k++) {
        __builtin_amdgcn_sched_barrier(0);
        if (k > 0) gate.done(k - 1);  // k-step k-1's B fragments were consumed by its MFMAs
        if (k > 0 && k < 32 && ((BND >> k) & 1u)) {  // a new scale group starts here
#pragma unroll
            for (int q = 0; q < NQ_; q++) {
                const float r = cur[q] / nxt[q];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    acc[t][q] = (acc[t][q] + lo[t][q]) * r;
                    lo[t][q] = zero4();
                }
                cur[q] = nxt[q];
            }
        }
        const uint32_t seen = k + 1 < NK ? gate.peek(k + 1) : 0u;
#pragma unroll
        for (int q = 0; q < NQ_; q++) {
            // the next tile's B fragment (or the next k-step's first) is in flight during this tile's MFMAs
            AFrag nb;
            if (q + 1 < NQ_) nb = load_b(Bk, q + 1);
            else if (k + 1 < NK) {
                gate.need(k + 1, seen);
                if (k + 1 < 32 && ((BND >> (k + 1)) & 1u))
#pragma unroll
                    for (int q2 = 0; q2 < NQ_; q2++) nxt[q2] = ksc[kidx(k + 1)][q0 + q2];
                Bk = kbase(k + 1);
                nb = load_b(Bk, 0);
            }
            // the reads stay ahead of ALL the MFMAs of this tile: without this barrier the scheduler,
            // short of registers, sank them below the tile's first MFMAs (reusing the current
            // fragment's registers), so the next tile's first MFMAs waited on them (k_fwd -1.4 %,
            // profiles/r5f_mlp_bread_pin_ab.txt)
            __builtin_amdgcn_sched_barrier(0);
            each_ntile<NT>([&](int t) __attribute__((always_inline)) { mma3(ring[k % RING][t], b, acc[t][q], lo[t][q]); });
            if (q + 1 < NQ_ || k + 1 < NK) b = nb;
            // pin the order per column tile: the next fragment's reads stay ahead of this tile's
            // MFMAs (left to itself the scheduler pulls each read down to its first use and waits on
            // it: lgkmcnt(0) in front of most MFMAs)
            __builtin_amdgcn_sched_barrier(0);
        }
        if (k + RING < NK)
            each_ntile<NT>([&](int t) __attribute__((always_inline)) { ring[k % RING][t] = load_a(Ap[t] + (k + RING) * AK); });
        __builtin_amdgcn_sched_barrier(0);
    }
    gate.done(NK - 1);
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < NQ_; q++) acc[t][q] += lo[t][q];
#pragma unroll
    for (int q = 0; q < NQ_; q++) ib[q] = cur[q];
}

// accumulator tile q (rows 16r + 4kq + i of this wave, point 16q + col) -> its 8-byte half of the
// split units of group 2r + (kq >> 1) (LDS image from group gbase)
// (times the layer's scale S)
__device__ inline void acc_to_lds(const f32x4 &v, h16x8 *lds, int gbase, int r, int q, int lane, float S) {
    const int kq = lane >> 4, col = lane & 15;
    const Split4 s = split4(v[0], v[1], v[2], v[3], S);
    h16x4 *u = reinterpret_cast<h16x4 *>(lds + (gbase + 2 * r + (kq >> 1)) * UG + 16 * q + col) + (kq & 1);
    u[0] = s.h;
    u[2 * BM] = s.l;  // h16x4 units: one 16-B unit = 2 of them
}

// A wave's 16-row x 64-point tile of a feature-major [rows][Ns] array through a buffer descriptor
// whose base is the tile origin (wave-uniform: SGPRs): store (i, q) writes rows 4kq + i of column
// tile q, one buffer instruction each with the row offset in an SGPR.
struct Tile16 {
    __amdgpu_buffer_rsrc_t rsrc;  // base = &dst[row0 * Ns + p0]
    int voff;                     // (4kq * Ns + col) * 4 bytes
    int ns4;                      // Ns * 4 bytes
// Cache policy of these stores (the saved activations / dZ: ~0.95 GB per launch, read back only by
// the dW kernel after the whole launch): nt. A/B r5m against plain stores: k_fwd -1.7 %, k_bwd -3 %,
// k_dws (their reader) -4..-6 %, step +2.5 %; sc1 (write-through, line dropped from L2) was 3-7 %
// slower. (Without any of these stores k_fwd / k_bwd ran 7 / 15 % faster, r5j; 16-byte stores after a
// quad transpose were 5-6 % slower, r5k; the next layer's first A fragment issued ahead of the stores
// changed nothing, r5l.)
#ifndef DGS_TILE_STORE_AUX
#define DGS_TILE_STORE_AUX 2
#endif
    __device__ void st(int i, int q, float v) const {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc, voff + 64 * q, i * ns4, DGS_TILE_STORE_AUX);
    }
    template <int NQ_>
    __device__ void store(const f32x4 (&v)[NQ_], int q0 = 0) const {
#pragma unroll
        for (int q = 0; q < NQ_; q++)
#pragma unroll
            for (int i = 0; i < 4; i++) st(i, q0 + q, v[q][i]);
    }
};

__device__ inline Tile16 tile16(const float *dst, size_t Ns, int row0, int p0, int lane) {
    const float *base = dst + (size_t)row0 * Ns + p0;
    return Tile16{__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, 0x7fffffff, 0x00020000),
                  (4 * (lane >> 4) * (int)Ns + (lane & 15)) * 4, (int)Ns * 4};
}

// relu' bits of a wave's 16 x 64 tile: bit 4q + i of lane (kq, col) = [row 4kq + i of point 16q + col
// > 0] (signed clamp of the float bits: -0.0 and +0.0 give 0); the backward's tiles have the same map
template <int NQ_>
__device__ inline uint32_t relu_bits(const f32x4 (&v)[NQ_]) {
    uint32_t w = 0;
#pragma unroll
    for (int q = 0; q < NQ_; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // v_med3_i32 + v_lshl_or_b32: 2 VALU per value (the compiler's own v_cmp + v_cndmask +
            // v_lshl + v_or3 take ~2.4)
            uint32_t m;
            asm("v_med3_i32 %0, %1, 0, 1" : "=v"(m) : "v"(__float_as_int(v[q][i])));
            if (q == 0 && i == 0) w = m;
            else asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(w) : "v"(m), "i"(4 * q + i), "v"(w));
        }
    return w;
}

template <int NQ_>
__device__ inline void mask_apply(f32x4 (&v)[NQ_], uint32_t bits) {
#pragma unroll
    for (int q = 0; q < NQ_; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // v_bfe_i32 + v_and (2 VALU): left to itself the compiler turns the sign-extended bit into
            // v_and + v_cmp + v_cndmask (3 VALU per value)
            int m;
            asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(bits), "i"(4 * q + i));
            v[q][i] = __int_as_float(__float_as_int(v[q][i]) & m);
        }
}

// this lane's 4 rows (16r + 4kq .. +3) of a padded bias vector
__device__ inline float4 load_bias4(const float *bias, int r, int lane) {
    return *reinterpret_cast<const float4 *>(bias + 16 * r + 4 * (lane >> 4));
}

// v[q] * (ia * ib[q]) + b (ia: A's inverse scale, ib: the GEMM's B scales per column tile), then ReLU
template <int NQ_>
__device__ inline void bias_relu(f32x4 (&v)[NQ_], float ia, const float (&ib)[NQ_], float4 b, bool relu) {
#pragma unroll
    for (int q = 0; q < NQ_; q++) {
        v[q] = v[q] * (ia * ib[q]) + f32x4{b.x, b.y, b.z, b.w};
        if (relu)
#pragma unroll
            for (int i = 0; i < 4; i++) v[q][i] = fmaxf(v[q][i], 0.f);
    }
}

template <int NQ_>
__device__ inline void scale_tiles(f32x4 (&v)[NQ_], float ia, const float (&ib)[NQ_]) {
#pragma unroll
    for (int q = 0; q < NQ_; q++) v[q] *= ia * ib[q];
}

template <int NQ_>
__device__ inline void zero_tiles(f32x4 (&v)[NQ_]) {
#pragma unroll
    for (int q = 0; q < NQ_; q++) v[q] = zero4();
}

// k_pack's statistic of an image n-tile: max over its 16 rows of sum_k |A[row][k]| (the float after the
// tile's inverse scale)
__device__ __forceinline__ float tile_stat(const h16x8 *tile_slot0) {
    return reinterpret_cast<const float *>(tile_slot0 + 128)[1];
}

// per column tile q (16 points): max |v| over this wave's tiles of it (two n-tiles: both), in every lane
template <int NQ_>
__device__ inline void col_absmax(const f32x4 (&v)[NQ_], float (&m)[NQ_]) {
#pragma unroll
    for (int q = 0; q < NQ_; q++) {
        float x = 0.f;
#pragma unroll
        for (int i = 0; i < 4; i++) x = fmaxf(x, fabsf(v[q][i]));
        m[q] = fmaxf(m[q], x);
    }
}
template <int NQ_>
__device__ inline void col_wave_max(float (&m)[NQ_]) {
#pragma unroll
    for (int q = 0; q < NQ_; q++) m[q] = wave_max(m[q]);
}

// the stage value of point slot m (0 .. 63 of the image) goes to column tile m >> 4
__device__ __forceinline__ int qof(int m) { return m >> 4; }

// Persistent launches (round 3): one workgroup per CU runs block after block, taking the next block
// index from a device counter, so faster XCDs take more blocks. The eight XCDs hold different clocks
// under this load (1.80-2.04 GHz measured, tools/mlp_clock.py) and the hardware hands workgroups to
// XCDs round-robin, so with one launch block per block the slowest XCD set the kernel time. Block b
// computes exactly what it computed before (same points, same mask slot): outputs are bitwise
// unchanged. The index of the next block is fetched at the start of the current one (latency hidden
// by the block); the last workgroup to finish zeroes the counter pair for the next launch.
// Block decomposition of the fused forward / dX kernels (one 147 KB workgroup per CU): when the last
// round of 64-point blocks would occupy at most a quarter of the ncu CUs, those blocks run as four times
// as many 16-point blocks instead (fwd_block / bwd_block NQB = 1), so the sparse last round ends in
// roughly a third of a full block's time (the A stream, not the MFMAs, bounds a 16-point block).
// ncu = 0 keeps 64-point blocks throughout. Mask slots: one per block (<= nb + 3 min(nb, 128)).
// Host and device: a launch whose point count is only known on the device (n_dev of FwdArgs / BwdArgs,
// the active set of mlp_active.h) derives its blocks from it there.
constexpr int TAIL_MAX_LAST = 128;
struct Blocks {
    int nfull, ntail;
};
__host__ __device__ inline Blocks split_blocks(int N, int ncu) {
    const int nb = div_up(N, BM);
    if (ncu <= 0 || nb == 0) return {nb, 0};
    const int rounds = div_up(nb, ncu), last = nb - ncu * (rounds - 1);
    if (rounds < 2 || last > TAIL_MAX_LAST || 4 * last > ncu) return {nb, 0};
    return {nb - last, 4 * last};
}
// n_dev launches: the device word's point count, clamped to the launch's N (a wave-uniform value)
__device__ __forceinline__ int device_points(const int *n_dev, int N) {
    return min(max(__builtin_amdgcn_readfirstlane(*n_dev), 0), N);
}

__device__ __forceinline__ int queue_take(uint32_t *q) { return (int)gridDim.x + (int)atomicAdd(q, 1u); }
__device__ __forceinline__ void queue_release(uint32_t *q) {
    // every workgroup's final take has returned before its increment of q[1]
    if (threadIdx.x == 0 && atomicAdd(q + 1, 1u) == gridDim.x - 1) {
        atomicExch(q, 0u);
        atomicExch(q + 1, 0u);
    }
}

}  // namespace mlps
}  // namespace dgs
