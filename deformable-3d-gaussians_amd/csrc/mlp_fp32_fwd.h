// Fused deformation MLP on fp32 MFMA, forward (device code of mlp.hip's translation unit):
// k_timenet, k_mlp_fwd<SAVE>.
#pragma once
#include "mlp_fp32_core.h"

namespace dgs {
namespace mlp {

// The network inputs (positional encodings) leave LDS for the saved-activation array in the first
// trunk GEMM's prologue: XE and TE are adjacent both in LDS (groups 0..23) and in the saved rows
// (S_XE.. S_XE + 95), TIN (blender) is one more range. A unit = 4 features x 1 point: one
// ds_read_b128 + 4 coalesced stores; a fixed unit count keeps the GEMM straight-line.
struct InputStore {
    const float4 *lds;
    float *dst;
    size_t Ns;
    int p0, tid;
    bool blender;
    __device__ void put(int g, int m, int row) const {
        const float4 v = lds[g * BM + m];
        float *d = dst + (size_t)row * Ns + p0 + m;
        d[0] = v.x; d[Ns] = v.y; d[2 * Ns] = v.z; d[3 * Ns] = v.w;
    }
    __device__ void operator()() const {
        static_assert(G_TE == G_XE + 16 && S_TE == S_XE + 64, "XE|TE must be one range");
#pragma unroll
        for (int u = 0; u < 2; u++) {  // 24 groups x 32 points = 768 units over 512 threads
            const int e = min(tid + NTHR * u, 24 * BM - 1);  // past the end: rewrite the last unit
            put(G_XE + e / BM, e % BM, S_XE + 4 * (e / BM));
        }
        if (blender && tid < 4 * BM) put(G_TIN + tid / BM, tid % BM, S_TIN + 4 * (tid / BM));  // waves 0-1
    }
};

// float offsets into the packed buffer (make_plan): forward A images and padded biases
struct FwdOffsets {
    int fT1, fT2, fL[8], fHd;
    int bT1, bT2, bL[8], bHd;
};

struct FwdArgs {
    int N;
    size_t Ns;
    const float *xyz, *t;
    const float *packed;
    float *out;
    float *saved;
    uint32_t *mask;  // relu' bits, [block][nmask] words (after the saved rows)
    float *tc;       // timenet of t[0] (k_timenet), or nullptr
    FwdOffsets o;
    int flags;
};

// What a forward GEMM carries along, chosen by type from SAVE: the training forward stores the
// network inputs in layer 0's prologue and the previous layer's tile under every later GEMM; the
// inference forward gets the empty hooks and never forms a saved-row address.
template <bool SAVE>  // InputStore or NoPre
__device__ inline auto fwd_pre(const FwdArgs &a, const float4 *lds, int p0, int tid, bool blender) {
    if constexpr (SAVE) return InputStore{lds, a.saved, a.Ns, p0, tid, blender};
    else return NoPre{};
}

template <bool SAVE>  // Stash1 or NoStash
__device__ inline auto fwd_stash(const FwdArgs &a, const f32x16 &t, int row0, int wave, int p0, int lane) {
    if constexpr (SAVE) return Stash1{t, tile_addr(a.saved, a.Ns, row0, wave * 32, p0, lane)};
    else return NoStash{};
}

// The reference feeds every Gaussian the same frame time (render(): fid.unsqueeze(0).expand(N, 1),
// train_baseline.py:107-108), so the timenet (time_utils.py:74-76, 13 -> 256 -> 30) has one value
// per launch. k_timenet evaluates it for t[0] (fp32, one workgroup); a k_mlp_fwd block whose points
// all carry that t broadcasts TE / TH instead of running T1, T2 and the t encodings per point.
__global__ __launch_bounds__(256) void k_timenet(FwdArgs a) {
    __shared__ float tin[16], th[256];
    const int j = threadIdx.x;
    const float t0 = a.t[0];
    const int tinF = 13;  // blender: t, sin / cos of 2^i t, i < 6
    if (j < 16) {
        float v = 0.f;
        if (j == 0) {
            v = t0;
        } else if (j < tinF) {
            float sv, cv;
            sincosf(t0 * (float)(1 << ((j - 1) >> 1)), &sv, &cv);
            v = (j & 1) ? sv : cv;
        }
        tin[j] = v;
        a.tc[TC_TIN + j] = v;
    }
    if (j == 0) a.tc[TC_T] = t0;
    __syncthreads();
    {  // TH[j]: A image element [tile j/32][chunk c][lane 32h + j%32] = W_T1[j][8c + 4h .. +3]
        const float4 *A = reinterpret_cast<const float4 *>(a.packed + a.o.fT1) + (j >> 5) * 2 * 64 + (j & 31);
        float acc = a.packed[a.o.bT1 + j];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float4 w = A[c * 64 + h * 32];
                const int f = 8 * c + 4 * h;
                acc += w.x * tin[f] + w.y * tin[f + 1] + w.z * tin[f + 2] + w.w * tin[f + 3];
            }
        acc = relu_nan(acc);
        th[j] = acc;
        a.tc[TC_TH + j] = acc;
    }
    __syncthreads();
    {  // TE[k], k < 32 (rows 30, 31 are zero padding): 8 lanes per output, 32 features each
        const int k = j >> 3, q = j & 7;
        const float4 *A = reinterpret_cast<const float4 *>(a.packed + a.o.fT2);
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 8; u++) {  // features 32q + 4u .. +3: chunk (32q + 4u) / 8, half u & 1
            const int f = 32 * q + 4 * u;
            const float4 w = A[(f >> 3) * 64 + ((f >> 2) & 1) * 32 + k];
            acc += w.x * th[f] + w.y * th[f + 1] + w.z * th[f + 2] + w.w * th[f + 3];
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        if (q == 0) a.tc[TC_TE + k] = acc + a.packed[a.o.bT2 + k];
    }
}

// Workgroup = 32 points x 8 waves (wave w owns output rows 32w..32w+31 of every 256-wide layer);
// 78 KiB of LDS, so two workgroups share a CU (4 waves per SIMD): one block's barrier waits and
// epilogues run under the other's MFMAs, and a partial last round of blocks runs at full rate.
template <bool SAVE>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_mlp_fwd(FwdArgs a) {
    __shared__ float4 lds[G_TOTAL * BM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (scalar branches)
    const int p0 = blockIdx.x * BM;
    const Flags F = make_flags(a.flags);
    const float4 *pk = reinterpret_cast<const float4 *>(a.packed);
    float *lf = reinterpret_cast<float *>(lds);
    const __amdgpu_buffer_rsrc_t mrsrc =
        __builtin_amdgcn_make_buffer_rsrc(a.mask + (SAVE ? (size_t)blockIdx.x * F.nmask : 0), 0, 0x7fffffff, 0x00020000);
    // frame-uniform t: every valid point of the block carries k_timenet's t0 (wave-local check on the
    // same 32 values in every wave, so the branch is block-uniform without a barrier)
    float tv_own = 0.f, tc_t0 = 1.f;
    if (SAVE && F.blender && a.tc) {
        tc_t0 = a.tc[TC_T];
        tv_own = (lane < BM && p0 + lane < a.N) ? a.t[p0 + lane] : tc_t0;
    }
    // timenet layer 0 operands, in flight during the positional encodings
    float4 t1a0 = make_float4(0.f, 0.f, 0.f, 0.f), t1a1 = t1a0;
    Bias4 t1b{};
    if (F.blender) {
        const float4 *At1 = pk + a.o.fT1 / 4 + wave * 2 * 64 + lane;
        t1a0 = At1[0];
        t1a1 = At1[64];
        t1b = load_bias(a.packed + a.o.bT1, wave * 32, lane);
    }
    // ---- positional encodings (utils/time_utils.py:42-54): feature 3 band + d, band 0 = x,
    // band 1 + 2i = sin(2^i x), band 2 + 2i = cos(2^i x); one sincosf per (point, dim, frequency) ----
    bool uniform_t = false;
    auto put = [&](int g0, int f, int m, float v) { lf[((g0 + f / 4) * BM + m) * 4 + (f & 3)] = v; };
    {
        for (int e = tid; e < BM * 3 * 11; e += NTHR) {
            const int m = e % BM, r = e / BM, d = r % 3, i = r / 3;  // i = 10: identity band
            const int p = p0 + m;
            const float x = p < a.N ? a.xyz[3 * p + d] : 0.f;
            if (i == 10) {
                put(G_XE, d, m, p < a.N ? x : 0.f);
            } else {
                float sv, cv;
                sincosf(x * (float)(1 << i), &sv, &cv);
                put(G_XE, 3 * (1 + 2 * i) + d, m, p < a.N ? sv : 0.f);
                put(G_XE, 3 * (2 + 2 * i) + d, m, p < a.N ? cv : 0.f);
            }
        }
        for (int m = tid; m < BM; m += NTHR) put(G_XE, 63, m, 0.f);  // padding feature
        uniform_t = SAVE && F.blender && a.tc && __ballot(tv_own != tc_t0) == 0;
    }
    if (uniform_t) {  // TE and TIN images: k_timenet's values broadcast over the 32 points
        const float4 *tc4 = reinterpret_cast<const float4 *>(a.tc);
        for (int e = tid; e < 12 * BM; e += NTHR) {
            const int gi = e / BM, m = e % BM;
            if (gi < 8) lds[(G_TE + gi) * BM + m] = tc4[TC_TE / 4 + gi];
            else lds[(G_TIN + gi - 8) * BM + m] = tc4[TC_TIN / 4 + gi - 8];
        }
    } else {
        const int tg = F.blender ? G_TIN : G_TE;
        const int nfreq = (F.tin - 1) / 2, ng = F.blender ? 4 : 8;
        for (int e = tid; e < BM * 4 * ng; e += NTHR) {  // zero the whole t image (padding)
            const int m = e % BM, f = e / BM;
            if (f >= F.tin) put(tg, f, m, 0.f);
        }
        for (int e = tid; e < BM * (nfreq + 1); e += NTHR) {
            const int m = e % BM, i = e / BM;  // i = nfreq: identity
            const int p = p0 + m;
            const float x = p < a.N ? a.t[p] : 0.f;
            if (i == nfreq) {
                put(tg, 0, m, x);
            } else {
                float sv, cv;
                sincosf(x * (float)(1 << i), &sv, &cv);
                put(tg, 1 + 2 * i, m, p < a.N ? sv : 0.f);
                put(tg, 2 + 2 * i, m, p < a.N ? cv : 0.f);
            }
        }
    }
    lds_barrier();
    // saved activations: the network inputs (XE|TE, TIN) leave LDS in the first trunk GEMM's
    // prologue (InputStore); every hidden layer's output is kept in registers and stored during the
    // next GEMM (Stash1)
    const float *bias = a.packed;
    f32x16 kt = zero16();  // previous layer's activations, awaiting their store
    // ---- timenet (blender): Linear(13,256) + ReLU -> H ; Linear(256,30) -> TE ----
    if (uniform_t) {  // TH tile of this wave from k_timenet: relu' bits and the saved rows
        const Bias4 th = load_bias(a.tc + TC_TH, wave * 32, lane);
        f32x16 c;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[4 * j] = th.v[j].x;
            c[4 * j + 1] = th.v[j].y;
            c[4 * j + 2] = th.v[j].z;
            c[4 * j + 3] = th.v[j].w;
        }
        store_mask_bits(c, mrsrc, (M_TH + wave * 32) * 4, lane);
        Stash1{c, tile_addr(a.saved, a.Ns, S_TH, wave * 32, p0, lane)}.store_all();
    } else if (F.blender) {
        f32x16 c = zero16();
        gemm_t1(t1a0, t1a1, lds, G_TIN, lane, c);
        bias_relu(c, t1b);
        if (SAVE) store_mask_bits(c, mrsrc, (M_TH + wave * 32) * 4, lane);
        acc_to_lds(c, lds, G_H, wave * 32, lane);
        lds_barrier();
        narrow_layer(pk + a.o.fT2 / 4, lds, G_H, G_TE, bias + a.o.bT2, wave, lane, tid,
                     fwd_stash<SAVE>(a, c, S_TH, wave, p0, lane));
    }
    // ---- trunk: 8 x (Linear + ReLU), skip cat after layer 4 (time_utils.py:107-112) ----
    for (int L = 0; L < 8; L++) {
        const int g0 = (L == 0 || L == 5) ? G_XE : G_H;
        const int nch = layer_kpad(L) / 8;
        f32x16 c = zero16();
        const float4 *Aw = pk + a.o.fL[L] / 4 + wave * nch * 64;
        const Bias4 bv = load_bias(bias + a.o.bL[L], wave * 32, lane);
        if (L == 0) {
            gemm<12>(Aw, 0, lds, g0, lane, c, fwd_pre<SAVE>(a, lds, p0, tid, F.blender));
        } else {
            const auto st = fwd_stash<SAVE>(a, kt, s_h(L - 1), wave, p0, lane);
            if (L == 5) gemm<44>(Aw, 0, lds, g0, lane, c, NoPre(), st);
            else gemm<32>(Aw, 0, lds, g0, lane, c, NoPre(), st);
        }
        lds_barrier();  // all waves finished reading H before it is overwritten
        bias_relu(c, bv);
        if (SAVE) store_mask_bits(c, mrsrc, (m_h(L) + wave * 32) * 4, lane);
        acc_to_lds(c, lds, G_H, wave * 32, lane);
        lds_barrier();
        kt = c;
    }
    // ---- heads (no activation): [warp | branch_w, branch_v], rotation, scaling -> TE region ----
    narrow_layer(pk + a.o.fHd / 4, lds, G_H, G_TE, bias + a.o.bHd, wave, lane, tid,
                 fwd_stash<SAVE>(a, kt, s_h(7), wave, p0, lane));
    for (int e = tid; e < F.nout * BM; e += NTHR) {
        int c = e % F.nout, m = e / F.nout;
        int p = p0 + m;
        if (p < a.N) a.out[(size_t)p * F.nout + c] = lf[((G_TE + c / 4) * BM + m) * 4 + (c & 3)];
    }
}

}  // namespace mlp
}  // namespace dgs
