// Fused deformation MLP on split f16, forward (device code of mlp_split.hip's translation unit): FwdArgs,
// k_timenet, the forward block, the bias table and the forward kernels k_fwd8 / k_fwd<SAVE, FOLD>.
#pragma once
#include "mlp_split_core.h"

namespace dgs {
namespace mlps {

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
struct FwdArgs {
    int N;
    size_t Ns;
    const float *xyz, *t;
    const h16x8 *img;  // A images
    const float *fp;    // fp32 region: biases, timenet weights
    float *out;
    float *saved;
    uint32_t *mask;     // relu' bits, [64-point block][row / 16][64 lanes] u16 (after the saved rows)
    float *tc;          // timenet of t[0] (k_timenet), or nullptr
    int nfull;          // 64-point blocks; the rest of [0, Ns) runs in 16-point blocks (block_split)
    int fT1, fT2, fL[8], fHd;      // image k-slots
    int bT1, bT2, bL[8], bHd;      // fp32 offsets
    int wT1, wT2;                  // fp32 timenet weights [256][16], [32][256]
    int w0te, w5te;                // fp32 t_emb columns of linear.0 / linear.5 [256][32] (C0 / C5)
    int flags;
    uint32_t *queue;  // block queue (persistent launch, BlockQueue) or nullptr: one launch block per block
    int nblk;         // blocks (64-point + 16-point)
    // the point count in device memory (the active set, mlp_active.h) or nullptr: the kernel clamps it
    // to N and derives nfull / nblk from it (split_blocks over ncu CUs); N, nfull and nblk above then
    // only size the grid and the buffers, and Ns stays the row stride of `saved`
    const int *n_dev;
    int ncu;
};

// The reference feeds every Gaussian the same frame time (train_baseline.py:107-110), so the
// timenet (time_utils.py:74-76, 13 -> 256 -> 30) has one value per launch: evaluated here once in
// fp32 (one workgroup); a k_fwd block whose points all carry that t broadcasts TE / TH.
// fpv(off): the value at offset `off` of the packed fp32 region k_pack wrote
template <class FPV>
__device__ __forceinline__ void timenet_body(const FwdArgs &a, FPV fpv) {
    __shared__ float tin[16], th[256], te[32];
    const int j = threadIdx.x;
    const float t0 = a.t[0];
    if (j < 16) {
        float v = 0.f;
        if (j == 0) {
            v = t0;
        } else if (j < 13) {  // blender: t, sin / cos of 2^i t, i < 6
            float sv, cv;
            sincosf(t0 * (float)(1 << ((j - 1) >> 1)), &sv, &cv);
            v = (j & 1) ? sv : cv;
        }
        tin[j] = v;
        a.tc[TC_TIN + j] = v;
    }
    if (j == 0) a.tc[TC_T] = t0;
    __syncthreads();
    {
        const int w = a.wT1 + j * 16;
        float acc = fpv(a.bT1 + j);
#pragma unroll
        for (int f = 0; f < 16; f++) acc = fmaf(fpv(w + f), tin[f], acc);
        acc = fmaxf(acc, 0.f);
        th[j] = acc;
        a.tc[TC_TH + j] = acc;
    }
    __syncthreads();
    {  // TE[k], k < 32 (rows 30, 31 are zero padding): 8 lanes per output, 32 features each
        const int k = j >> 3, q = j & 7;
        const int w = a.wT2 + k * 256 + 32 * q;
        float acc = 0.f;
#pragma unroll
        for (int f = 0; f < 32; f++) acc = fmaf(fpv(w + f), th[32 * q + f], acc);
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        if (q == 0) {
            const float b = fpv(a.bT2 + k);
            a.tc[TC_TE + k] = acc + b;
            te[k] = k < 30 ? acc + b : 0.f;
        }
    }
    __syncthreads();
    {  // C0 / C5: the biases of linear.0 / linear.5 with the t_emb columns folded in (k_fwd, uniform t)
        const int w0 = a.w0te + j * 32, w5 = a.w5te + j * 32;
        float c0 = fpv(a.bL[0] + j), c5 = fpv(a.bL[5] + j);
#pragma unroll
        for (int k = 0; k < 30; k++) {
            c0 = fmaf(fpv(w0 + k), te[k], c0);
            c5 = fmaf(fpv(w5 + k), te[k], c5);
        }
        a.tc[TC_C0 + j] = c0;
        a.tc[TC_C5 + j] = c5;
    }
}

__global__ __launch_bounds__(256) void k_timenet(FwdArgs a) {
    const float *fp = a.fp;
    timenet_body(a, [fp](int o) { return fp[o]; });
}

// One block of NQB 16-point column tiles (NQB = 4: the 64-point blocks; NQB = 1: the 16-point tail
// blocks that spread the last, sparse round of blocks over the idle CUs). p0: first point; slot: the
// block's relu'-mask slot; npts: the launch's point count (a.N, or the device's: FwdArgs::n_dev).
// NT: n-tiles per wave. NT = 1: 16 waves (4 per SIMD), wave r owns rows 16r .. 16r + 15 of every trunk
// layer, so an H k-step has two writers (hand-off target 2 L per layer) and 16 readers. NT = 2: the
// training forward (saved activations, frame-uniform t folded) as 8 waves (k_fwd8, 512 threads, 2 per
// SIMD): wave r owns rows 32r .. 32r + 31 = H k-step r, so each k-step has ONE writer (target L) and 8
// readers. Same LDS image, saved-activation / relu'-mask layouts, scales and arithmetic either way.
template <bool SAVE, int NQB, bool FOLD, int NT>
__device__ __forceinline__ void fwd_block(const FwdArgs &a, h16x8 *lds, uint32_t *hwr, uint32_t *hrd, const float4 *sb,
                                          uint32_t *s_mpend, ScaleLDS *sc, int npts, int p0, int slot) {
    static_assert(NT == 1 || (NT == 2 && FOLD), "two n-tiles per wave: the training forward only");
    constexpr int NW = NWAVE / NT, NTH = 64 * NW;  // waves, threads
    constexpr uint32_t HWR = 2 / NT;               // writer waves of an H k-step
    constexpr int BMB = 16 * NQB;  // points of this block (the LDS images keep the BM-point stride)
    float *lf = reinterpret_cast<float *>(lds);
    float *stage = lf + G_H * UG * 4;  // fp32 [112][BM] feature staging (H region, before the trunk)
    // re-derived per block (opaque to loop-invariant hoisting): in the persistent loop, lane
    // addresses hoisted out of it would stay live across the whole block and spill
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int r = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave: n-tiles NT r .. (provably uniform)
    const int hk = (NT * r) >> 1;                            // the H k-step its rows are part of
    const int kq = lane >> 4, col = lane & 15;
    const int pend = min(npts, p0 + BMB);  // real points of the block: [p0, pend)
    const Flags F = make_flags(a.flags);
    const size_t Ns = a.Ns;
    const __amdgpu_buffer_rsrc_t mrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.mask + (SAVE ? (size_t)slot * 2 * F.nmask : 0), 0, 0x7fffffff, 0x00020000);
    auto store_mask = [&](uint32_t w, int mr) {  // u16 mask tile mr (= row / 16): the timenet's TH
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)w, mrsrc, lane * 2, mr * 128, 0);
    };
    // the trunk's: layer L's bits wait in LDS (this thread's own word) until layer L + 1 (odd) stores
    // both as one dword: half the mask stores, and k_bwd loads one dword per two layers
    // (tools/mlp_time.py A/B: k_fwd -0.8 %, k_bwd -2 %, profiles/r4j_mlp_mask_pairs_ab.txt)
    auto trunk_mask = [&](uint32_t w, int L, int nt) {  // n-tile nt of layer L; s_mpend: [n-tile][64 lanes]
        if ((L & 1) == 0) {
            s_mpend[64 * nt + lane] = w;
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(s_mpend[64 * nt + lane] | (w << 16), mrsrc, lane * 4,
                                                  (16 * (L >> 1) + nt) * 256, 0);
        }
    };
    DGS_STAMP(0);
    // frame-uniform t: all points of the block carry k_timenet's t0 (every wave checks the same
    // values, so the branch is block-uniform without a barrier)
    bool uniform_t = FOLD || (F.uniform_t && a.tc);  // the caller's guarantee (DGS_MLP_UNIFORM_T), else checked
    if (!FOLD && F.blender && a.tc && !uniform_t) {
        const float t0 = a.tc[TC_T];
        const int p = p0 + lane;
        const float tv = (lane < BMB && p < npts) ? a.t[p] : t0;
        uniform_t = __ballot(tv != t0) == 0;
    }
    // t_emb folded into the linear.0 / linear.5 biases (FOLD = DGS_MLP_UNIFORM_T; the host always
    // provides tc then): no t_emb / TIN staging, the trunk GEMMs read x_emb (| h) only
    constexpr bool fold = FOLD;
    if (tid < 8) {
        hwr[tid] = 0;
        hrd[tid] = 0;
    }
    if constexpr (FOLD && NT == 2) {  // nothing but x_emb is staged
        if (tid < 4) sc->bsync[BS_XE][tid] = 0;
    } else {
        if (tid < 32) (&sc->bsync[0][0])[tid] = 0;
    }
    // ---- positional encodings (utils/time_utils.py:42-54) into fp32 staging: feature 3 band + d,
    // band 0 = x, band 1 + 2i = sin(2^i x), band 2 + 2i = cos(2^i x). The block's xyz rows are read
    // once (one coalesced load per thread, a single HBM round trip) into the identity band, then the
    // 10 sin/cos bands are evaluated from LDS in two rounds of the workgroup. x_emb's scale bound per
    // column tile: max(1, max |xyz|) (|sin|, |cos| <= 1) ----
    float xmax = 0.f;
    if (tid < 3 * BMB) {
        const int m = tid / 3, d = tid - 3 * m;
        const float v = p0 + m < pend ? a.xyz[3 * (size_t)p0 + tid] : 0.f;
        stage[d * BM + m] = v;
        xmax = fabsf(v);
    }
    if (tid < BMB) stage[63 * BM + tid] = 0.f;  // padding feature
    __syncthreads();
    if (tid < 3 * BMB) lds_fmax(&sc->bsync[BS_XE][qof(tid / 3)], xmax);
    for (int e = tid; e < BMB * 3 * 10; e += NTH) {
        const int m = e % BMB, rr = e / BMB, d = rr % 3, i = rr / 3;
        const bool ok = p0 + m < pend;
        float sv, cv;
        sincosf(stage[d * BM + m] * (float)(1 << i), &sv, &cv);
        stage[(3 * (1 + 2 * i) + d) * BM + m] = ok ? sv : 0.f;
        stage[(3 * (2 + 2 * i) + d) * BM + m] = ok ? cv : 0.f;
    }
    if (fold) {
    } else if (uniform_t) {  // TE and TIN: k_timenet's values broadcast over the points
        for (int e = tid; e < 48 * BMB; e += NTH) {
            const int f = e / BMB, m = e % BMB;
            const float v = f < 32 ? a.tc[TC_TE + f] : a.tc[TC_TIN + f - 32];
            stage[(ST_TE + f) * BM + m] = v;
            lds_fmax(&sc->bsync[f < 32 ? BS_TE : BS_TIN][qof(m)], fabsf(v));
        }
    } else {  // per-point t encodings: TIN (blender, 16 rows) or the raw t PE as TE (32 rows)
        const int row0 = F.blender ? ST_TIN : ST_TE, nrow = F.blender ? 16 : 32;
        for (int e = tid; e < nrow * BMB; e += NTH) {
            const int f = e / BMB, m = e % BMB;
            const int p = p0 + m;
            const float x = p < pend ? a.t[p] : 0.f;
            float v = 0.f;
            if (p < pend && f < F.tin) {
                if (f == 0) {
                    v = x;
                } else {
                    float sv, cv;
                    sincosf(x * (float)(1 << ((f - 1) >> 1)), &sv, &cv);
                    v = (f & 1) ? sv : cv;
                }
            }
            stage[(row0 + f) * BM + m] = v;
            lds_fmax(&sc->bsync[F.blender ? BS_TIN : BS_TE][qof(m)], fabsf(v));
        }
    }
    __syncthreads();
    // column-tile scales of the staged inputs (every thread evaluates the same values)
    if (tid < 4) {
        const int q = tid;
        const float xe_b = fmaxf(1.f, __uint_as_float(sc->bsync[BS_XE][q]));
        sc->ksc[0][q] = sc->ksc[1][q] = scale_for(xe_b).inv;
        sc->ain[0][q] = xe_b;
        uint32_t bad = bound_bad(__uint_as_float(sc->bsync[BS_XE][q]));  // the bits: fmaxf drops a NaN
        if (!fold) bad |= bound_bad(__uint_as_float(sc->bsync[BS_TE][q])) | bound_bad(__uint_as_float(sc->bsync[BS_TIN][q]));
        sc->bad[q] = bad;
        if (!fold) {
            sc->ksc[G_TE / 4][q] = scale_for(__uint_as_float(sc->bsync[BS_TE][q])).inv;
            sc->ksc[G_TIN / 4][q] = scale_for(__uint_as_float(sc->bsync[BS_TIN][q])).inv;
            sc->ain[1][q] = __uint_as_float(sc->bsync[BS_TE][q]);  // per-point blender: replaced by the TE tile's
        }
    }
    // saved network inputs (fp32, coalesced) and their split LDS images
    const bool te_ready = uniform_t || !F.blender;
    if (SAVE) {
        // XE | TE rows are adjacent in saved (S_TE = S_XE + 64); folded: dW reads x_emb only
        const int nrow = te_ready && !fold ? 96 : 64;
        for (int e = tid; e < nrow * BMB; e += NTH) {
            const int f = e / BMB, m = e % BMB;
            a.saved[(size_t)(S_XE + f) * Ns + p0 + m] = stage[f * BM + m];
        }
        if (F.blender && !fold)
            for (int e = tid; e < 16 * BMB; e += NTH) {
                const int f = e / BMB, m = e % BMB;
                a.saved[(size_t)(S_TIN + f) * Ns + p0 + m] = stage[(ST_TIN + f) * BM + m];
            }
    }
    {
        const int ngrp = fold ? 8 : F.blender ? 14 : 12;  // staging groups: XE 0-7 | TE 8-11 | TIN 12-13
        for (int u = tid; u < ngrp * BMB; u += NTH) {
            const int g = u / BMB, m = u % BMB;
            if (g >= G_TE && g < G_H && !te_ready) continue;  // TE comes from the per-point timenet
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = stage[(8 * g + j) * BM + m];
            const int slot_b = g < G_TE ? BS_XE : g < 12 ? BS_TE : BS_TIN;
            const float bnd = __uint_as_float(sc->bsync[slot_b][qof(m)]);
            put_unit8(lds, g < 12 ? g : G_TIN + g - 12, m, v, scale_for(g < G_TE ? fmaxf(1.f, bnd) : bnd).s);
        }
        if (F.blender && !fold)  // TIN k-step padding (features 16..31): zero, not stale LDS
            for (int u = tid; u < 2 * UG; u += NTH) lds[(G_TIN + 2) * UG + u] = h16x8{};
    }
    lds_barrier();
    DGS_STAMP(1);
    f32x4 c[NT][NQB];
    float ib[NQB];
    if constexpr (!FOLD) {  // the timenet tiles: one n-tile per wave (NT == 1)
        f32x4(&c0)[NQB] = c[0];
        if (SAVE && uniform_t && !F.uniform_t) {  // TH tile from k_timenet: relu' bits + saved rows (per-point backward)
            const float4 th = load_bias4(a.tc + TC_TH, r, lane);
#pragma unroll
            for (int q = 0; q < NQB; q++) c0[q] = f32x4{th.x, th.y, th.z, th.w};
            store_mask(relu_bits(c0), MR_TH + r);
            tile16(a.saved, Ns, S_TH + 16 * r, p0, lane).store(c0);
        }
        // ---- per-point timenet (blender, t not frame-uniform): Linear(13,256)+ReLU -> H; Linear(256,30) -> TE.
        // Both outputs are narrow per-block tiles: their scales are the actual maxima per column tile,
        // gathered behind a workgroup barrier
        if (F.blender && !uniform_t) {
            zero_tiles(c0);
            const h16x8 *A1 = a.img + (size_t)(a.fT1 + r) * KSLOT;
            gemm<1, 1, NQB>(A1, 0, lds, G_TIN, 0, lane, c, ib, sc->ksc);
            bias_relu(c0, a_inv(A1), ib, load_bias4(a.fp + a.bT1, r, lane), true);
            if (SAVE) {
                store_mask(relu_bits(c0), MR_TH + r);
                tile16(a.saved, Ns, S_TH + 16 * r, p0, lane).store(c0);
            }
            float thm[NQB] = {};
            col_absmax(c0, thm);
            col_wave_max(thm);
            if (lane == 0)
#pragma unroll
                for (int q = 0; q < NQB; q++) lds_fmax(&sc->bsync[BS_TH][q], thm[q]);
            lds_barrier();
#pragma unroll
            for (int q = 0; q < NQB; q++)
                acc_to_lds(c0[q], lds, G_H, r, q, lane, scale_for(__uint_as_float(sc->bsync[BS_TH][q])).s);
            if (tid < 32) sc->ksc[G_H / 4 + (tid >> 2)][tid & 3] = scale_for(__uint_as_float(sc->bsync[BS_TH][tid & 3])).inv;
            lds_barrier();
            f32x4 c1[1][1] = {{zero4()}};
            if (r < 2 * NQB) {  // TE tile (n-tile r / NQB of 2, column tile r % NQB), full K on one wave
                const int nt = r / NQB, q = r % NQB;
                const h16x8 *A2 = a.img + (size_t)(a.fT2 + nt * 8) * KSLOT;
                float ib2[1];
                gemm<1, 8, 1>(A2, 0, lds, G_H, q, lane, c1, ib2, sc->ksc);
                const float4 b = load_bias4(a.fp + a.bT2, nt, lane);
                c1[0][0] = c1[0][0] * (a_inv(A2) * ib2[0]) + f32x4{b.x, b.y, b.z, b.w};
                if (SAVE) tile16(a.saved, Ns, S_TE + 16 * nt, p0, lane).store(c1[0], q);
                float tm[1] = {0.f};
                col_absmax(c1[0], tm);
                col_wave_max(tm);
                if (lane == 0) lds_fmax(&sc->bsync[BS_TET][q], tm[0]);
            }
            lds_barrier();
            if (r < 2 * NQB)  // TE groups: not read by the T2 GEMM
                acc_to_lds(c1[0][0], lds, G_TE, r / NQB, r % NQB, lane,
                           scale_for(__uint_as_float(sc->bsync[BS_TET][r % NQB])).s);
            if (tid < 4) {
                const float tet = __uint_as_float(sc->bsync[BS_TET][tid]);
                sc->ksc[G_TE / 4][tid] = scale_for(tet).inv;
                sc->ain[1][tid] = tet;
            }
            lds_barrier();
        }
    }
    // ---- trunk: 8 x (Linear + ReLU), skip cat after layer 4 (time_utils.py:107-112) ----
    // No workgroup barriers: the waves of a SIMD finish a GEMM thousands of cycles apart (the oldest
    // issues first), so each wave runs its epilogue as soon as every wave has read the H k-step it
    // overwrites (hrd), and the next layer reads an H k-step once its HWR writer waves have stored it
    // (hwr): early waves' epilogues overlap late waves' MFMAs. Every writer derives the layer's output
    // scales from the same bounds (header note), so none waits for another's maximum.
#pragma unroll 1
    for (int L = 0; L < 8; L++) {
        const int g0 = (L == 0 || L == 5) ? G_XE : G_H;
        const int nk = layer_kpad_f(F, L) / 32;
#pragma unroll
        for (int t = 0; t < NT; t++) zero_tiles(c[t]);
        const h16x8 *Aw = a.img + (size_t)(a.fL[L] + NT * r * nk) * KSLOT;
        const int astride = nk * KSLOT;
        const HGate hg{hwr, hrd, L == 5 ? (fold ? 2 : 3) : 0, HWR * L, true, lane};
        if constexpr (NT == 2) DGS_WSTAMP8(24, L);
        if (L == 0) {
            if constexpr (FOLD) gemm<NT, 2, NQB>(Aw, astride, lds, g0, 0, lane, c, ib, sc->ksc);  // XE only
            else gemm<NT, 3, NQB, NoPre, NoGate, 1 << 20, 1u << 2>(Aw, astride, lds, g0, 0, lane, c, ib, sc->ksc);  // XE | TE
        } else if (L == 5) {
            if constexpr (FOLD) gemm<NT, 10, NQB, NoPre, HGate, 2, 1u << 2>(Aw, astride, lds, g0, 0, lane, c, ib, sc->ksc, NoPre(), hg);  // XE | H
            else gemm<NT, 11, NQB, NoPre, HGate, 1 << 20, (1u << 2) | (1u << 3)>(Aw, astride, lds, g0, 0, lane, c, ib, sc->ksc, NoPre(), hg);  // XE | TE | H
        } else {
            gemm<NT, 8, NQB>(Aw, astride, lds, g0, 0, lane, c, ib, sc->ksc, NoPre(), hg);
        }
        if constexpr (NT == 1) {
            DGS_STAMP(4 + 2 * L);
            DGS_WSTAMP(22, L);  // per wave: GEMM end (layer 3)
        } else {
            DGS_WSTAMP8(32, L);
        }
        float my[NQB] = {};
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int nt = NT * r + t;
            bias_relu(c[t], a_inv(Aw + t * astride), ib, sb[64 * L + 4 * nt + kq], true);
            if (SAVE) {
                trunk_mask(relu_bits(c[t]), L, nt);
#ifndef DGS_DIAG_NOSAVE  // diagnostic only (wrong backward): the trunk's saved-activation stores skipped
                tile16(a.saved, Ns, s_h(L) + 16 * nt, p0, lane).store(c[t]);
#endif
            }
            col_absmax(c[t], my);
        }
        // the layer's output scales: max_rows sum |W_L| x max |input| + max |b_L| per column tile (the
        // same on every wave)
        float so[NQB];
        const float ws = __uint_as_float(sc->wstat[L]), bm = __uint_as_float(sc->bmax[L]);
        const float4 am = L > 0 ? amax_of4(sc, (L - 1) & 1, NW) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < NQB; q++) {
            float ain = fmaxf(L == 0 || L == 5 ? sc->ain[0][q] : 0.f, f4get(am, q));
            if (!fold && (L == 0 || L == 5)) ain = fmaxf(ain, sc->ain[1][q]);
            so[q] = fmaf(ws, ain, bm);
        }
        col_wave_max(my);
        if constexpr (NT == 1) {
            if (L == 3 && r == 0) DGS_STAMP(54);
        } else {
            DGS_WSTAMP8(40, L);
        }
        // this wave's rows are (part of) H k-step hk: every wave must have read it (and its scales) in this layer
        if (L > 0) lds_wait_ge(hrd + hk, (uint32_t)NW * L, lds_peek(hrd + hk));
        if constexpr (NT == 1) {
            if (L == 3 && r == 0) DGS_STAMP(56);
        } else {
            DGS_WSTAMP8(48, L);
        }
#pragma unroll
        for (int q = 0; q < NQB; q++) {
            const Scale s = scale_for(so[q]);
            if (lane == 0) {
                sc->amax[L & 1][r][q] = my[q];
                sc->ksc[G_H / 4 + hk][q] = s.inv;
            }
#pragma unroll
            for (int t = 0; t < NT; t++) acc_to_lds(c[t][q], lds, G_H, NT * r + t, q, lane, s.s);
        }
        lds_signal(hwr + hk, lane);
        if constexpr (NT == 1) {
            if (L == 3 && r == 0) DGS_STAMP(55);
            DGS_STAMP(5 + 2 * L);
        } else {
            DGS_WSTAMP8(56, L);
        }
    }
    DGS_STAMP(20);
    // ---- heads (no activation): [warp | branch_w, branch_v], rotation, scaling: 16 rows (nout <= 13),
    // one column tile per wave, once all 8 layers' writers have signalled ----
    // on the LAST wave of each SIMD (waves NW - NQB ..): they finish layer 7 last (the MFMA pipe
    // serves the oldest wave of a SIMD first), so they start the heads without waiting on a signal,
    // while the earlier waves are already done
    const int hq = r - (NW - NQB);
    if (hq >= 0) {
        f32x4 c1[1][1] = {{zero4()}};
        float ib1[1];
        const h16x8 *Ah = a.img + (size_t)a.fHd * KSLOT;
        gemm<1, 8, 1>(Ah, 0, lds, G_H, hq, lane, c1, ib1, sc->ksc, NoPre(), HGate{hwr, hrd, 0, HWR * 8u, false, lane});
        const float4 b = sb[8 * 64 + kq];
        c1[0][0] = c1[0][0] * (a_inv(Ah) * ib1[0]) + f32x4{b.x, b.y, b.z, b.w};
        const int p = p0 + 16 * hq + col;
        // a column tile with a bound the split cannot carry (bound_bad) is poisoned: NaN for all its points
        const bool poison = sc->bad[hq] != 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (a.out && p < pend && 4 * kq + i < F.nout)
                a.out[(size_t)p * F.nout + 4 * kq + i] = poison ? __builtin_nanf("") : c1[0][0][i];
    }
    if constexpr (NT == 1) {
        DGS_STAMP(21);
#ifdef DGS_MLP_PROFILE
        if (threadIdx.x == 0 && p0 == (int)blockIdx.x * BM) {
            dgs_mlps_prof[blockIdx.x * 64 + 60] = __builtin_amdgcn_s_memrealtime();
            dgs_mlps_prof[blockIdx.x * 64 + 61] = __builtin_amdgcn_s_memtime();
        }
#endif
    }
}

// The launch-constant bias table of the forward kernels (one float4 per (layer, 4 rows), the heads' 16
// rows last; FOLD's linear.0 / linear.5 biases come from k_timenet), each layer's max |b| and the trunk
// images' row statistics (over their 16 n-tiles) for the output-scale bounds
template <bool FOLD>
__device__ inline void load_bias_table(const FwdArgs &a, float4 *s_bias, ScaleLDS *sc, int nthr) {
    if (threadIdx.x < 10) sc->bmax[threadIdx.x] = sc->wstat[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x < 8 * 16) {
        const int L = threadIdx.x >> 4, t = threadIdx.x & 15;
        const int nk = layer_kpad_f(make_flags(a.flags), L) / 32;
        lds_fmax(&sc->wstat[L], tile_stat(a.img + (size_t)(a.fL[L] + t * nk) * KSLOT));
    }
    for (int i = threadIdx.x; i < 8 * 64 + 4; i += nthr) {
        const int L = i >> 6;
        const float *bias = L == 8                ? a.fp + a.bHd
                            : FOLD && L == 0      ? a.tc + TC_C0
                            : FOLD && L == 5      ? a.tc + TC_C5
                                                  : a.fp + a.bL[L];
        const float4 v = reinterpret_cast<const float4 *>(bias)[i & 63];
        s_bias[i] = v;
        lds_fmax(&sc->bmax[L], fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
}

// A forward workgroup of 16 / NT waves: LDS, bias table, then block after block from the queue
template <bool SAVE, bool FOLD, int NT>
__device__ __forceinline__ void fwd_kernel(const FwdArgs &a) {
    __shared__ h16x8 lds[G_FWD * UG];
    __shared__ uint32_t hwr[8], hrd[8];  // trunk hand-off counters (HGate)
    __shared__ int s_next;
    __shared__ float4 s_bias[8 * 64 + 4];
    __shared__ uint32_t s_mpend[NTHR];  // relu' bits of an even trunk layer, [n-tile][64 lanes] (fwd_block)
    __shared__ ScaleLDS sc;
    // the first block's staging barriers publish the bias table
    load_bias_table<FOLD>(a, s_bias, &sc, NTHR / NT);
    CLK_BEGIN();
    int npts = a.N, nfull = a.nfull, nblk = a.nblk;
    if (a.n_dev) {  // the launch was sized for a.N points; the device's count says how many there are
        npts = device_points(a.n_dev, a.N);
        const Blocks bs = split_blocks(npts, a.ncu);
        nfull = bs.nfull;
        nblk = bs.nfull + bs.ntail;
    }
    for (int b = blockIdx.x; b < nblk;) {  // persistent: block after block from the queue (mlp_split_core.h)
        int nx = 0;
        if (a.queue && threadIdx.x == 0) nx = queue_take(a.queue);
        if (b < nfull) fwd_block<SAVE, NQ, FOLD, NT>(a, lds, hwr, hrd, s_bias, s_mpend, &sc, npts, b * BM, b);
        else fwd_block<SAVE, 1, FOLD, NT>(a, lds, hwr, hrd, s_bias, s_mpend, &sc, npts, nfull * BM + (b - nfull) * 16, b);
        if (!a.queue) break;
        if (threadIdx.x == 0) s_next = nx;
        __syncthreads();  // also: the next block's staging overwrites LDS this one's heads read
        b = s_next;
        if (b >= nblk) break;
    }
    if (a.queue) queue_release(a.queue);
    if constexpr (NT == 1) CLK_END(0);  // (diagnostic clock stamps: the 16-wave kernels only)
}

template <bool SAVE, bool FOLD>
__global__ __launch_bounds__(NTHR) void k_fwd(FwdArgs a) {
    fwd_kernel<SAVE, FOLD, 1>(a);
}

// the training forward (saved activations, frame-uniform t folded): 8 waves of two n-tiles
__global__ __launch_bounds__(NTHR8) void k_fwd8(FwdArgs a) { fwd_kernel<true, true, 2>(a); }
// the same block with the saved-row and relu'-mask stores compiled out: `out` is bitwise k_fwd8's (the
// step's first forward when the saved activations are recomputed on the active set, mlp_active.h)
__global__ __launch_bounds__(NTHR8) void k_fwd8_nosave(FwdArgs a) { fwd_kernel<false, true, 2>(a); }

}  // namespace mlps
}  // namespace dgs
