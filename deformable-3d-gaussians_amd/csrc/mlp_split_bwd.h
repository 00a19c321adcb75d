// Fused deformation MLP on split f16, dX chain (device code of mlp_split.hip's translation unit): BwdArgs,
// the relu'-mask loaders, dOut staging, the dX block, the backward kernels k_bwd8 / k_bwd<TE_ROWS>, k_tgrad.
#pragma once
#include "mlp_split_core.h"

namespace dgs {
namespace mlps {

// ------------------------------------------------------------------------------------------------
// backward (dX chain): dZ_i for every layer -> scratch; deterministic
// ------------------------------------------------------------------------------------------------
struct BwdArgs {
    int N;
    size_t Ns;
    const h16x8 *img;
    const uint32_t *mask;
    const float *dout;
    float *dz;
    int nfull;            // as FwdArgs::nfull
    int tHd, tL[8], tT2;  // image k-slots
    int flags;
    uint32_t *queue;      // as FwdArgs
    int nblk;
    const int *n_dev;     // as FwdArgs
    int ncu;
};

// relu' bits of a trunk layer's output tiles of this wave, NT n-tiles (the [layer pair][row / 16][64
// lanes] u32 layout), loaded ahead of the GEMM
template <int NT>
struct MaskPre32 {
    uint32_t *mk;          // [NT]
    const uint32_t *word;  // &mask[block][layer pair][the wave's first n-tile][0]; the next n-tile's is 64 words on
    int shift, lane;
    __device__ void operator()() const {
#pragma unroll
        for (int t = 0; t < NT; t++) mk[t] = word[64 * t + lane] >> shift;
    }
};

// relu' bits of the layer input for this wave's 16 x 64 tile (u16 tiles: TH), loaded ahead of the GEMM
struct MaskPre {
    uint32_t *mk;
    const unsigned short *tile;  // &mask[block][mr][0]
    int lane;
    __device__ void operator()() const { *mk = tile[lane]; }
};

// the dX chain's row statistics (launch constants): wstat[L] over tL[L]'s n-tiles (max column abs sum
// of W_L), wstat[8] over the heads' transposed image; published by the first block's staging barriers
__device__ inline void load_wstats_bwd(const BwdArgs &a, ScaleLDS *sc) {
    if (threadIdx.x < 10) sc->wstat[threadIdx.x] = 0;
    __syncthreads();
    const int i = threadIdx.x;
    if (i < 16) {
        lds_fmax(&sc->wstat[8], tile_stat(a.img + (size_t)(a.tHd + i) * KSLOT));
    } else if (i < 16 + 7 * 32) {
        const int L = 1 + (i - 16) / 32, t = (i - 16) % 32;
        if (t < layer_kpad(L) / 16) lds_fmax(&sc->wstat[L], tile_stat(a.img + (size_t)(a.tL[L] + t * 8) * KSLOT));
    }
}

// dOut -> dz rows Z_G (heads' dW) and the split G image, scaled by its max |dOut| per column tile
template <int NQB, int NTH>
__device__ inline void stage_dout(const BwdArgs &a, h16x8 *lds, ScaleLDS *sc, float *stage, int npts, int p0, int tid) {
    constexpr int BMB = 16 * NQB;
    const Flags F = make_flags(a.flags);
    if (tid < 32) (&sc->bsync[0][0])[tid] = 0;
    for (int e = tid; e < 32 * BMB; e += NTH) {
        const int c = e / BMB, m = e % BMB;
        const int p = p0 + m;
        const float v = (p < npts && c < F.nout) ? a.dout[(size_t)p * F.nout + c] : 0.f;
        a.dz[(size_t)(Z_G + c) * a.Ns + p] = v;
        stage[c * BM + m] = v;
    }
    __syncthreads();
    for (int e = tid; e < 32 * BMB; e += NTH) {
        const int c = e / BMB, m = e % BMB;
        lds_fmax(&sc->bsync[BS_G][qof(m)], fabsf(stage[c * BM + m]));
    }
    __syncthreads();
    if (tid < 4) {
        const float gmax = __uint_as_float(sc->bsync[BS_G][tid]);
        sc->ksc[G_BG / 4][tid] = scale_for(gmax).inv;
        sc->ain[0][tid] = gmax;
    }
    if (tid < 4 * BMB) {
        const int g = tid / BMB, m = tid % BMB;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = stage[(8 * g + j) * BM + m];
        put_unit8(lds, G_BG + g, m, v, scale_for(__uint_as_float(sc->bsync[BS_G][qof(m)])).s);
    }
    lds_barrier();
}

// The output scales of a dX-chain step per column tile: max_cols sum |W| x max |dZ in| (the relu' mask
// only zeroes), the same on every wave
template <int NQB>
__device__ inline void chain_scales(const ScaleLDS *sc, float ws, int par, int nw, float (&so)[NQB]) {
    const float4 am = par < 0 ? *reinterpret_cast<const float4 *>(sc->ain[0]) : amax_of4(sc, par, nw);
#pragma unroll
    for (int q = 0; q < NQB; q++) so[q] = ws * f4get(am, q);
}

// One chain step's epilogue for wave r's NT n-tiles (A images at Aw + t * astride): undo the scales,
// relu' mask, dz rows zrow + 16 (NT r + t) .., the output scales (ws: the step's row statistic; par_in:
// the parity of the input's published maxima, < 0: dOut's), then the hand-off: the wave overwrites H
// k-step hk = NT r / 2 once all 16 / NT waves have read it in this step, and signals it written.
template <int NQB, int NT>
__device__ __forceinline__ void chain_epilogue(const BwdArgs &a, h16x8 *lds, uint32_t *hwr, uint32_t *hrd, ScaleLDS *sc,
                                               f32x4 (&c)[NT][NQB], const float (&ib)[NQB], const h16x8 *Aw, int astride,
                                               const uint32_t (&mk)[NT], int zrow, float ws, int par_in, uint32_t step,
                                               int r, int lane, int p0) {
    constexpr int NW = NWAVE / NT;
    const int hk = (NT * r) >> 1;
    float my[NQB] = {};
#pragma unroll
    for (int t = 0; t < NT; t++) {
        scale_tiles(c[t], a_inv(Aw + t * astride), ib);
        mask_apply(c[t], mk[t]);
#ifndef DGS_DIAG_NOSAVE  // diagnostic only (wrong dW): the dZ chain's stores skipped
        tile16(a.dz, a.Ns, zrow + 16 * (NT * r + t), p0, lane).store(c[t]);
#endif
        col_absmax(c[t], my);
    }
    float so[NQB];
    chain_scales(sc, ws, par_in, NW, so);
    col_wave_max(my);
    if (step > 0) lds_wait_ge(hrd + hk, (uint32_t)NW * step, lds_peek(hrd + hk));
#pragma unroll
    for (int q = 0; q < NQB; q++) {
        const Scale s = scale_for(so[q]);
        if (lane == 0) {
            sc->amax[step & 1][r][q] = my[q];
            sc->ksc[G_BH / 4 + hk][q] = s.inv;
        }
#pragma unroll
        for (int t = 0; t < NT; t++) acc_to_lds(c[t][q], lds, G_BH, NT * r + t, q, lane, s.s);
    }
    lds_signal(hwr + hk, lane);
}

// One block of the dX chain (NQB, npts, p0, slot: as fwd_block). NT: n-tiles per wave. NT = 1: 16 waves, two
// writers per H k-step and step; NT = 2 (k_bwd8: a frame-uniform t, every training step): 8 waves, wave
// r writes dZ rows 32r .. 32r + 31 = H k-step r (one writer, 8 readers). Same arithmetic, scales,
// layouts and outputs either way.
// TE_ROWS: per-point dL/dt_emb (blender, t not frame-uniform; NT = 1); without it the block carries no
// t_emb registers or code (raw t PE has no parameters upstream; uniform t: k_tgrad)
template <bool TE_ROWS, int NQB, int NT>
__device__ __forceinline__ void bwd_block(const BwdArgs &a, h16x8 *lds, uint32_t *hwr, uint32_t *hrd, ScaleLDS *sc,
                                          int npts, int p0, int slot) {
    static_assert(NT == 1 || (NT == 2 && !TE_ROWS), "two n-tiles per wave: no t_emb rows");
    constexpr uint32_t HWR = 2 / NT;  // writer waves of an H k-step
    float *lf = reinterpret_cast<float *>(lds);
    float *stage = lf + G_BH * UG * 4;  // fp32 [32][BM] (H region, before the first dZ)
    // re-derived per block (opaque to loop-invariant hoisting): in the persistent loop, lane
    // addresses hoisted out of it would stay live across the whole block and spill
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int r = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Flags F = make_flags(a.flags);
    const uint32_t *mwords = a.mask + (size_t)slot * 2 * F.nmask;
    auto trunk_pre = [&](uint32_t *mk, int L) {  // layer L's output tiles NT r .. of this wave
        return MaskPre32<NT>{mk, mwords + (size_t)(16 * (L >> 1) + NT * r) * 64, 16 * (L & 1), lane};
    };
    if (tid < 8) {
        hwr[tid] = 0;
        hrd[tid] = 0;
    }
    stage_dout<NQB, NTHR / NT>(a, lds, sc, stage, npts, p0, tid);
    f32x4 c[NT][NQB];
    float ib[NQB];
    // The dZ chain runs without workgroup barriers (see fwd_block's trunk): step 0 (heads^T) and steps
    // i = 1..7 (layer L = 8 - i) each write dZ into H; step i reads H once the HWR writers of each
    // k-step have signalled (hwr >= HWR i) and overwrites its own k-step once all waves have read it
    // (chain_epilogue).
    {  // heads^T: dH7 = W_h^T dOut (K = 32 from G) -> mask H7 -> dZ7
        uint32_t mk[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) zero_tiles(c[t]);
        const h16x8 *Ah = a.img + (size_t)(a.tHd + NT * r) * KSLOT;
        gemm<NT, 1, NQB>(Ah, KSLOT, lds, G_BG, 0, lane, c, ib, sc->ksc, trunk_pre(mk, 7));
        chain_epilogue(a, lds, hwr, hrd, sc, c, ib, Ah, KSLOT, mk, Z_L0 + 7 * 256, __uint_as_float(sc->wstat[8]), -1,
                       0u, r, lane, p0);
    }
    f32x4 te5[1][1] = {{zero4()}};  // t_emb tile of layer 5's dX (waves 0-7, TE_ROWS), true units
#pragma unroll 1
    for (int L = 7; L >= 1; L--) {
        const uint32_t step = 8 - L;
        // dX_L = W_L^T dZ_L; the H-part rows of the padded L5 input are n-tiles F_H / 16 + NT r ..
        if (TE_ROWS && L == 5 && r < 2 * NQB) {  // t_emb rows (padded 64..95 = n-tiles 4, 5) x column tile r % NQB
            const h16x8 *At = a.img + (size_t)(a.tL[5] + (F_TE / 16 + r / NQB) * 8) * KSLOT;
            float ib1[1];
            gemm<1, 8, 1>(At, 0, lds, G_BH, r % NQB, lane, te5, ib1, sc->ksc, NoPre(),
                          HGate{hwr, hrd, 0, HWR * step, false, lane});
            te5[0][0] *= a_inv(At) * ib1[0];
        }
        const int tile0 = (L == 5) ? F_H / 16 : 0;
        uint32_t mk[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) zero_tiles(c[t]);
        const h16x8 *Aw = a.img + (size_t)(a.tL[L] + (tile0 + NT * r) * 8) * KSLOT;
        gemm<NT, 8, NQB>(Aw, 8 * KSLOT, lds, G_BH, 0, lane, c, ib, sc->ksc, trunk_pre(mk, L - 1),
                         HGate{hwr, hrd, 0, HWR * step, true, lane});
        chain_epilogue(a, lds, hwr, hrd, sc, c, ib, Aw, 8 * KSLOT, mk, Z_L0 + (L - 1) * 256,
                       __uint_as_float(sc->wstat[L]), (int)((step - 1) & 1), step, r, lane, p0);
    }
    if constexpr (TE_ROWS) {
        const size_t Ns = a.Ns;
        f32x4(&c0)[NQB] = c[0];
        // layer 0's t_emb rows added to layer 5's: dTE tile (n-tile r / NQB, column tile r % NQB) -> dz rows
        // Z_TE (timenet.2's dW) and the split G image (dOut's, no longer read), scaled by its column tile's max
        if (r < 2 * NQB) {
            const int nt = r / NQB, q = r % NQB;
            f32x4 t0[1][1] = {{zero4()}};
            float ib1[1];
            const h16x8 *At = a.img + (size_t)(a.tL[0] + (F_TE / 16 + nt) * 8) * KSLOT;
            gemm<1, 8, 1>(At, 0, lds, G_BH, q, lane, t0, ib1, sc->ksc, NoPre(), HGate{hwr, hrd, 0, HWR * 8u, false, lane});
            te5[0][0] += t0[0][0] * (a_inv(At) * ib1[0]);
            tile16(a.dz, Ns, Z_TE + 16 * nt, p0, lane).store(te5[0], q);
            float tm[1] = {0.f};
            col_absmax(te5[0], tm);
            col_wave_max(tm);
            if (lane == 0) lds_fmax(&sc->bsync[BS_GTE][q], tm[0]);
        }
        lds_barrier();
        if (r < 2 * NQB)
            acc_to_lds(te5[0][0], lds, G_BG, r / NQB, r % NQB, lane,
                       scale_for(__uint_as_float(sc->bsync[BS_GTE][r % NQB])).s);
        if (tid < 4) sc->ksc[G_BG / 4][tid] = scale_for(__uint_as_float(sc->bsync[BS_GTE][tid])).inv;
        lds_barrier();
        // timenet.2^T: dTH = W_T2^T dTE (K = 32) -> mask TH -> dZ_T1
        {
            const unsigned short *mtiles = reinterpret_cast<const unsigned short *>(mwords);
            uint32_t mk;
            zero_tiles(c0);
            const h16x8 *A2 = a.img + (size_t)(a.tT2 + r) * KSLOT;
            gemm<1, 1, NQB>(A2, 0, lds, G_BG, 0, lane, c, ib, sc->ksc, MaskPre{&mk, mtiles + (size_t)(MR_TH + r) * 64, lane});
            scale_tiles(c0, a_inv(A2), ib);
            mask_apply(c0, mk);
            tile16(a.dz, Ns, Z_T1 + 16 * r, p0, lane).store(c0);
        }
    }
}

// A dX-chain workgroup of 16 / NT waves: LDS, row statistics, then block after block from the queue
template <bool TE_ROWS, int NT>
__device__ __forceinline__ void bwd_kernel(const BwdArgs &a) {
    __shared__ h16x8 lds[G_BWD * UG];
    __shared__ uint32_t hwr[8], hrd[8];  // dZ hand-off counters (HGate), as in the forward's trunk
    __shared__ int s_next;
    __shared__ ScaleLDS sc;
    load_wstats_bwd(a, &sc);
    CLK_BEGIN();
    int npts = a.N, nfull = a.nfull, nblk = a.nblk;
    if (a.n_dev) {  // as fwd_kernel
        npts = device_points(a.n_dev, a.N);
        const Blocks bs = split_blocks(npts, a.ncu);
        nfull = bs.nfull;
        nblk = bs.nfull + bs.ntail;
    }
    for (int b = blockIdx.x; b < nblk;) {  // persistent: as fwd_kernel
        int nx = 0;
        if (a.queue && threadIdx.x == 0) nx = queue_take(a.queue);
        if (b < nfull) bwd_block<TE_ROWS, NQ, NT>(a, lds, hwr, hrd, &sc, npts, b * BM, b);
        else bwd_block<TE_ROWS, 1, NT>(a, lds, hwr, hrd, &sc, npts, nfull * BM + (b - nfull) * 16, b);
        if (!a.queue) break;
        if (threadIdx.x == 0) s_next = nx;
        __syncthreads();
        b = s_next;
        if (b >= nblk) break;
    }
    if (a.queue) queue_release(a.queue);
    if constexpr (NT == 1) CLK_END(1);  // (diagnostic clock stamps: the 16-wave kernels only)
}

template <bool TE_ROWS>
__global__ __launch_bounds__(NTHR) void k_bwd(BwdArgs a) {
    bwd_kernel<TE_ROWS, 1>(a);
}

// the dX chain for a frame-uniform t (every training step): 8 waves of two n-tiles
__global__ __launch_bounds__(NTHR8) void k_bwd8(BwdArgs a) { bwd_kernel<false, 2>(a); }


// Timenet gradients for a frame-uniform t (DGS_MLP_UNIFORM_T). With one TIN / TH for every point,
// dL/dt_emb summed over points is S = W0[:, TE]^T gb0 + W5[:, TE]^T gb5 (gb = the layer-0 / 5 bias
// gradients = sums of dZ over points), and then
//   timenet.2: dW = S TH^T, db = S;   dZ_T1 = relu'(TH) (W_T2^T S);   timenet.0: dW = dZ_T1 TIN^T, db = dZ_T1
// — the per-point sums of the general path (time_utils.py:74-76 autograd) regrouped. TG_WG
// workgroups: each evaluates S (same order in every one: identical values) and writes the outputs
// of its TG_N rows n (the single-workgroup version was a 17 us latency chain); bitwise deterministic.
constexpr int TG_WG = 8, TG_N = 256 / TG_WG;
struct TGradArgs {
    const float *fp;
    int w0te, w5te, wT2;  // fp32 [256][32] t_emb columns of linear.0 / linear.5, [32][256] timenet.2
    const float *tc;      // k_timenet's TIN / TH
    const float *gb0, *gb5;
    float *gT0w, *gT0b, *gT2w, *gT2b;
    float *gW0, *gW5;     // linear.0 / linear.5 weight gradients: their folded t_emb columns
    int tin;
};

__global__ __launch_bounds__(1024) void k_tgrad(TGradArgs a) {
    __shared__ float S[32], th[TG_N], dz1[TG_N], Sp[32][33];
    const int j = threadIdx.x;
    const int n0 = blockIdx.x * TG_N;
    if (j < TG_N) th[j] = a.tc[TC_TH + n0 + j];
    {  // S[k]: thread (part, k) sums 16 of the 512 (n, layer) terms (a wave reads two 128-B rows of
       // the [n][32] weight images per step: coalesced), then 32 threads add the parts in order
        const int k = j & 31, part = j >> 5;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int n = part * 16 + i;  // n < 256: linear.0, else linear.5
            const float w = n < 256 ? a.fp[a.w0te + n * 32 + k] : a.fp[a.w5te + (n - 256) * 32 + k];
            const float gb = n < 256 ? a.gb0[n] : a.gb5[n - 256];
            s = fmaf(w, gb, s);
        }
        Sp[part][k] = s;
        __syncthreads();
        if (j < 32) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 32; q++) t += Sp[q][j];
            S[j] = t;
        }
    }
    // the folded t_emb columns 63..92 of linear.0 / linear.5: dW = gb (x) te (the dW kernel covers
    // x_emb and h only)
    for (int e = j; e < TG_N * 30; e += 1024) {
        const int n = n0 + e / 30, k = e % 30;
        const float te = a.tc[TC_TE + k];
        a.gW0[n * 93 + 63 + k] = a.gb0[n] * te;
        a.gW5[n * 349 + 63 + k] = a.gb5[n] * te;
    }
    __syncthreads();
    for (int e = j; e < 30 * TG_N; e += 1024) {
        const int k = e / TG_N, n = e % TG_N;
        a.gT2w[k * 256 + n0 + n] = S[k] * th[n];
    }
    if (blockIdx.x == 0 && j < 30) a.gT2b[j] = S[j];
    if (j < 4 * TG_N) {  // dZ_T1[n]: 4 lanes per n over 8 of the 30 (+2 zero) k terms each, then a fixed xor tree
        const int n = j >> 2, q = j & 3;
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int k = q * 8 + i;
            if (k < 30) d = fmaf(a.fp[a.wT2 + k * 256 + n0 + n], S[k], d);
        }
        d += __shfl_xor(d, 1);
        d += __shfl_xor(d, 2);
        d = th[n] > 0.f ? d : 0.f;
        if (q == 0) {
            dz1[n] = d;
            a.gT0b[n0 + n] = d;
        }
    }
    __syncthreads();
    for (int e = j; e < TG_N * a.tin; e += 1024) {  // coalesced [256][tin] outer product (this block's rows)
        const int n = e / a.tin, f = e - n * a.tin;
        a.gT0w[(n0 + n) * a.tin + f] = dz1[n] * a.tc[TC_TIN + f];
    }
}

}  // namespace mlps
}  // namespace dgs
