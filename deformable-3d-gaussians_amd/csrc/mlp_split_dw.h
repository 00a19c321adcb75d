// Fused deformation MLP on split f16, dW (device code of mlp_split.hip's translation unit): k_dws.
#pragma once
#include "mlp_split_core.h"

namespace dgs {
namespace mlps {

// ------------------------------------------------------------------------------------------------
// dW = dZ X^T on split f16 (k_dws, the default dW). Per job tile (<= 256 dZ rows x 256 X rows) and
// 32-point chunk, each wave owns 32 rows of ONE operand ("private": loaded, scaled, split and kept as
// MFMA fragments in its own registers) against all rows of the other ("shared": staged by the whole
// workgroup, scaled and split once, through LDS):
//   COL (krows = 256 jobs): private = X rows 32 w..+31, shared = dZ rows (NS tiles)
//   ROW (krows <= 96 jobs): private = dZ rows 32 w..+31, shared = X rows (NS tiles)
// so every fp32 value is split exactly once per workgroup and only the shared operand makes the LDS
// round trip. The private fragments are always the A operand and the shared ones B (the 32x32x16 A and
// B lane maps are the same): a tile's MFMA output is [private row][shared row], lane i holding shared
// row i. Per chunk: split the private registers -> fragments | MFMAs on LDS buffer c & 1 with the next
// chunk's shared split (2 ds_write_b64 per float4) and loads interleaved | ONE barrier.
//   Scales (power of two, as the forward): the private operand one per (wave, chunk) from the wave's
// max over its 32 rows x 32 points; the shared operand one per (row, chunk) from the 8 lanes that stage
// the row (3 DPP steps), kept in LDS beside the planes. Lane i of a tile's output then carries ONE
// inverse scale (private x shared row i), applied when the chunk's fresh accumulator T joins the
// running sum: acc = T * s + acc (one fma per element, where the bf16x6 split had one add).
//   LDS: split planes in fragment order, unit (16 B) [split][k-step][32-row block][lane = 32 h + i]
//   (row i, points 8h..8h+7): a fragment is one conflict-free ds_read_b128 per split; 2 x 32 KiB.
//   Numerics: each tile's six products of a chunk (per k-step the two corrections, then hh) go into a
// fresh accumulator T, added to the running sum in fp32 (tools/mfma_accum_probe.hip: a long running
// MFMA C loses the low bits of small terms with a bias; within one chunk's T that loss stays below
// fp32's own rounding of T).
//   Output: ROW jobs' tiles are [dZ row][X row] (the slab's own layout, stored as before); COL jobs'
// are [X row][dZ row] and go through a per-wave LDS transpose so the slab stores stay coalesced.
// Same job plan, slab layout and k_dw_reduce (mlp_dw_reduce.h) as the fp32 k_dw (mlp_dw_fp32.h).
//   Ns is the row stride of both operands; ext <= Ns (a multiple of BM) is the extent the chunks cover: the
// whole allocation, or the active set's padded point count (n_dev, mlp_active.h), beyond which the rows
// hold other launches' values that no chunk reads. ext = 0: every slab is written as zeros.
// ------------------------------------------------------------------------------------------------
constexpr int DW_THREADS = 512;
constexpr int S_UNITS = NSPLIT * 2 * 8 * 64;  // 16-B units per chunk buffer
constexpr int S_NBUF = 2;
constexpr int S_RSC = WT;                     // shared-row inverse scales per buffer (floats)
constexpr int S_LDS = S_NBUF * S_UNITS * 16 + S_NBUF * S_RSC * 4;  // bytes (66 KiB)
constexpr int S_TRP = 32 * 33;                // per-wave transpose scratch (floats), after the loop
static_assert(S_LDS <= 160 * 1024 && 8 * S_TRP * 4 <= S_LDS, "dWs LDS");

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#ifdef DGS_DIAG_DWS_L2  // diagnostic (wrong results): every chunk re-reads the split's first chunk (L2-resident)
#define DWS_DIAG_C(c) (c0)
#else
#define DWS_DIAG_C(c) (c)
#endif

// unit of (split p, k-step ks, row block rb, point half hh, row i): each 32-unit half is rotated
// by 4 ks + 2 hh, so the row-major staging stores (8 lanes per row: all (ks, hh, 8-byte half)
// combinations of 2 rows per 16-lane group) hit 32 distinct banks; a fragment read stays one
// conflict-free 1 KiB ds_read_b128
__device__ __forceinline__ constexpr int s_unit(int p, int ks, int rb, int hh, int i) {
    return ((p * 2 + ks) * 8 + rb) * 64 + 32 * hh + ((i + 4 * ks + 2 * hh) & 31);
}

__device__ __forceinline__ AFrag s_frag(const h16x8 *L, int ks, int rb, int lane) {
    const int hh = lane >> 5, i = lane & 31;
    return AFrag{L[s_unit(0, ks, rb, hh, i)], L[s_unit(1, ks, rb, hh, i)]};
}

// 8 fp32 (one row, points 8h .. 8h + 7) times S -> the hi / lo f16 fragments
__device__ __forceinline__ AFrag split8(const float4 &a, const float4 &b, float S) {
    uint32_t h[4], l[4];
    hsplit2(a.x * S, a.y * S, h[0], l[0]);
    hsplit2(a.z * S, a.w * S, h[1], l[1]);
    hsplit2(b.x * S, b.y * S, h[2], l[2]);
    hsplit2(b.z * S, b.w * S, h[3], l[3]);
    return AFrag{__builtin_bit_cast(h16x8, make_uint4(h[0], h[1], h[2], h[3])),
                 __builtin_bit_cast(h16x8, make_uint4(l[0], l[1], l[2], l[3]))};
}

__device__ __forceinline__ float sum8(const float4 &a, const float4 &b) {
    return ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
}

__device__ __forceinline__ float absmax4(const float4 &v) {
    return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// one k-step's three products into t (the two corrections first)
__device__ __forceinline__ f32x16 mma3_into(const AFrag &a, const AFrag &b, f32x16 t) {
    t = MFMA32(a.l, b.h, t);
    t = MFMA32(a.h, b.l, t);
    return MFMA32(a.h, b.h, t);
}

// max over the 8 consecutive lanes (aligned groups) of non-negative floats, in every lane of the group:
// quad_perm [1,0,3,2], [2,3,0,1], then row_half_mirror
__device__ __forceinline__ float max8(float v) {
    uint32_t x = __float_as_uint(v);
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xb1, 0xf, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4e, 0xf, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xf, 0xf, false));
    return __uint_as_float(x);
}

template <bool COL, int NS>
__device__ __forceinline__ void dws_run(const WJob &J, size_t Ns, size_t ext, const float *__restrict__ dz,
                                        const float *__restrict__ saved, float *__restrict__ slabs, h16x8 *lds) {
    constexpr int SROWS = 32 * NS;                   // shared rows staged per chunk
    constexpr int NSF = (SROWS * 8 + 511) / 512;     // staged float4 per thread per chunk
    const int split = blockIdx.x - J.block0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, i = lane & 31;
    const int nch = (int)(ext / 32);
    const int per = div_up(nch, J.nsplit);
    const int c0 = split * per;
    const int c1 = min(nch, c0 + per);
    // operands through buffer descriptors whose record count ends at the job's extent: rows past
    // it read as zero (32-bit offsets: the host keeps 256 rows x Ns x 4 B below 2^31)
    const float *zb = dz + (size_t)J.zrow * Ns, *xb = saved + (size_t)J.xrow * Ns;
    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(COL ? zb : xb), 0, (int)((COL ? J.nrows : J.krows) * Ns * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(COL ? xb : zb), 0, (int)((COL ? J.krows : J.nrows) * Ns * 4), 0x00020000);
    const bool pact = 32 * wave < (COL ? J.krows : J.nrows);  // this wave has private rows (uniform)
    // private: lane (i, h) holds row 32 w + i, points 8 h .. + 7 of each k-step (fragment layout)
#ifdef DGS_DIAG_DWS_TILED  // diagnostic (wrong results): chunk-major addressing [chunk][row][32 points]
    const int pvoff = ((32 * wave + i) * 32 + 8 * h) * 4;
    const int pcst = (COL ? J.krows : J.nrows) * 128, scst = (COL ? J.nrows : J.krows) * 128;
#else
    const int pvoff = ((32 * wave + i) * (int)Ns + 8 * h) * 4;
    constexpr int pcst = 128, scst = 128;
#endif
    float4 pr[4];  // [k-step][half]
    auto pload = [&](int c) {
#pragma unroll
        for (int q = 0; q < 4; q++)
            pr[q] = __builtin_bit_cast(float4,
                                       __builtin_amdgcn_raw_buffer_load_b128(rsP, pvoff, DWS_DIAG_C(c) * pcst + (q >> 1) * 64 + (q & 1) * 16, 0));
    };
    // shared staging: slot g = tid + 512 f -> row g >> 3, points 4 (g & 7) .. + 3 of the chunk (8
    // lanes read a row's 128 B)
    float4 st[NSF];
    auto sslot = [&](int f, int &row, int &q) {
        const int g = tid + 512 * f;
        row = g >> 3;
        q = g & 7;
        return SROWS * 8 % 512 == 0 || g < SROWS * 8;
    };
    auto sload = [&](int c) {
#pragma unroll
        for (int f = 0; f < NSF; f++) {
            int row, q;
            if (sslot(f, row, q))
                st[f] = __builtin_bit_cast(
#ifdef DGS_DIAG_DWS_TILED
                    float4, __builtin_amdgcn_raw_buffer_load_b128(rsS, (row * 32 + 4 * q) * 4, DWS_DIAG_C(c) * scst, 0));
#else
                    float4, __builtin_amdgcn_raw_buffer_load_b128(rsS, (row * (int)Ns + 4 * q) * 4, DWS_DIAG_C(c) * scst, 0));
#endif
        }
    };
    float bsum[NSF] = {};  // COL: bias row sums of the staged dZ rows; ROW: bsum[0] of the private row
    char *lb = reinterpret_cast<char *>(lds);
    float *rsc = reinterpret_cast<float *>(lb + S_NBUF * S_UNITS * 16);  // [buffer][row]
    // `live`: the staged chunk is a real one (the last chunk re-splits a stale copy into the buffer
    // nobody reads again; it must not count in the bias sums)
    auto sput = [&](int f, int buf, bool live) {
        int row, q;
        const bool ok = sslot(f, row, q);
        const float4 v = st[f];
        // the row's scale: max over its 8 staging lanes (a partial last slot group lies in one wave, past
        // the valid rows: its lanes see zeros, never a valid row's)
#ifdef DGS_DIAG_DWS_NOSCALE  // diagnostic (wrong results): constant scales, no per-chunk maxima
        const Scale s = Scale{1024.f, 1.f / 1024.f};
#else
        const Scale s = scale_for(max8(ok ? absmax4(v) : 0.f));
#endif
        if (!ok) return;
        if (COL) bsum[f] += live ? (v.x + v.y) + (v.z + v.w) : 0.f;
        const Split4 sp = split4(v.x, v.y, v.z, v.w, s.s);
        char *p = lb + buf * (S_UNITS * 16) +
                  s_unit(0, q >> 2, row >> 5, (q >> 1) & 1, row & 31) * 16 + 8 * (q & 1);
        *reinterpret_cast<h16x4 *>(p) = sp.h;
        *reinterpret_cast<h16x4 *>(p + 2 * 8 * 64 * 16) = sp.l;
        // the row's 8 lanes store the same value (a `q == 0` branch here split the block and cost 72
        // VGPRs of spills)
        rsc[buf * S_RSC + row] = s.inv;
    };
    f32x16 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[s][r] = 0.f;
    if (c0 < c1) {
        sload(c0);
        pload(c0);
#pragma unroll
        for (int f = 0; f < NSF; f++) sput(f, 0, true);
        sload(min(c0 + 1, c1 - 1));
    }
    lds_barrier();
    // shared float4 f of the next chunk is split after tile put_at(f) of this one (within the first
    // half of the tiles), then the loads of the chunk after are issued
    constexpr int NH = (NS + 1) / 2;
    auto put_at = [](int f) { return (f * NH) / NSF; };
    auto chunk = [&](int c, auto BUFC) {
        constexpr int buf = decltype(BUFC)::value;
        const h16x8 *L = lds + buf * S_UNITS;
        const bool more = c + 1 < c1;
        if (pact) {
            // private fragments of this chunk (scaled by the wave's max), then the private loads of
            // the next (in flight for the whole chunk)
#ifdef DGS_DIAG_DWS_NOSCALE
            const Scale sp = Scale{1024.f, 1.f / 1024.f};
#else
            const float pm = wave_max(fmaxf(fmaxf(absmax4(pr[0]), absmax4(pr[1])), fmaxf(absmax4(pr[2]), absmax4(pr[3]))));
            const Scale sp = scale_for(pm);
#endif
            AFrag pf0 = split8(pr[0], pr[1], sp.s), pf1 = split8(pr[2], pr[3], sp.s);
            if (!COL) bsum[0] += sum8(pr[0], pr[1]) + sum8(pr[2], pr[3]);
            pload(min(c + 1, c1 - 1));
#pragma unroll
            for (int s = 0; s < NS; s++) {
                // the tile's two k-steps into a fresh accumulator, one shared fragment live at a time
                const float si = sp.inv * rsc[buf * S_RSC + 32 * s + i];
                const AFrag s0 = s_frag(L, 0, s, lane);
#ifdef DGS_DIAG_DWS_NOFOLD  // diagnostic (wrong results): the MFMAs accumulate into acc directly
                acc[s] = mma3_into(pf0, s0, acc[s]);
                const AFrag s1 = s_frag(L, 1, s, lane);
                acc[s] = mma3_into(pf1, s1, acc[s]);
                (void)si;
#else
                f32x16 T = mma3_into(pf0, s0, (f32x16)(0.f));
                const AFrag s1 = s_frag(L, 1, s, lane);
                T = mma3_into(pf1, s1, T);
#pragma unroll
                for (int r = 0; r < 16; r++) acc[s][r] = fmaf(T[r], si, acc[s][r]);
#endif
#pragma unroll
                for (int f = 0; f < NSF; f++)
                    if (put_at(f) == s) sput(f, buf ^ 1, more);
                if (s == put_at(NSF - 1)) sload(min(c + 2, c1 - 1));
            }
        } else {
            pload(min(c + 1, c1 - 1));  // (keeps the waves' vmcnt streams alike; reads row 0 + OOB zeros)
#pragma unroll
            for (int f = 0; f < NSF; f++) sput(f, buf ^ 1, more);
            sload(min(c + 2, c1 - 1));
        }
        lds_barrier();
    };
    for (int c = c0; c < c1; c += 2) {
        chunk(c, std::integral_constant<int, 0>{});
        if (c + 1 < c1) chunk(c + 1, std::integral_constant<int, 1>{});
    }
    float *slab = slabs + (size_t)blockIdx.x * SLAB;
    if (COL) {
        // bias row sums: the 8 lanes staging a row hold its partial sums (fixed xor-tree order)
#pragma unroll
        for (int f = 0; f < NSF; f++) {
            float v = bsum[f];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            int row, q;
            if (sslot(f, row, q) && q == 0) slab[WT * WT + row] = v;
        }
    } else if (pact) {
        const float v = bsum[0] + __shfl_xor(bsum[0], 32);
        if (h == 0) slab[WT * WT + 32 * wave + i] = v;
    }
    if (!pact) return;
    // rows past nrows / cols past krows hold zeros that k_dw_reduce never reads
    if (!COL) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int nb = 32 * wave, kb = 32 * s;
#pragma unroll
            for (int r = 0; r < 16; r++) slab[(nb + TileAddr::row(r) + 4 * h) * WT + kb + i] = acc[s][r];
        }
        return;
    }
    // COL: tile s is [X row 32 w + row(r) + 4 h][dZ row 32 s + i]; through this wave's LDS scratch so
    // that 32 lanes store 32 consecutive X rows of one dZ row (the last chunk's barrier ended every
    // wave's reads of the planes)
    float *tp = reinterpret_cast<float *>(lds) + wave * S_TRP;
#pragma unroll
    for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int r = 0; r < 16; r++) tp[i * 33 + TileAddr::row(r) + 4 * h] = acc[s][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's LDS writes before its reads
#pragma unroll
        for (int rr = 0; rr < 16; rr++) {
            const int m = 2 * rr + h;  // dZ row 32 s + m, X rows 32 w + i
            slab[(32 * s + m) * WT + 32 * wave + i] = tp[m * 33 + i];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // the reads done before the next tile's writes
    }
}

__global__ __launch_bounds__(DW_THREADS) void k_dws(WJobs JT, size_t Ns, int N, const int *__restrict__ n_dev,
                                                    const float *__restrict__ dz, const float *__restrict__ saved,
                                                    float *__restrict__ slabs) {
    extern __shared__ h16x8 dws_lds[];
    const size_t ext = n_dev ? (size_t)div_up(device_points(n_dev, N), BM) * BM : Ns;
    WJob J = JT.j[0];
#pragma unroll
    for (int q = 1; q < MAXJ; q++)
        if (q < JT.n && (int)blockIdx.x >= JT.j[q].block0) J = JT.j[q];
    // job shapes (host-checked in dw_split_once): krows = 256 with nrows 256 or 32 -> COL; nrows =
    // 256 with krows 96, 64 (folded t_emb) or 16 -> ROW
    CLK_BEGIN();
    if (J.krows == 256) {
        if (J.nrows == 256)
            dws_run<true, 8>(J, Ns, ext, dz, saved, slabs, dws_lds);
        else
            dws_run<true, 1>(J, Ns, ext, dz, saved, slabs, dws_lds);
    } else if (J.krows > 64) {
        dws_run<false, 3>(J, Ns, ext, dz, saved, slabs, dws_lds);
    } else if (J.krows > 32) {
        dws_run<false, 2>(J, Ns, ext, dz, saved, slabs, dws_lds);
    } else {
        dws_run<false, 1>(J, Ns, ext, dz, saved, slabs, dws_lds);
    }
    CLK_END(2);
}

}  // namespace mlps
}  // namespace dgs
