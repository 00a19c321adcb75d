// Rasterizer, binning stage (device code of raster.hip's translation unit; the pipeline map is at the top
// of raster.hip): from the per-Gaussian tile rectangles to every tile's depth-ordered list and range.
//   k_rect_count     rect binning, Gaussians in index order: per (256-Gaussian block, tile) pair counts
//   k_rect_colscan   column scan of the count matrix -> tile starts and ranges; stores the pair count into
//                    a pinned host word the host polls (speculative binning: no event, no copy)
//   k_rect_place     every block writes its Gaussians' ids into its slice of each tile's list
//   k_tile_sort      per-tile stable sort of the list by depth key (LDS; global scratch for long lists)
//   k_rect_gather    DGS_DETERMINISTIC=1: sums the blend backward's per-pair slots in k_rect_place's order
//   k_duplicate, k_ranges   DGS_BINNING=sort: (tile, id) pairs in global depth order for the stable radix
//                    sort on the tile bits, then the ranges
//   k_clip_ranges    a deferred pair count that overflowed: the ranges clipped to the launched capacity
#pragma once
#include "raster_kernels.h"

namespace dgs {

// Pairs are emitted in depth order (Gaussians pre-sorted by depth, stable on the index), so a
// stable sort on the tile id alone yields the reference's (tile, depth) key order, ties on the
// Gaussian index included: 2 radix passes over 16-bit keys instead of 6 over 64-bit ones.
template <class KT>
__global__ __launch_bounds__(256) void k_duplicate(int P, const uint32_t *__restrict__ order,
                                                   const float2 *__restrict__ xy, const int *__restrict__ radii,
                                                   const uint32_t *__restrict__ offsets, int gx, int gy,
                                                   KT *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t cap,
                                                   uint2 *__restrict__ ranges, int T) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    // folded fills (no separate memsets): empty tile ranges, and all-ones keys over the
    // speculative capacity past the pair count so the radix sort leaves the padding at the end
    const int nthreads = gridDim.x * blockDim.x;
    for (int t = j; t < T; t += nthreads) ranges[t] = make_uint2(0u, 0u);
    for (uint32_t k = offsets[P - 1] + (uint32_t)j; k < cap; k += (uint32_t)nthreads) keys[k] = (KT)~(KT)0;
    if (j >= P) return;
    const uint32_t g = order[j];
    const int r = radii[g];
    if (r <= 0) return;
    uint32_t off = (j == 0) ? 0u : offsets[j - 1];
    const float2 c = xy[g];
    int x0, y0, x1, y1;
    tile_rect(c.x, c.y, r, gx, gy, x0, y0, x1, y1);
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            if (off < cap) {  // speculative capacity: an overflowing launch is redone by the host
                keys[off] = (KT)(y * gx + x);
                vals[off] = g;
            }
            off++;
        }
}

// ------------------------------------------------------------------------------------------------
// Rect binning (the default for images up to RECT_MAX_TILES tiles): the (tile, Gaussian) pairs are
// placed directly at their position in the tile-sorted order instead of being emitted and radix-
// sorted. The Gaussians are already in depth order (stable on the index), and Gaussian j covers the
// tile rectangle of its 3-sigma radius, so the position of pair (j, t) in the stable tile sort is
//   tile_start[t] + #{j' < j : t in rect(j')}
// counted hierarchically over blocks of 256 depth-ordered Gaussians: k_rect_count (per block and
// tile), k_rect_colscan (exclusive down each tile's column of blocks, tile totals, pair count; its
// last workgroup scans the totals into the tile starts and ranges), k_rect_place (per wave and tile in
// LDS, then the lanes below in the wave). Same order as the sort, bit for bit; no keys.
// ------------------------------------------------------------------------------------------------
constexpr int RECT_MAX_TILES = 12288;     // LDS of the count/place kernels: 4 B per tile (<= 64 KiB)
constexpr long long RECT_MAX_CELLS = 1 << 24;  // blocks x tiles of the count matrix

__device__ inline bool gauss_rect(uint32_t g, const float2 *xy, const int *radii, int gx, int gy, int4 &rc) {
    const int r = radii[g];
    if (r <= 0) return false;
    const float2 c = xy[g];
    tile_rect(c.x, c.y, r, gx, gy, rc.x, rc.y, rc.z, rc.w);
    return rc.x < rc.z && rc.y < rc.w;
}

__global__ __launch_bounds__(256) void k_rect_count(int P, const uint32_t *__restrict__ order, const float2 *__restrict__ xy,
                                                    const int *__restrict__ radii, int gx, int gy,
                                                    uint32_t *__restrict__ cnt, uint32_t *__restrict__ total) {
    extern __shared__ uint32_t h[];  // [T]  (total[0] = pair count, total[1] = column-scan ticket)
    const int T = gx * gy;
    for (int t = threadIdx.x; t < T; t += 256) h[t] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 2) total[threadIdx.x] = 0;  // k_rect_colscan adds into them
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    int4 rc;
    if (j < P && gauss_rect(order ? order[j] : (uint32_t)j, xy, radii, gx, gy, rc))
        for (int y = rc.y; y < rc.w; y++)
            for (int x = rc.x; x < rc.z; x++) atomicAdd(&h[y * gx + x], 1u);
    __syncthreads();
    uint32_t *row = cnt + (size_t)blockIdx.x * T;
    for (int t = threadIdx.x; t < T; t += 256) row[t] = h[t];
}

// tile starts = exclusive scan of the tile totals, and the (unclipped) ranges; one workgroup of
// 1024 threads (the column scan's last workgroup). The totals come as agent-scope atomic words
// tagged with the launch generation (written by the other workgroups, no fences): spin on the tag.
__device__ inline uint32_t tagged_total(const unsigned long long *tot, int t, uint32_t gen) {
    unsigned long long v;
    do {
        v = __hip_atomic_load(tot + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } while ((uint32_t)(v >> 32) != gen);
    return (uint32_t)v;
}

__device__ void rect_starts(int T, const unsigned long long *__restrict__ tot, uint32_t gen, uint32_t *__restrict__ tile_start,
                            uint2 *__restrict__ ranges, uint32_t *wsum, uint32_t *host_total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int MAXPER = 12;  // RECT_MAX_TILES / 1024
    const int per = div_up(T, 1024);
    const int t0 = tid * per;
    uint32_t c[MAXPER], local = 0;
#pragma unroll
    for (int k = 0; k < MAXPER; k++) {
        c[k] = (k < per && t0 + k < T) ? tagged_total(tot, t0 + k, gen) : 0u;
        local += c[k];
    }
    uint32_t x = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t run = x - local;
    for (int k = 0; k < w; k++) run += wsum[k];
#pragma unroll
    for (int k = 0; k < MAXPER; k++) {
        const int t = t0 + k;
        if (k < per && t < T) {
            tile_start[t] = run;
            ranges[t] = make_uint2(run, run + c[k]);
            run += c[k];
        }
    }
    // the pair count straight into the host's pinned word (no copy launch): the last thread's run
    if (host_total && tid == 1023) *host_total = run;
}

// the column of block counts of 64 tiles per workgroup -> exclusive offsets (in place), the tile
// totals, the pair count, then the tile starts and ranges (last workgroup): 16 waves take 32 rows each per 512-row chunk (loads all in flight),
// cross-wave prefix in LDS, carry between chunks
__global__ __launch_bounds__(1024) void k_rect_colscan(int nb, int T, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ tot, uint32_t gen,
                                                       uint32_t *__restrict__ total, uint32_t *__restrict__ ticket,
                                                       uint32_t *__restrict__ tile_start, uint2 *__restrict__ ranges,
                                                       uint32_t *host_total) {
    __shared__ uint32_t part[16][64];
    __shared__ uint32_t carry[64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    const bool ok = t < T;
    if (w == 0) carry[lane] = 0;
    for (int b0 = 0; b0 < nb; b0 += 512) {
        const int r0 = b0 + 32 * w;
        uint32_t v[32], sum = 0;
#pragma unroll
        for (int k = 0; k < 32; k++) {
            v[k] = (ok && r0 + k < nb) ? cnt[(size_t)(r0 + k) * T + t] : 0u;
            sum += v[k];
        }
        part[w][lane] = sum;
        __syncthreads();
        uint32_t run = carry[lane];
        for (int k = 0; k < w; k++) run += part[k][lane];
#pragma unroll
        for (int k = 0; k < 32; k++) {
            if (ok && r0 + k < nb) cnt[(size_t)(r0 + k) * T + t] = run;
            run += v[k];
        }
        __syncthreads();  // carry and part read by every wave
        if (w == 15) carry[lane] = run;
        __syncthreads();
    }
    if (w == 0) {
        const uint32_t c = carry[lane];
        if (ok) __hip_atomic_store(tot + t, ((unsigned long long)gen << 32) | c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t s = c;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o);
        if (lane == 0) atomicAdd(total, s);
    }
    // the last workgroup to take a ticket scans the tile totals
    __shared__ uint32_t wsum[16];
    __shared__ bool last;
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    rect_starts(T, tot, gen, tile_start, ranges, wsum, host_total);
}

__host__ __device__ inline size_t rect_place_lds(int gx, int gy, bool stage) {
    return 4ull * ((gx * gy + 1) & ~1) * (stage ? 2 : 1) + 4ull * 8ull * (gx + gy);
}
// the block's output base per tile (tile start + the block's column offset) staged in LDS when it fits
__host__ __device__ inline bool rect_place_stage(int gx, int gy) { return rect_place_lds(gx, gy, true) <= 65536; }

// The pair positions of one block of depth-ordered Gaussians (one per thread): per wave and tile the
// lanes' counts packed one byte each, per wave the lanes whose rectangle spans each tile column / row; a
// pair's position is the tile start + the block's column offset + the waves below + its rank among the
// wave's lanes. f(g, t, pos) is called per covered tile t in row-major order (k_rect_place writes the
// list, k_rect_gather sums the deterministic blend backward's per-pair slots).
template <class F>
__device__ __forceinline__ void rect_walk(int P, const uint32_t *__restrict__ order, const float2 *__restrict__ xy,
                                          const int *__restrict__ radii, int gx, int gy,
                                          const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ tile_start,
                                          int stage, uint32_t *lds, F &&f) {
    const int T = gx * gy, G = gx + gy;
    // per tile, the four waves' counts packed one byte each (a wave adds at most 64 per tile)
    const int Tp = (T + 1) & ~1;
    uint32_t *wc = lds;  // [T]
    // stage: the block's first output position per tile (tile start + this block's column offset),
    // read coalesced once instead of gathered per pair
    uint32_t *base = lds + Tp;  // [T] (stage)
    // per wave, the lanes whose rectangle spans tile column x ([x]) / tile row y ([gx + y])
    unsigned long long *span = reinterpret_cast<unsigned long long *>(lds + (stage ? 2 * Tp : Tp));  // [4][G]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t *crow = cnt + (size_t)blockIdx.x * T;
    for (int t = tid; t < T; t += 256) wc[t] = 0;
    if (stage)
        for (int t = tid; t < T; t += 256) base[t] = tile_start[t] + crow[t];
    for (int t = tid; t < 4 * G; t += 256) span[t] = 0ull;
    const int j = blockIdx.x * 256 + tid;
    // order == nullptr: index order (the per-tile sort orders each list by depth afterwards)
    const uint32_t g = j < P ? (order ? order[j] : (uint32_t)j) : 0u;
    int4 rc = make_int4(0, 0, 0, 0);
    if (j < P && !gauss_rect(g, xy, radii, gx, gy, rc)) rc = make_int4(0, 0, 0, 0);
    __syncthreads();
    unsigned long long *ws = span + w * G;
    const unsigned long long me = 1ull << lane;
    for (int x = rc.x; x < rc.z; x++) atomicOr(&ws[x], me);
    for (int y = rc.y; y < rc.w; y++) {
        atomicOr(&ws[gx + y], me);
        for (int x = rc.x; x < rc.z; x++) atomicAdd(&wc[y * gx + x], 1u << (8 * w));
    }
    __syncthreads();
    for (int y = rc.y; y < rc.w; y++) {
        const unsigned long long rows = ws[gx + y] & (me - 1ull);  // lanes below spanning row y
        for (int x = rc.x; x < rc.z; x++) {
            const int t = y * gx + x;
            const uint32_t rank = (uint32_t)__popcll(rows & ws[x]);
            // waves below: byte w-1 of the packed inclusive sums (partial sums <= 192, no carries)
            const uint32_t below = w ? ((wc[t] * 0x01010101u) >> (8 * (w - 1))) & 0xffu : 0u;
            f(g, t, (stage ? base[t] : tile_start[t] + crow[t]) + below + rank);
        }
    }
}

__global__ __launch_bounds__(256) void k_rect_place(int P, const uint32_t *__restrict__ order, const float2 *__restrict__ xy,
                                                    const int *__restrict__ radii, int gx, int gy,
                                                    const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ tile_start,
                                                    uint32_t cap, uint32_t *__restrict__ vals, int stage) {
    extern __shared__ uint32_t lds[];
    // (writing each pair's depth key beside it here, for k_tile_sort to read coalesced, made this kernel
    // 15 us slower per step at the bench size, more than the gather it saved)
    rect_walk(P, order, xy, radii, gx, gy, cnt, tile_start, stage, lds, [&](uint32_t g, int, uint32_t pos) {
        if (pos < cap) vals[pos] = g;
    });
}

// Deterministic blend backward (dgs_raster_set_deterministic): k_blend_bwd2<DEPTH, true> leaves every
// pair of the replayed lists one 12-float slot (the pair's reduced sums in the accumulator row's field
// order, zeros for a pair the tile culled or both waves skipped) instead of adding them into acc with
// float atomics. This gather walks the same rectangles as k_rect_place (in its order: Gaussian index
// with the per-tile sort, whose position map takes each walked pair to its sorted list position; depth
// order without it), one thread per Gaussian, and sums its pairs' slots in tile row-major order: a fixed
// order, so acc (and every gradient after it) is bitwise reproducible. A pair past the launched
// capacity is skipped; one past its tile's replayed prefix holds zeros: neither adds anything, exactly
// as with the atomics. Every row of acc is written (zeros for a Gaussian without a rectangle).
__global__ __launch_bounds__(256) void k_rect_gather(int P, const uint32_t *__restrict__ order, const float2 *__restrict__ xy,
                                                     const int *__restrict__ radii, int gx, int gy,
                                                     const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ tile_start,
                                                     uint32_t cap, const float4 *__restrict__ slot, float *__restrict__ acc,
                                                     int stage) {
    extern __shared__ uint32_t lds[];
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 s0 = z4, s1 = z4, s2 = z4;
    // one pair behind: a pair's slot loads are added at the next pair, so their latency overlaps the
    // walk to the next pair (same order of additions)
    float4 pa = z4, pb = z4, pc = z4;
    rect_walk(P, order, xy, radii, gx, gy, cnt, tile_start, stage, lds, [&](uint32_t, int, uint32_t pos) {
        float4 na = z4, nb = z4, nc = z4;
        if (pos < cap) {
            const float4 *q = slot + 3ull * pos;
            na = q[0];
            nb = q[1];
            nc = q[2];
        }
        s0 = s0 + pa;
        s1 = s1 + pb;
        s2 = s2 + pc;
        pa = na;
        pb = nb;
        pc = nc;
    });
    s0 = s0 + pa;
    s1 = s1 + pb;
    s2 = s2 + pc;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    // (order == nullptr: the index-order walk of the per-tile sort's placement)
    float4 *dst = reinterpret_cast<float4 *>(acc + (size_t)(order ? order[j] : (uint32_t)j) * ACC_STRIDE);
    dst[0] = s0;
    dst[1] = s1;
    dst[2] = s2;
}

// Per-tile depth sort (rect binning, the default; DGS_TILE_SORT=0 restores the global depth sort): the
// count / place kernels run over the Gaussians in index order, so every tile's list comes out in index
// order, and each list is then sorted stably by its 32-bit depth key, i.e. by (depth, index): exactly
// the order the global stable depth sort produced. The lists, and everything computed from them, are
// bit-identical. k_tile_sort: one workgroup per tile, a stable LSD radix sort of up to TS_MAX entries
// in LDS — 8-bit digits, in-wave ranking by one ballot per digit bit (as radix.hip's passes), per-wave
// digit offsets from one block scan, scatter through LDS — skipping the passes whose digit is the same
// for every key of the tile (the depth exponent byte, typically). Per entry and pass that is ~15 VALU;
// a bitonic network in registers measured 37 us per step at the bench size (~55 exchange stages of
// 64-bit keys at E = 16 per lane), one in LDS 42 us, counting ranks from LDS 66 us (O(L^2)). A list
// longer than TS_MAX is sorted as TS_MAX-long runs into scratch as (depth << 32 | index) keys, then each
// entry's position = its index in its run + its lower bound in every other run (binary search, the run
// staged in LDS).
constexpr int TS_MAX = 1024;  // (2048: no faster at the bench size, whose longest list is 591)
constexpr int TS_THR = 256;
struct TileSortLds {
    union {
        struct {
            uint32_t key[TS_MAX], val[TS_MAX];
        } kv;
        unsigned long long run[TS_MAX];  // a long list's merge: one sorted run staged
    } u;
    uint32_t cnt[4][256];  // per-wave digit counts -> per-wave output offsets
    uint16_t opos[TS_MAX];  // POS: each sorted entry's position in the index-ordered list
    uint32_t misc[8];
};

// sorts the m <= TS_MAX entries ids[0, m) (index order) stably by dkey[id]; returns the number of passes
// run (0: the order is unchanged) with the sorted (key, id) pairs in L.u.kv
// POS (the deterministic backward): L.opos carries each entry's position in the input list along
template <int NI, bool POS>
__device__ __forceinline__ int ts_block_radix(TileSortLds &L, const uint32_t *ids, int m, const uint32_t *__restrict__ dkey,
                                              int tid) {
    const int lane = tid & 63, w = tid >> 6, base = w * 64 * NI;
    const uint64_t lanes_lt = (1ull << lane) - 1ull;
    uint32_t key[NI], val[NI];
    [[maybe_unused]] uint32_t opos[NI];
    if constexpr (POS) {
#pragma unroll
        for (int r = 0; r < NI; r++) opos[r] = (uint32_t)(base + 64 * r + lane);
    }
    uint32_t kor = 0u, kand = ~0u;
#pragma unroll
    for (int r = 0; r < NI; r++) {
        const int i = base + 64 * r + lane;
        val[r] = i < m ? ids[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < NI; r++) {
        const int i = base + 64 * r + lane;
        key[r] = i < m ? dkey[val[r]] : 0u;
        if (i < m) {
            kor |= key[r];
            kand &= key[r];
        }
    }
    // the bits that differ between keys: a pass over a byte none of them has runs for nothing. Wave OR /
    // AND in DPP (row shifts, then the row broadcasts: lane 63 holds the wave's), combined across the
    // four waves in LDS (LDS atomics from every lane on one word cost 10 us per step at the bench size)
    {
        int o = (int)kor, n = (int)kand;
        o |= __builtin_amdgcn_update_dpp(0, o, 0x111, 0xf, 0xf, false);
        n &= __builtin_amdgcn_update_dpp(-1, n, 0x111, 0xf, 0xf, false);
        o |= __builtin_amdgcn_update_dpp(0, o, 0x112, 0xf, 0xf, false);
        n &= __builtin_amdgcn_update_dpp(-1, n, 0x112, 0xf, 0xf, false);
        o |= __builtin_amdgcn_update_dpp(0, o, 0x114, 0xf, 0xf, false);
        n &= __builtin_amdgcn_update_dpp(-1, n, 0x114, 0xf, 0xf, false);
        o |= __builtin_amdgcn_update_dpp(0, o, 0x118, 0xf, 0xf, false);
        n &= __builtin_amdgcn_update_dpp(-1, n, 0x118, 0xf, 0xf, false);
        o |= __builtin_amdgcn_update_dpp(0, o, 0x142, 0xa, 0xf, false);
        n &= __builtin_amdgcn_update_dpp(-1, n, 0x142, 0xa, 0xf, false);
        o |= __builtin_amdgcn_update_dpp(0, o, 0x143, 0xc, 0xf, false);
        n &= __builtin_amdgcn_update_dpp(-1, n, 0x143, 0xc, 0xf, false);
        if (lane == 63) {
            L.misc[2 * w] = (uint32_t)o;
            L.misc[2 * w + 1] = (uint32_t)n;
        }
    }
    __syncthreads();
    uint32_t kor4 = 0u, kand4 = ~0u;
#pragma unroll
    for (int ww = 0; ww < 4; ww++) {
        kor4 |= L.misc[2 * ww];
        kand4 &= L.misc[2 * ww + 1];
    }
    __syncthreads();  // misc is reused by the passes' scans
#ifdef TS_DIAG_PASSES  // diagnostic builds (tools/build_diag.sh): at most this many passes (wrong order)
    const uint32_t diff = TS_DIAG_PASSES == 0 ? 0u : (kor4 ^ kand4) & (0xffffffffu >> (32 - 8 * (TS_DIAG_PASSES + (TS_DIAG_PASSES == 0))));  // wrong order
#else
    const uint32_t diff = kor4 ^ kand4;
#endif
    int passes = 0;
    for (int shift = 0; shift < 32; shift += 8) {
        if (((diff >> shift) & 255u) == 0u) continue;  // workgroup-uniform
        passes++;
#pragma unroll
        for (int ww = 0; ww < 4; ww++) L.cnt[ww][tid] = 0;
        __syncthreads();
        uint32_t rank[NI];
#pragma unroll
        for (int r = 0; r < NI; r++) {
            const bool ok = base + 64 * r + lane < m;
            const uint32_t d = (key[r] >> shift) & 255u;
            // lanes holding the same digit: the ones where no digit bit differs from this lane's
            // (mismatch bits OR-ed per 32-lane half: one 3-input bit op per half and bit)
            const uint64_t okm = __ballot(ok);
            uint32_t xlo = ~(uint32_t)okm, xhi = ~(uint32_t)(okm >> 32);
#pragma unroll
            for (int bb = 0; bb < 8; bb++) {
                const uint64_t bal = __ballot((d >> bb) & 1u);
                const uint32_t t = (uint32_t)((int32_t)(d << (31 - bb)) >> 31);  // the bit, sign-extended
                xlo |= (uint32_t)bal ^ t;
                xhi |= (uint32_t)(bal >> 32) ^ t;
            }
            const uint64_t mk = ~(((uint64_t)xhi << 32) | xlo);
            const int leader = mk ? __ffsll((unsigned long long)mk) - 1 : 0;
            // every lane of a digit group reads the group's count before its leader advances it (the
            // wave's LDS operations complete in order): no broadcast from the leader needed
            const uint32_t b0 = ok ? L.cnt[w][d] : 0u;
            if (ok && lane == leader) L.cnt[w][d] = b0 + (uint32_t)__popcll(mk);
            rank[r] = b0 + (uint32_t)__popcll(mk & lanes_lt);
        }
        __syncthreads();
        {
            const int d = tid;  // one thread per digit: per-wave offsets, then the digit starts
            uint32_t c[4], tot = 0;
#pragma unroll
            for (int ww = 0; ww < 4; ww++) {
                c[ww] = L.cnt[ww][d];
                tot += c[ww];
            }
            // inclusive wave scan in DPP: row shifts 1/2/4/8, then the row broadcasts 15 / 31
            int x = (int)tot;
            x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);
            x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);
            x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);
            x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);
            x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
            x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
            if (lane == 63) L.misc[w] = (uint32_t)x;
            __syncthreads();
            uint32_t start = (uint32_t)x - tot;
            for (int ww = 0; ww < w; ww++) start += L.misc[ww];
#pragma unroll
            for (int ww = 0; ww < 4; ww++) {
                L.cnt[ww][d] = start;
                start += c[ww];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NI; r++) {
            if (base + 64 * r + lane < m) {
                const uint32_t dst = L.cnt[w][(key[r] >> shift) & 255u] + rank[r];
                L.u.kv.key[dst] = key[r];
                L.u.kv.val[dst] = val[r];
                if constexpr (POS) L.opos[dst] = (uint16_t)opos[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NI; r++) {
            const int i = base + 64 * r + lane;
            if (i < m) {
                key[r] = L.u.kv.key[i];
                val[r] = L.u.kv.val[i];
                if constexpr (POS) opos[r] = L.opos[i];
            }
        }
    }
    return passes;
}
template <bool POS = false>
__device__ __forceinline__ int ts_block_any(TileSortLds &L, const uint32_t *ids, int m, const uint32_t *__restrict__ dkey,
                                            int tid) {
    if (m <= 256) return ts_block_radix<1, POS>(L, ids, m, dkey, tid);
    if (m <= 512) return ts_block_radix<2, POS>(L, ids, m, dkey, tid);
    return ts_block_radix<4, POS>(L, ids, m, dkey, tid);
}

// pre (the deterministic backward, or nullptr): pre[a + p] = the position q, in the index-ordered list
// k_rect_place wrote, of the entry the sort put at position p (the backward leaves the pair's sums at
// a + q, where k_rect_gather's index-order walk finds them); vorig: scratch for the long-list path's
// copy of that list
template <bool PRE>
__global__ __launch_bounds__(TS_THR) void k_tile_sort(const uint2 *__restrict__ ranges, uint32_t cap,
                                                      const uint32_t *__restrict__ dkey, uint32_t *__restrict__ vals,
                                                      unsigned long long *__restrict__ scratch,
                                                      uint32_t *__restrict__ spos, uint32_t *__restrict__ pre,
                                                      uint32_t *__restrict__ vorig) {
    __shared__ TileSortLds L;
    const int tid = threadIdx.x;
    const uint2 rg = ranges[blockIdx.x];
    const uint32_t a = min(rg.x, cap), b = min(rg.y, cap);
    const int len = (int)(b - a);
    if (PRE && len == 1 && tid == 0) pre[a] = 0u;
    if (len <= 1) return;
    uint32_t *v = vals + a;
    if (len <= TS_MAX) {
        // every entry is read (into registers) before the first barrier; written back after the sort
        if (ts_block_any<PRE>(L, v, len, dkey, tid) == 0) {
            if constexpr (PRE)
                for (int i = tid; i < len; i += TS_THR) pre[a + i] = (uint32_t)i;
            return;
        }
        for (int i = tid; i < len; i += TS_THR) {
            v[i] = L.u.kv.val[i];
            if constexpr (PRE) pre[a + i] = L.opos[i];
        }
        return;
    }
    // a long list: TS_MAX-long runs sorted into scratch as (depth << 32 | index), then merged by rank
    unsigned long long *sc = scratch + a;
    uint32_t *ps = spos + a;
    if constexpr (PRE)  // the index-ordered list, kept for the positions (the list is overwritten below)
        for (int i = tid; i < len; i += TS_THR) vorig[a + i] = v[i];
    for (int c0 = 0; c0 < len; c0 += TS_MAX) {
        const int m = min(TS_MAX, len - c0);
        __syncthreads();  // L is reused
        if (ts_block_any(L, v + c0, m, dkey, tid) == 0) {  // all keys equal: the run is in index order
            for (int i = tid; i < m; i += TS_THR) {
                const uint32_t g = v[c0 + i];
                sc[c0 + i] = ((unsigned long long)dkey[g] << 32) | g;
            }
        } else {
            for (int i = tid; i < m; i += TS_THR) sc[c0 + i] = ((unsigned long long)L.u.kv.key[i] << 32) | L.u.kv.val[i];
        }
        for (int i = tid; i < m; i += TS_THR) ps[c0 + i] = (uint32_t)i;  // its rank in its own run
    }
    __threadfence();
    __syncthreads();
    // per run q staged in LDS: every entry of the other runs adds its lower bound in q
    for (int q0 = 0; q0 < len; q0 += TS_MAX) {
        const int mq = min(TS_MAX, len - q0);
        __syncthreads();  // the previous run's searches are done
        for (int i = tid; i < mq; i += TS_THR) L.u.run[i] = __hip_atomic_load(sc + q0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        for (int i = tid; i < len; i += TS_THR) {
            if (i >= q0 && i < q0 + mq) continue;
            const unsigned long long k = __hip_atomic_load(sc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int lo = 0, hi = mq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (L.u.run[mid] < k) lo = mid + 1;
                else hi = mid;
            }
            ps[i] += (uint32_t)lo;  // this thread's own entry
        }
    }
    // every list entry was read in the run phase: the list is overwritten in place
    for (int i = tid; i < len; i += TS_THR) {
        const uint32_t g = (uint32_t)__hip_atomic_load(sc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[ps[i]] = g;
        if constexpr (PRE) {  // g's position in the index-ordered (ascending id) list
            int lo = 0, hi = len;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (__hip_atomic_load(vorig + a + mid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < g) lo = mid + 1;
                else hi = mid;
            }
            pre[a + ps[i]] = (uint32_t)lo;
        }
    }
}

// L (the pair count) is read on the device and clipped to the launched capacity: an overflowing
// speculative launch (count > cap) then covers exactly the cap sorted pairs it wrote, never the
// padding or stale slots past them, and every range stays inside [0, cap); the host redoes the
// whole binning at the exact size afterwards.
template <class KT>
__global__ __launch_bounds__(256) void k_ranges(const uint32_t *__restrict__ count, uint32_t cap,
                                                const KT *__restrict__ keys, uint2 *__restrict__ ranges) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int L = (int)min(*count, cap);
    if (idx >= L) return;
    uint32_t t = (uint32_t)keys[idx];
    if (idx == 0) {
        ranges[t].x = 0;
    } else {
        uint32_t prev = (uint32_t)keys[idx - 1];
        if (t != prev) {
            ranges[prev].y = idx;
            ranges[t].x = idx;
        }
    }
    if (idx == L - 1) ranges[t].y = L;
}

}  // namespace dgs

// (outside the namespace: the kernel keeps the name it had next to the host code that launches it)
__global__ void k_clip_ranges(int T, uint2 *ranges, uint32_t cap) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) {
        uint2 r = ranges[t];
        ranges[t] = make_uint2(min(r.x, cap), min(r.y, cap));
    }
}
