// Rasterizer, blend stage (device code of raster.hip's translation unit; the pipeline map is at the top of
// raster.hip). Every kernel here runs one workgroup per 16x16 tile over the tile's depth-ordered list:
//   k_blend_fwd      1 workgroup (4 waves) / 16x16 tile, LDS-staged 256-Gaussian batches, block-wide
//                    early exit; writes colour, depth, final T, last contributor
//   k_blend_img      the forward-only blend of dgs_render_frames (+ k_depth8): same staging and step
//   k_blend_bwd2     back-to-front replay from the block's max contributor, two pixels per lane; the 12
//                    per-Gaussian gradient sums reduced across the wave and added with float atomics
//                    (<.., true>, DGS_DETERMINISTIC=1: left in per-pair slots for k_rect_gather)
// The backward replays the forward's alphas bit for bit, so what the kernels share is stated once:
//   the cull (tile_reach), the alpha evaluation (conic_q, q_power, q_alpha)
//   stage_fwd<TRACK>       the forward's staging round (both forward kernels)
//   blend_step<TRACK>      the forward's per-(pixel, Gaussian) step
//   pair_alpha, pair_load, pair_grad<DEPTH>, lane_scale, row_add   the backward's pixel-pair pieces
#pragma once
#include "raster_kernels.h"

namespace dgs {

// Tile culling of a staged batch (blend fwd / bwd): a Gaussian of the tile's list whose
// alpha >= 1/255 ellipse misses every pixel centre of the tile is skipped by every pixel anyway
// (alpha < 1/255 -> `continue`), so the batch is compacted to the Gaussians that can reach the tile
// before the per-pixel loop. alpha = min(0.99, o exp(-Q/2)) with Q = c_x dx^2 + 2 c_y dx dy + c_z dy^2
// (the blend's power): a pixel can take part only if Q <= 2 ln(255 o). The minimum of the convex Q
// over the tile's pixel-centre rectangle is 0 when the centre is inside, else on an edge at the
// clamped 1-D stationary point. The bound is widened by 1 % + 1e-3 so the fp32 rounding of either
// side can never cull a contributor: images and gradients are unchanged (the list positions kept in
// n_contrib are those of the full list).
// min over the pixel-centre rectangle [x0, x1] x [y0, y1] of the conic's quadratic form <= thr
__device__ __forceinline__ bool rect_reach(float2 g, float4 co, float x0, float x1, float y0, float y1, float thr) {
    const float dxl = g.x - x1, dxh = g.x - x0;
    const float dyl = g.y - y1, dyh = g.y - y0;
    if (dxl <= 0.f && dxh >= 0.f && dyl <= 0.f && dyh >= 0.f) return true;
    auto Q = [&](float dx, float dy) { return co.x * dx * dx + 2.f * co.y * dx * dy + co.z * dy * dy; };
    float q = Q(dxl, fminf(fmaxf(-co.y * dxl / co.z, dyl), dyh));
    q = fminf(q, Q(dxh, fminf(fmaxf(-co.y * dxh / co.z, dyl), dyh)));
    q = fminf(q, Q(fminf(fmaxf(-co.y * dyl / co.x, dxl), dxh), dyl));
    q = fminf(q, Q(fminf(fmaxf(-co.y * dyh / co.x, dxl), dxh), dyh));
    return q <= thr;
}
__device__ __forceinline__ float reach_thr(float o) { return 2.f * __logf(255.f * o) * 1.01f + 1e-3f; }
__device__ __forceinline__ bool tile_reach(float2 g, float4 co, float x0, float y0) {
    if (!(co.w >= 1.f / 255.f)) return false;  // alpha <= o < 1/255 on every pixel
    return rect_reach(g, co, x0, x0 + (float)(TILE_X - 1), y0, y0 + (float)(TILE_Y - 1), reach_thr(co.w));
}
// The staged conic in exponent form: power * log2(e) = dx (q.x dx + q.y dy) + q.z dy^2 with
// q = (-0.5 a, -b, -0.5 c) log2(e) and q.w = opacity, so G = 2^p is one v_exp_f32 (no scaling
// multiply per pixel and Gaussian; 4 ops for the quadratic form). Every blend kernel evaluates
// alpha through q_power / q_alpha with the same fused operations, so the forward's and the
// backward's alphas agree bitwise (the backward's transmittance replay depends on it).
constexpr float BL_L2E = 1.4426950408889634f;
__device__ __forceinline__ float4 conic_q(float4 co) {
    return make_float4(-0.5f * BL_L2E * co.x, -BL_L2E * co.y, -0.5f * BL_L2E * co.z, co.w);
}
__device__ __forceinline__ float q_power(float4 q, float dx, float dy) {
    return fmaf(dx, fmaf(q.x, dx, q.y * dy), q.z * (dy * dy));
}
__device__ __forceinline__ float q_alpha(const float4 &q, float G) { return fminf(0.99f, q.w * G); }  // G = 2^power

// The two layouts of a 16x16 tile. One pixel per lane: TILE_PIX threads (4 waves), TILE_PIX Gaussians
// staged per round (k_blend_fwd, k_blend_img). Two pixels per lane: B2 threads (2 waves), wave w covering
// the 16x8 half (rows 8w..8w+7), lane l the pixel pair (l & 7, row) and (8 + (l & 7), row): one dy, a
// packed dx, the per-(pixel, Gaussian) arithmetic as packed fp32 (v_pk_fma_f32 / v_pk_mul_f32 /
// v_pk_add_f32); B2 Gaussians staged per round (k_blend_bwd2).
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int B2 = 128;
__device__ __forceinline__ f2 sel2(bool a, bool b, f2 x, f2 y) { return f2{a ? x.x : y.x, b ? x.y : y.y}; }

// Block-wide stable compaction slot of a kept item (tid order) over NW waves: (slot, kept count); one
// barrier, and s_wcnt holds the waves' kept counts after it
template <int NW>
__device__ __forceinline__ int2 compact_slot_n(bool keep, int tid, uint32_t *s_wcnt) {
    const unsigned long long m = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const int c = (int)s_wcnt[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    return make_int2(base + below, tot);
}

// Pixel of thread tid within its 16x16 tile: wave w takes the 8x8 quadrant (w & 1, w >> 1), not a
// 16x4 row strip, so a Gaussian covering part of the tile touches fewer waves (each (wave, Gaussian)
// pair costs the wave's whole gradient reduction in a one-pixel-per-lane backward: blend_bwd 0.336 ->
// 0.319 ms at P = 1.0 M pairs, 3 A/B pairs; forward unchanged).
__device__ __forceinline__ int2 tile_pixel(int tid) {
    const int w = tid >> 6, l = tid & 63;
    return make_int2((w & 1) * 8 + (l & 7), (w >> 1) * 8 + (l >> 3));
}

// Tile front matter: the tile's origin, this lane's pixel(s) and whether they lie inside the image, and the
// tile's list range clipped to the launched capacity (a speculative launch under capacity is redone at the
// exact size; a deferred count not resolved yet: the capacity bounds the list).
__device__ __forceinline__ uint2 tile_range(const uint2 *__restrict__ ranges, int tile, uint32_t cap) {
    const uint2 r = ranges[tile];
    return make_uint2(min(r.x, cap), min(r.y, cap));
}
struct TilePix {  // one pixel per lane
    int tx0, ty0;  // tile origin
    int2 tp;       // the pixel within the tile
    int px, py;
    bool inside;
    float pfx, pfy;
    uint2 range;
};
__device__ __forceinline__ TilePix tile_front(int tile, int tid, int gx, int W, int H, const uint2 *__restrict__ ranges,
                                              uint32_t cap) {
    TilePix t;
    t.tx0 = (tile % gx) * TILE_X;
    t.ty0 = (tile / gx) * TILE_Y;
    t.tp = tile_pixel(tid);
    t.px = t.tx0 + t.tp.x;
    t.py = t.ty0 + t.tp.y;
    t.inside = t.px < W && t.py < H;
    t.pfx = (float)t.px;
    t.pfy = (float)t.py;
    t.range = tile_range(ranges, tile, cap);
    return t;
}
struct TilePix2 {  // the pixel pair (px0, py), (px1 = px0 + 8, py) of lane `lane` of wave wv
    int tx0, ty0;
    int lx0, ly;  // the first pixel within the tile
    int px0, px1, py;
    bool in0, in1;
    f2 pfx;
    float pfy;
    uint2 range;
};
__device__ __forceinline__ TilePix2 tile_front2(int tile, int lane, int wv, int gx, int W, int H,
                                                const uint2 *__restrict__ ranges, uint32_t cap) {
    TilePix2 t;
    t.tx0 = (tile % gx) * TILE_X;
    t.ty0 = (tile / gx) * TILE_Y;
    t.lx0 = lane & 7;
    t.ly = 8 * wv + (lane >> 3);
    t.px0 = t.tx0 + t.lx0;
    t.px1 = t.px0 + 8;
    t.py = t.ty0 + t.ly;
    t.in0 = t.px0 < W && t.py < H;
    t.in1 = t.px1 < W && t.py < H;
    t.pfx = f2{(float)t.px0, (float)t.px1};
    t.pfy = (float)t.py;
    t.range = tile_range(ranges, tile, cap);
    return t;
}

// ------------------------------------------------------------------------------------------------
// The forward blend core: one staging round and one per-(pixel, Gaussian) step, shared by k_blend_fwd
// and k_blend_img. The cull, the alpha evaluation and the predicates are changed here, once; the
// kernels keep their loops, exits and bookkeeping.
// ------------------------------------------------------------------------------------------------
// Staging round r of the workgroup's TILE_PIX threads over the tile's list: positions [TILE_PIX r,
// TILE_PIX (r + 1)) are loaded, culled against the tile (tile_reach) and compacted into s_xy / s_co
// (exponent form) / s_cd, with s_pos (TRACK) each kept entry's position in the list. The batch is padded to
// a multiple of 4 with inert entries (zero conic and opacity: power 0, alpha 0, never used), so the blend
// loop tests for its early exit once per 4 Gaussians. Returns the padded count; the barrier behind the
// stores is taken.
template <bool TRACK>
__device__ __forceinline__ int stage_fwd(int r, int tid, uint2 range, float tx0, float ty0,
                                         const uint32_t *__restrict__ vals, const float2 *__restrict__ xy,
                                         const float4 *__restrict__ conic_o, const float4 *__restrict__ rgbd,
                                         float2 *s_xy, float4 *s_co, float4 *s_cd, int *s_pos, uint32_t *s_wcnt) {
    const int prog = r * TILE_PIX + tid;
    bool keep = false;
    uint32_t id = 0;
    float2 gl;
    float4 cl;
    if ((int)range.x + prog < (int)range.y) {
        id = vals[range.x + prog];
        gl = xy[id];
        cl = conic_o[id];
        keep = tile_reach(gl, cl, tx0, ty0);
    }
    const int2 sl = compact_slot_n<TILE_PIX / 64>(keep, tid, s_wcnt);
    if (keep) {
        s_xy[sl.x] = gl;
        s_co[sl.x] = conic_q(cl);
        s_cd[sl.x] = rgbd[id];
        if constexpr (TRACK) s_pos[sl.x] = prog;
    }
    const int n = sl.y, n4 = (sl.y + 3) & ~3;
    if (tid >= n && tid < n4) {
        s_xy[tid] = make_float2(0.f, 0.f);
        s_co[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        s_cd[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (TRACK) s_pos[tid] = 0;
    }
    __syncthreads();
    return n4;
}

// One pixel's blend state, and its step over staged Gaussian j (g: mean, q: exponent-form conic + opacity,
// cd: colour + depth). `done` (the pixel stopped, or lies outside the image) goes in and comes back by
// value, a plain bool of the kernel: as a member of the state, or through a reference, the compiler kept
// it as a byte in a VGPR instead of a lane mask, and k_blend_img measured 0.7 % slower. Branch-free per lane (a skipped Gaussian adds cd * 0): the skips and the stop of the
// reference's loop become predicates, so the wave runs no exec-mask bookkeeping per Gaussian; it leaves
// the batch once all of its lanes are done. Every staged word is a broadcast read that still costs the
// wave's full LDS cycles (b64 2, b128 4), so the last contributor (TRACK) is tracked as a batch index and
// mapped to its list position once per batch (12 -> 10 LDS cycles per Gaussian and wave: blend_fwd -3.5 %).
struct BlendPix {
    float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dd = 0.f;
    int lastj = 0;  // TRACK: batch index + 1 of this batch's last contributor (0: none)
};
template <bool TRACK>
__device__ __forceinline__ bool blend_step(const float2 &g, const float4 &q, const float4 &cd, float pfx, float pfy, int j,
                                           bool done, BlendPix &p) {
    const float dx = g.x - pfx, dy = g.y - pfy;
    const float power = q_power(q, dx, dy);
    const float alpha = q_alpha(q, __builtin_amdgcn_exp2f(power));
    const float testT = p.T * (1.f - alpha);
    bool use = !done && !(power > 0.f) && !(alpha < 1.f / 255.f);
    const bool stop = use && testT < 0.0001f;
    use = use && !stop;
    const float w = use ? alpha * p.T : 0.f;
    p.C0 += cd.x * w;
    p.C1 += cd.y * w;
    p.C2 += cd.z * w;
    p.Dd += cd.w * w;
    p.T = use ? testT : p.T;
    if constexpr (TRACK) p.lastj = use ? j + 1 : p.lastj;
    return done || stop;
}
// The same evaluation for a pixel pair: dx, power, G = 2^power and alpha, packed
struct PairAlpha {
    f2 dx;
    float dy;
    f2 power, G, alpha;
};
__device__ __forceinline__ PairAlpha pair_alpha(float mx, float my, const float4 &q, f2 pfx, float pfy) {
    PairAlpha a;
    a.dx = mx - pfx;
    a.dy = my - pfy;
    a.power = f2{q_power(q, a.dx.x, a.dy), q_power(q, a.dx.y, a.dy)};
    a.G = f2{__builtin_amdgcn_exp2f(a.power.x), __builtin_amdgcn_exp2f(a.power.y)};
    a.alpha = f2{q_alpha(q, a.G.x), q_alpha(q, a.G.y)};
    return a;
}

__global__ __launch_bounds__(256) void k_blend_fwd(const uint2 *__restrict__ ranges, const uint32_t *__restrict__ vals,
                                                   uint32_t cap, int W, int H, int gx, const float2 *__restrict__ xy,
                                                   const float4 *__restrict__ conic_o, const float4 *__restrict__ rgbd,
                                                   const float *bg, float *__restrict__ final_T,
                                                   uint32_t *__restrict__ n_contrib, float *__restrict__ out_color,
                                                   float *__restrict__ out_depth) {
    __shared__ float2 s_xy[TILE_PIX];
    __shared__ float4 s_co[TILE_PIX];
    __shared__ float4 s_cd[TILE_PIX];
    __shared__ int s_pos[TILE_PIX];
    __shared__ uint32_t s_wcnt[TILE_PIX / 64];
    const int tile = blockIdx.x;
    const int tid = threadIdx.x;
    const TilePix t = tile_front(tile, tid, gx, W, H, ranges, cap);
    const int rounds = div_up((int)(t.range.y - t.range.x), TILE_PIX);
    BlendPix p;
    bool done = !t.inside;
    uint32_t last = 0;
    for (int r = 0; r < rounds; r++) {
        if (__syncthreads_count(done) == TILE_PIX) break;
        const int n4 = stage_fwd<true>(r, tid, t.range, (float)t.tx0, (float)t.ty0, vals, xy, conic_o, rgbd, s_xy, s_co,
                                       s_cd, s_pos, s_wcnt);
        p.lastj = 0;
        for (int j0 = 0; j0 < n4; j0 += 4) {
            if (__ballot(!done) == 0ull) break;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u;
                const float2 g = s_xy[j];
                const float4 q = s_co[j];
                const float4 cd = s_cd[j];
                done = blend_step<true>(g, q, cd, t.pfx, t.pfy, j, done, p);
            }
        }
        if (p.lastj) last = (uint32_t)s_pos[p.lastj - 1] + 1u;  // list position + 1 (n_contrib of the full list)
    }
    if (t.inside) {
        int pid = t.py * W + t.px;
        final_T[pid] = p.T;
        n_contrib[pid] = last;
        int HW = H * W;
        out_color[pid] = p.C0 + p.T * bg[0];
        out_color[HW + pid] = p.C1 + p.T * bg[1];
        out_color[2 * HW + pid] = p.C2 + p.T * bg[2];
        out_depth[pid] = p.Dd;
    }
}

// Forward-only blend (dgs_render_frames): k_blend_fwd's staging round and per-pixel step (stage_fwd,
// blend_step, above), so T, C and depth are bitwise its values; what differs is the bookkeeping
// (TRACK = false). No last-contributor tracking (no s_pos in LDS, no per-batch map), no final_T / n_contrib, and
// the epilogue writes only what the caller asked for, from registers: float CHW colour / depth, 1 - T, the
// quantised HWC bytes and the frame's depth maximum.
//   rgb8: trunc(255 * clamp(c, 0, 1)) per channel. With pack8 (W % 4 == 0 and a 4-byte aligned frame, so
//   every tile row segment starts on a word and holds whole words) the tile's 16 x 48 bytes are assembled
//   in LDS and stored as dwords (192 per tile instead of 768 byte stores); otherwise byte stores.
//   dmax: max of the frame's depth as the float's bit pattern (depth is a sum of non-negative terms, so
//   unsigned order is float order): a wave reduction, then one atomicMax per workgroup.
__device__ __forceinline__ uint32_t to8b(float c) { return (uint32_t)(255.f * fminf(fmaxf(c, 0.f), 1.f)); }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_blend_img(const uint2 *__restrict__ ranges, const uint32_t *__restrict__ vals,
                                                   uint32_t cap, int W, int H, int gx, const float2 *__restrict__ xy,
                                                   const float4 *__restrict__ conic_o, const float4 *__restrict__ rgbd,
                                                   const float *bg, float *__restrict__ out_color,
                                                   float *__restrict__ out_depth, float *__restrict__ out_alpha,
                                                   uint8_t *__restrict__ out_rgb8, int pack8,
                                                   uint32_t *__restrict__ dmax) {
    __shared__ float2 s_xy[TILE_PIX];
    __shared__ float4 s_co[TILE_PIX];
    __shared__ float4 s_cd[TILE_PIX];
    __shared__ uint32_t s_wcnt[TILE_PIX / 64];
    __shared__ uint32_t s_px[TILE_Y * TILE_X * 3 / 4];  // the tile's HWC bytes (pack8)
    __shared__ uint32_t s_wmax[TILE_PIX / 64];
    const int tile = blockIdx.x;
    const int tid = threadIdx.x;
    const TilePix t = tile_front(tile, tid, gx, W, H, ranges, cap);
    const int rounds = div_up((int)(t.range.y - t.range.x), TILE_PIX);
    BlendPix p;
    bool done = !t.inside;
    for (int r = 0; r < rounds; r++) {
        if (__syncthreads_count(done) == TILE_PIX) break;
        const int n4 = stage_fwd<false>(r, tid, t.range, (float)t.tx0, (float)t.ty0, vals, xy, conic_o, rgbd, s_xy, s_co,
                                        s_cd, nullptr, s_wcnt);
        for (int j0 = 0; j0 < n4; j0 += 4) {
            if (__ballot(!done) == 0ull) break;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u;
                const float2 g = s_xy[j];
                const float4 q = s_co[j];
                const float4 cd = s_cd[j];
                done = blend_step<false>(g, q, cd, t.pfx, t.pfy, j, done, p);
            }
        }
    }
    const float T = p.T, Dd = p.Dd;
    const float c0 = p.C0 + T * bg[0], c1 = p.C1 + T * bg[1], c2 = p.C2 + T * bg[2];
    const int px = t.px, py = t.py;
    const bool inside = t.inside;
    if (inside) {
        const int pid = py * W + px;
        const int HW = H * W;
        if (out_color) {
            out_color[pid] = c0;
            out_color[HW + pid] = c1;
            out_color[2 * HW + pid] = c2;
        }
        if (out_depth) out_depth[pid] = Dd;
        if (out_alpha) out_alpha[pid] = 1.f - T;
    }
    if (out_rgb8) {
        if (pack8) {
            // (no barrier needed before: s_px is not touched by the blend loop)
            uint8_t *b = reinterpret_cast<uint8_t *>(s_px) + (t.tp.y * TILE_X + t.tp.x) * 3;
            b[0] = (uint8_t)to8b(c0);
            b[1] = (uint8_t)to8b(c1);
            b[2] = (uint8_t)to8b(c2);
            __syncthreads();
            // row y of the tile: nw words (3 bytes x the row's pixels inside the image, a multiple of 4)
            const int tx = t.tx0, ty = t.ty0;
            const int nw = 3 * min(TILE_X, W - tx) / 4;
            const int y = tid / 12, k = tid - 12 * y;
            if (tid < TILE_Y * 12 && ty + y < H && k < nw)
                reinterpret_cast<uint32_t *>(out_rgb8 + ((size_t)(ty + y) * W + tx) * 3)[k] = s_px[y * 12 + k];
        } else if (inside) {
            uint8_t *b = out_rgb8 + ((size_t)py * W + px) * 3;
            b[0] = (uint8_t)to8b(c0);
            b[1] = (uint8_t)to8b(c1);
            b[2] = (uint8_t)to8b(c2);
        }
    }
    if (dmax) {
        uint32_t m = inside ? __float_as_uint(Dd) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        if ((tid & 63) == 0) s_wmax[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) atomicMax(dmax, max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3])));
    }
}

// depth8 of one frame once its maximum is known (dmax: k_blend_img's word, read on the device, so the
// host never sees it): trunc(255 * clamp(depth / (max + 1e-5), 0, 1)). 4 pixels per thread, one dword
// store when pack8 (HW % 4 == 0 and an aligned frame), else bytes.
__global__ __launch_bounds__(256) void k_depth8(int HW, const float *__restrict__ depth, const uint32_t *__restrict__ dmax,
                                                uint8_t *__restrict__ out, int pack8) {
    const float den = __uint_as_float(dmax[0]) + 1e-5f;
    const int i = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= HW) return;
    if (pack8) {
        const float4 d = *reinterpret_cast<const float4 *>(depth + i);
        *reinterpret_cast<uint32_t *>(out + i) =
            to8b(d.x / den) | to8b(d.y / den) << 8 | to8b(d.z / den) << 16 | to8b(d.w / den) << 24;
        return;
    }
    for (int j = i; j < min(i + 4, HW); j++) out[j] = (uint8_t)to8b(depth[j] / den);
}

// ------------------------------------------------------------------------------------------------
// backward kernels
// ------------------------------------------------------------------------------------------------
// Reduce-scatter of the 12 per-Gaussian partial gradients over the 64 lanes (gfx950 lane swaps):
//   fold32(a, b): v_permlane32_swap pairs lane l with l+32 -> lanes 0-31 carry a, 32-63 carry b;
//   fold16(a, b): v_permlane16_swap pairs 16-lane rows 0<->1, 2<->3 -> each row carries one value;
//   row_sum15: DPP row_shr 1/2/4/8 -> the row total in the row's lane 15.
// 6 + 3 swaps and 3 x 4 DPP adds replace 12 independent 64-lane reductions (72 DPP adds + 12
// readlanes); the sums end in lanes 15/31/47/63 of three registers.
__device__ inline float fold32(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ inline float fold16(float a, float b) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ inline float row_sum15(float v) {
    int x = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true));
    x = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true));
    x = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true));
    x = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true));
    return v;
}

// ------------------------------------------------------------------------------------------------
// Blend backward, two pixels per lane (k_blend_bwd2): the pixel-pair layout, so the per-(pixel, Gaussian) arithmetic runs as packed fp32 (two pixels per
// instruction), and the per-(wave, Gaussian) gradient reduction covers 128 pixels instead of 64 (half as
// many reductions and atomics per Gaussian as with one pixel per lane, which measured 0.315-0.322 against
// 0.283 ms at P = 1.0 M pairs). Per-pixel activity becomes selects: an inactive pixel of a pair keeps its
// state and contributes zero. 128 Gaussians staged per round (6 KB of LDS: staging 256, two per thread,
// took 0.29 ms: 24 KB per workgroup capped the occupancy).
// (The same packing in the forward was slower: 0.137 vs 0.127 ms; its per-Gaussian work is too small
// to pay for half the waves per tile.)
// The shared pieces: pair_load (a pixel pair's inputs), lane_scale and row_add (the fields' constant
// factors and the add of the reduced sums), and pair_grad, the per-(pixel pair, Gaussian) gradient with
// its reduction: the one place to change a gradient term. The kernel keeps its staging, its skip test
// and where the sums go.
// ------------------------------------------------------------------------------------------------
struct PairIn {
    f2 Tfinal, dp0, dp1, dp2, ddep;  // final transmittance, dL/dcolour, dL/ddepth (DEPTH, else 0)
    f2 kbg;                          // dL/dalpha's background term / (1 - alpha)
    uint32_t last0, last1;           // n_contrib (0 outside the image: the pixel takes no Gaussian)
};
template <bool DEPTH>
__device__ __forceinline__ PairIn pair_load(const TilePix2 &t, int W, int H, const float *bg,
                                            const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib,
                                            const float *__restrict__ dL_dpix, const float *__restrict__ dL_ddepth) {
    PairIn p;
    p.Tfinal = f2{1.f, 1.f};
    p.dp0 = p.dp1 = p.dp2 = p.ddep = f2{0.f, 0.f};
    p.last0 = p.last1 = 0;
    const int HW = H * W;
    const int pid0 = t.py * W + t.px0, pid1 = t.py * W + t.px1;
    if (t.in0) {
        p.Tfinal.x = final_T[pid0];
        p.last0 = n_contrib[pid0];
        p.dp0.x = dL_dpix[pid0];
        p.dp1.x = dL_dpix[HW + pid0];
        p.dp2.x = dL_dpix[2 * HW + pid0];
        if (DEPTH) p.ddep.x = dL_ddepth[pid0];
    }
    if (t.in1) {
        p.Tfinal.y = final_T[pid1];
        p.last1 = n_contrib[pid1];
        p.dp0.y = dL_dpix[pid1];
        p.dp1.y = dL_dpix[HW + pid1];
        p.dp2.y = dL_dpix[2 * HW + pid1];
        if (DEPTH) p.ddep.y = dL_ddepth[pid1];
    }
    const float b0 = bg[0], b1 = bg[1], b2 = bg[2];
    p.kbg = -p.Tfinal * (b0 * p.dp0 + b1 * p.dp1 + b2 * p.dp2);
    return p;
}

// The reduce-scatter leaves field 4k + {0, 2, 1, 3}[row] (ACC_MX..ACC_DY order) of register k in the
// row's lane 15: the per-pixel terms are summed unscaled and each field's constant factor is applied
// once, by the lane that adds the sum.
struct LaneScale {
    float sc0, sc1, sc2;
};
__device__ __forceinline__ LaneScale lane_scale(int lane, int W, int H) {
    const float hx = 0.5f * W, hy = 0.5f * H;
    const int frow = lane >> 4;
    LaneScale s;
    s.sc0 = frow == 0 ? -hx : frow == 2 ? -hy : -0.5f;  // mean2D x, conic x, mean2D y, conic y
    s.sc1 = frow == 0 ? -0.5f : 1.f;                     // conic z, r, opacity, g
    s.sc2 = frow == 1 ? hx : frow == 3 ? hy : 1.f;       // b, |mean2D x|, depth, |mean2D y|
    return s;
}
// a row's lane 15: its three fields of the 12-float row at dst (an accumulator row, or a DET slot in LDS)
__device__ __forceinline__ void row_add(float *dst, int lane, const LaneScale &s, float w0, float w1, float w2) {
    const int row = lane >> 4;
    dst += ((row & 1) << 1) + (row >> 1);
    atomicAdd(dst, w0 * s.sc0);
    atomicAdd(dst + 4, w1 * s.sc1);
    atomicAdd(dst + 8, w2 * s.sc2);
}

// The replayed state of a pixel pair (transmittance in front of, and colour / depth behind, the current
// Gaussian) and one Gaussian's gradient terms for the pair: a = the pair's alpha evaluation (pair_alpha),
// act0 / act1 = whether each pixel takes the Gaussian, cd = its colour + depth, co = its conic + opacity.
// w0..w2 are the 12 sums reduced over the wave, unscaled (lane_scale), in the rows' lanes 15.
struct PairState {
    f2 T, acc0, acc1, acc2, accd;
};
template <bool DEPTH>
__device__ __forceinline__ void pair_grad(bool act0, bool act1, const PairAlpha &a, const float4 &cd, const float4 &co,
                                          const PairIn &in, PairState &s, float &w0, float &w1, float &w2) {
    const f2 zero = f2{0.f, 0.f};
    // an inactive pixel of the pair runs with alpha = 0 and G = 0: T (1 / (1 - 0) = 1), its
    // pending colour and every gradient term stay unchanged / zero without per-state selects
    const f2 ae = sel2(act0, act1, a.alpha, zero);
    const f2 Ge = sel2(act0, act1, a.G, zero);
    // 1 / (1 - alpha): hardware reciprocal + one Newton step (<= 1 ulp; exactly 1 at alpha = 0)
    const f2 om = 1.f - ae;
    f2 inv = f2{__builtin_amdgcn_rcpf(om.x), __builtin_amdgcn_rcpf(om.y)};
    inv = inv * (1.f - om * inv) + inv;
    s.T = s.T * inv;
    const f2 w = ae * s.T;
    // colour behind this Gaussian (acc) is updated eagerly after its use: the reference's
    // deferred last_alpha * last_color + (1 - last_alpha) * acc at the next active Gaussian
    const f2 d0 = cd.x - s.acc0, d1 = cd.y - s.acc1, d2 = cd.z - s.acc2;
    f2 dLda = d0 * in.dp0 + d1 * in.dp1 + d2 * in.dp2;
    if constexpr (DEPTH) {
        const f2 d3 = cd.w - s.accd;
        dLda = dLda + d3 * in.ddep;
        s.accd = ae * d3 + s.accd;
    }
    s.acc0 = ae * d0 + s.acc0;
    s.acc1 = ae * d1 + s.acc1;
    s.acc2 = ae * d2 + s.acc2;
    dLda = dLda * s.T + in.kbg * inv;
    // dG/dmean2D = -G (conic . d), dG/dconic = -G d d^T / 2: with u = dL/dG G the per-pixel
    // terms are co (u d) and u d d^T, their factors (-hx, -hy, -0.5) applied after the sums
    const f2 dx = a.dx;
    const float dy = a.dy;
    const f2 vop = Ge * dLda;
    const f2 u = co.w * vop;
    const f2 udx = u * dx, udy = u * dy;
    const f2 mxp = co.x * udx + co.y * udy, myp = co.y * udx + co.z * udy;
    const f2 cxp = udx * dx, cyp = udx * dy, czp = udy * dy;
    const f2 vr = w * in.dp0, vg = w * in.dp1, vb = w * in.dp2, vd = DEPTH ? w * in.ddep : zero;
    // pairs (a, b) fold to rows [a_lo, b_lo, a_hi, b_hi] of w
    w0 = row_sum15(fold16(fold32(mxp.x + mxp.y, myp.x + myp.y), fold32(cxp.x + cxp.y, cyp.x + cyp.y)));
    w1 = row_sum15(fold16(fold32(czp.x + czp.y, vop.x + vop.y), fold32(vr.x + vr.y, vg.x + vg.y)));
    w2 = row_sum15(fold16(fold32(vb.x + vb.y, vd.x + vd.y),
                          fold32(fabsf(mxp.x) + fabsf(mxp.y), fabsf(myp.x) + fabsf(myp.y))));
}

// DEPTH: the depth output has a gradient (dL_ddepth != nullptr); without one (every training step: the
// loss reads only the image) the depth terms, the depth colour-behind state and its loads drop out.
// DET: the deterministic mode (k_rect_gather): the two waves' reduced sums for a staged Gaussian meet in
// an LDS row (each field gets at most one add per wave onto zero: a + b either way round), written out
// after the batch to the pair's slot (12 floats; the staging thread writes zeros for a culled entry), and
// the tile's replayed length to tile_todo, instead of adding into acc; the pairs past the replayed
// prefix get zeros. A pair's slot is its list position when the lists were placed in depth order, else
// (the per-tile sort) the position k_rect_place gave it in index order (tile start + pre[position]):
// where k_rect_gather's walk, in k_rect_place's order, finds it
template <bool DEPTH, bool DET>
__global__ __launch_bounds__(B2) void k_blend_bwd2(const uint2 *__restrict__ ranges, const uint32_t *__restrict__ vals,
                                                   uint32_t cap, int W, int H, int gx, const float *bg,
                                                   const float2 *__restrict__ xy, const float4 *__restrict__ conic_o,
                                                   const float4 *__restrict__ rgbd, const float *__restrict__ final_T,
                                                   const uint32_t *__restrict__ n_contrib,
                                                   const float *__restrict__ dL_dpix, const float *__restrict__ dL_ddepth,
                                                   float *__restrict__ acc, float *__restrict__ slot,
                                                   uint32_t *__restrict__ tile_todo, const uint32_t *__restrict__ pre) {
    __shared__ float4 s_q[B2];   // staged conic in exponent form + opacity
    __shared__ float4 s_xyc[B2]; // mean2D x, y, list position (bits), Gaussian id (bits)
    __shared__ float4 s_co[B2];
    __shared__ float4 s_cd[B2];
    __shared__ uint32_t s_wcnt[B2 / 64];
    __shared__ uint32_t s_maxlast;
    __shared__ float4 s_slot[DET ? 3 * B2 : 1];  // DET: per staged Gaussian, its 12 gradient sums
    const int tile = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TilePix2 t = tile_front2(tile, lane, wv, gx, W, H, ranges, cap);
    const uint2 range = t.range;
    const PairIn in = pair_load<DEPTH>(t, W, H, bg, final_T, n_contrib, dL_dpix, dL_ddepth);
    if (tid == 0) s_maxlast = 0;
    __syncthreads();
    atomicMax(&s_maxlast, max(in.last0, in.last1));
    __syncthreads();
    const int todo_total = (int)s_maxlast;  // Gaussians past every pixel's last contributor are skipped
    if (DET && tid == 0) tile_todo[tile] = (uint32_t)todo_total;
    // DET: a pair's slot (pre: the per-tile sort's map back to the walk's index-order position)
    [[maybe_unused]] auto slot_of = [&](uint32_t lp) { return reinterpret_cast<float4 *>(slot + 12ull * (pre ? range.x + pre[lp] : lp)); };
    if constexpr (DET) {  // the pairs past the replayed prefix add nothing: zeros (the gather reads every pair)
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t lp = range.x + (uint32_t)todo_total + tid; lp < range.y; lp += B2) {
            float4 *z = slot_of(lp);
            z[0] = z4;
            z[1] = z4;
            z[2] = z4;
        }
    }
    const LaneScale sc = lane_scale(lane, W, H);
    const f2 zero = f2{0.f, 0.f};
    PairState st = {in.Tfinal, zero, zero, zero, zero};
    const int rounds = div_up(todo_total, B2);
    const int end = (int)range.x + todo_total;
    for (int r = 0; r < rounds; r++) {
        __syncthreads();
        const int prog = r * B2 + tid;
        bool keep = false;
        uint32_t id = 0;
        float2 gl;
        float4 cl;
        if (prog < todo_total) {
            id = vals[end - prog - 1];
            gl = xy[id];
            cl = conic_o[id];
            keep = tile_reach(gl, cl, (float)t.tx0, (float)t.ty0);
            if (DET && !keep) {
                float4 *z = slot_of((uint32_t)(end - prog - 1));
                const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                z[0] = z4;
                z[1] = z4;
                z[2] = z4;
            }
        }
        if constexpr (DET) {  // this round's rows (the previous round's were written out before the barrier)
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            s_slot[3 * tid] = z4;
            s_slot[3 * tid + 1] = z4;
            s_slot[3 * tid + 2] = z4;
        }
        const int2 sl = compact_slot_n<B2 / 64>(keep, tid, s_wcnt);
        if (keep) {
            // the position in the full list and the Gaussian's id, staged as bits beside the mean
            // (the atomic lanes used to read the id from a separate LDS array after the reduction,
            // a wait with the whole wave behind it)
            s_xyc[sl.x] = make_float4(gl.x, gl.y, __uint_as_float((uint32_t)(todo_total - 1 - prog)), __uint_as_float(id));
            s_co[sl.x] = cl;
            s_q[sl.x] = conic_q(cl);
            s_cd[sl.x] = rgbd[id];
        }
        __syncthreads();
        const int n = sl.y;
        // the next Gaussian's mean / position / id and conic are read while this one is processed:
        // the loop's first LDS reads otherwise waited out their latency at the top of every iteration
        // (blend_bwd -3.3 % at 86 VGPRs, occupancy 6 -> 5; also prefetching the colour and conic
        // read after the skip test was slower: profiles/r4zj_blend_bwd_prefetch_ab.txt, and again at
        // 96 VGPRs with the id staged here, occupancy 5 either way: profiles/r5g_blend_bwd_id_ab.txt)
        // two Gaussians per loop trip with alternating register sets: with one per trip the compiler
        // copied the prefetched mean / conic into the working registers every iteration (4 moves)
        auto gauss = [&](int j, const float4 &xc, const float4 &q) {
            const uint32_t contributor = __float_as_uint(xc.z);  // position in the full list
            const PairAlpha a = pair_alpha(xc.x, xc.y, q, t.pfx, t.pfy);
            // a pixel takes the Gaussian iff it lies within the pixel's contributors (last = 0 outside
            // the image), power <= 0 and alpha >= 1/255: the alpha gated by the first two decides, and
            // the wave's skip test is ONE compare on the larger of the pair (a ballot of a plain
            // compare is its lane mask; of a combined predicate the compiler materialises it first)
            const float ga0 = (contributor < in.last0 && a.power.x <= 0.f) ? a.alpha.x : 0.f;
            const float ga1 = (contributor < in.last1 && a.power.y <= 0.f) ? a.alpha.y : 0.f;
            if (__ballot(fmaxf(ga0, ga1) >= 1.f / 255.f) == 0ull) return;  // wave-uniform
            const bool act0 = ga0 >= 1.f / 255.f, act1 = ga1 >= 1.f / 255.f;
            const float4 cd = s_cd[j];
            const float4 co = s_co[j];
            float w0, w1, w2;
            pair_grad<DEPTH>(act0, act1, a, cd, co, in, st, w0, w1, w2);
            if ((lane & 15) == 15) {
                if constexpr (DET)
                    row_add(reinterpret_cast<float *>(s_slot + 3 * j), lane, sc, w0, w1, w2);
                else
                    row_add(acc + (size_t)__float_as_uint(xc.w) * ACC_STRIDE, lane, sc, w0, w1, w2);
            }
        };
        float4 xa = s_xyc[0], qa = s_q[0], xb, qb;
        int j = 0;
        for (; j + 1 < n; j += 2) {
            xb = s_xyc[j + 1];
            qb = s_q[j + 1];
            gauss(j, xa, qa);
            const int j2 = min(j + 2, B2 - 1);  // (the batch's last trip reads a spare slot)
            xa = s_xyc[j2];
            qa = s_q[j2];
            gauss(j + 1, xb, qb);
        }
        if (j < n) gauss(j, xa, qa);
        if constexpr (DET) {
            __syncthreads();  // both waves' adds are in
            if (tid < n) {
                float4 *dst = slot_of((uint32_t)range.x + __float_as_uint(s_xyc[tid].z));
                dst[0] = s_slot[3 * tid];
                dst[1] = s_slot[3 * tid + 1];
                dst[2] = s_slot[3 * tid + 2];
            }
        }
    }
}

}  // namespace dgs
