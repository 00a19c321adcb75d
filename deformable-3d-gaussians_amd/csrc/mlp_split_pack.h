// Fused deformation MLP on split f16, weight packing (part of mlp_split.hip's translation unit): the
// packing plan, k_pack, and the pack-map and n-tile table builders.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "mlp_split_core.h"

namespace dgs {
namespace mlps {

// ------------------------------------------------------------------------------------------------
// packing plan (host)
// ------------------------------------------------------------------------------------------------
struct Img {           // one A-operand image: ntiles x nk k-slots
    int src;           // parameter index (weight)
    int transpose;     // 0: A[n][f] = W[n][f]; 1: A[n][f] = W[f][n]
    int ntiles, nk;
    int nseg_n, nseg_f;
    Seg segn[3], segf[3];
    int slot;          // first k-slot
};
struct F32Job {        // fp32 region entry: dst[r * cpad + c] = W[sr][sc] (bias: cpad = 1)
    int src;
    int rpad, cpad;
    int nseg_r, nseg_c;
    Seg segr[3], segc[3];
    int off;
};

struct Plan : Params {
    Flags F;
    std::vector<Img> imgs;
    std::vector<F32Job> f32;
    int fT1 = -1, fT2 = -1, fL[8], fHd, tHd, tL[8], tT2 = -1;  // k-slots
    int bT1 = -1, bT2 = -1, bL[8], bHd, wT1 = -1, wT2 = -1;     // fp32 offsets
    int w0te = -1, w5te = -1;                                    // fp32 t_emb columns of linear.0 / .5
    int nslots = 0, nf32 = 0;
    std::vector<int2> units;  // k_pack's workgroups: (first k-slot, k-slots) of every 16-row n-tile
    bool fits = true;         // every n-tile has at most PACK_MAXK k-slots (k_pack's register tile)
    size_t img_floats() const { return (size_t)nslots * KSLOT * 4; }  // 16-B unit = 4 floats
    size_t total() const { return img_floats() + nf32; }
};

Plan make_plan(int flags) {
    Plan P;
    P.F = make_flags(flags);
    const Flags &F = P.F;
    static_cast<Params &>(P) = make_params(F);
    auto img = [&](int src, int tr, int ntiles, int nk, int nsn, const Seg *sn, int nsf, const Seg *sf, int slot) {
        Img j{};
        j.src = src; j.transpose = tr; j.ntiles = ntiles; j.nk = nk; j.nseg_n = nsn; j.nseg_f = nsf;
        for (int q = 0; q < nsn; q++) j.segn[q] = sn[q];
        for (int q = 0; q < nsf; q++) j.segf[q] = sf[q];
        j.slot = slot;
        P.imgs.push_back(j);
    };
    auto new_img = [&](int src, int tr, int ntiles, int nk, int nsn, const Seg *sn, int nsf, const Seg *sf) {
        const int slot = P.nslots;
        img(src, tr, ntiles, nk, nsn, sn, nsf, sf, slot);
        P.nslots += ntiles * nk;
        return slot;
    };
    auto f32 = [&](int src, int rpad, int cpad, int nsr, const Seg *sr, int nsc, const Seg *sc, int off) {
        F32Job j{};
        j.src = src; j.rpad = rpad; j.cpad = cpad; j.nseg_r = nsr; j.nseg_c = nsc;
        for (int q = 0; q < nsr; q++) j.segr[q] = sr[q];
        for (int q = 0; q < nsc; q++) j.segc[q] = sc[q];
        j.off = off;
        P.f32.push_back(j);
    };
    auto new_f32 = [&](int src, int rpad, int cpad, int nsr, const Seg *sr, int nsc, const Seg *sc) {
        const int off = P.nf32;
        f32(src, rpad, cpad, nsr, sr, nsc, sc, off);
        P.nf32 += rpad * cpad;
        return off;
    };
    const Seg full = seg(0, 256, 0), one = seg(0, 1, 0);
    if (F.blender) {
        const Seg st = seg(0, F.tin, 0), s30 = seg(0, 30, 0);
        P.fT1 = new_img(P.pT0w, 0, 16, 1, 1, &full, 1, &st);   // K = TIN (13) padded to one k-step
        P.fT2 = new_img(P.pT2w, 0, 2, 8, 1, &s30, 1, &full);
        P.tT2 = new_img(P.pT2w, 1, 16, 1, 1, &full, 1, &s30);  // A[n = TH feature][f = TE feature]
        P.bT1 = new_f32(P.pT0b, 256, 1, 1, &full, 1, &one);
        P.bT2 = new_f32(P.pT2b, 32, 1, 1, &s30, 1, &one);
        P.wT1 = new_f32(P.pT0w, 256, 16, 1, &full, 1, &st);
        P.wT2 = new_f32(P.pT2w, 32, 256, 1, &s30, 1, &full);
        const Seg te0 = seg(0, 30, 63);  // linear.0 / linear.5 columns 63..92 = t_emb (layer_in_segs)
        P.w0te = new_f32(P.pLw[0], 256, 32, 1, &full, 1, &te0);
        P.w5te = new_f32(P.pLw[5], 256, 32, 1, &full, 1, &te0);
    }
    for (int i = 0; i < 8; i++) {
        Seg s[3], sf[3];
        const int ns = layer_in_segs(F, i, s);             // forward: t_emb folded with a uniform t
        const int nsf = layer_in_segs(F, i, sf, false);    // backward: the full padded input
        P.fL[i] = new_img(P.pLw[i], 0, 16, layer_kpad_f(F, i) / 32, 1, &full, ns, s);
        P.tL[i] = new_img(P.pLw[i], 1, layer_kpad(i) / 16, 8, nsf, sf, 1, &full);  // rows = padded input features
        P.bL[i] = new_f32(P.pLb[i], 256, 1, 1, &full, 1, &one);
    }
    // heads: rows stacked in output order (nout <= 13) in one 16-row image each way
    P.fHd = P.nslots;
    P.nslots += 8;   // 1 n-tile x 8 k-steps
    P.tHd = P.nslots;
    P.nslots += 16;  // 16 n-tiles x 1 k-step (K = head rows padded to 32)
    P.bHd = P.nf32;
    P.nf32 += 32;
    int r0 = 0;
    for (int h = 0; h < P.nheads; h++) {
        const Seg sr = seg(r0, P.hrows[h], 0);
        img(P.pHw[h], 0, 1, 8, 1, &sr, 1, &full, P.fHd);
        img(P.pHw[h], 1, 16, 1, 1, &full, 1, &sr, P.tHd);
        f32(P.pHb[h], 32, 1, 1, &sr, 1, &one, P.bHd);
        r0 += P.hrows[h];
    }
    P.nf32 = (P.nf32 + 3) & ~3;
    // one pack workgroup per n-tile of every image region (its scale and row statistics span the tile's
    // whole K): the region list is fixed by the flags
    auto region = [&](int slot0, int ntiles, int nk) {
        if (nk > PACK_MAXK) P.fits = false;  // pack() reports it
        for (int t = 0; t < ntiles; t++) P.units.push_back(make_int2(slot0 + t * nk, nk));
    };
    if (F.blender) {
        region(P.fT1, 16, 1);
        region(P.fT2, 2, 8);
        region(P.tT2, 16, 1);
    }
    for (int i = 0; i < 8; i++) {
        region(P.fL[i], 16, layer_kpad_f(F, i) / 32);
        region(P.tL[i], layer_kpad(i) / 16, 8);
    }
    region(P.fHd, 1, 8);
    region(P.tHd, 16, 1);
    return P;
}

// Packing is one gather + scale + split launch over map[i] = (parameter << 22) | element, or -1 for
// zero padding: i < nslots * 512 are the A-image elements in [k-slot][lane][8] order, the rest the
// fp32 region. The map depends only on the flags (built once on the host, cached on the device).
// Workgroup b < nunits packs one 16-row n-tile (its k-slots slot0 .. slot0 + nk - 1): the tile's max
// |w| sets its power-of-two scale S (scale_for), each element x is stored as hi = f16(S x) and lo =
// f16(S x - hi) in the slot's first two planes, and the third plane of the tile's first slot holds
// [1 / S, max over the tile's 16 rows of sum_k |w|] (the output-scale bounds of the forward / dX
// kernels); the other workgroups copy the fp32 region.
constexpr int PACK_MAXP = 32;
constexpr int PACK_SHIFT = 22;
struct PackPtrs {
    const float *p[PACK_MAXP];
};

__global__ __launch_bounds__(512) void k_pack(const int *__restrict__ map, PackPtrs src, const int2 *__restrict__ units,
                                              int nunits, _Float16 *__restrict__ img, float *__restrict__ fp, int nimg,
                                              int nf32) {
    __shared__ float s_rs[4][16];
    __shared__ uint32_t s_max;
    const int b = blockIdx.x, tid = threadIdx.x;
    auto gather = [&](int i) {
        const int c = map[i];
        return c < 0 ? 0.f : src.p[c >> PACK_SHIFT][c & ((1 << PACK_SHIFT) - 1)];
    };
    if (b >= nunits) {
        const int j = (b - nunits) * 512 + tid;
        if (j < nf32) fp[j] = gather(nimg + j);
        return;
    }
    const int2 u = units[b];  // (first k-slot, k-slots <= PACK_MAXK)
    if (tid == 0) s_max = 0;
    // element tid of a slot: lane l = tid >> 3 holds row l & 15 of the tile (v_mfma_f32_16x16x32_f16 A map);
    // the tile's values stay in registers between the statistics and the split: one gather each, all
    // in flight at once (the rolled loops made 2 x k-slots dependent map -> parameter round trips)
    float v[PACK_MAXK];
    float am = 0.f, rs = 0.f;
#pragma unroll
    for (int k = 0; k < PACK_MAXK; k++) {
        v[k] = k < u.y ? gather((u.x + k) * 512 + tid) : 0.f;
        am = fmaxf(am, fabsf(v[k]));
        rs += fabsf(v[k]);
    }
    rs += __shfl_xor(rs, 1);  // the 8 elements of a lane (tid bits 0-2): same row
    rs += __shfl_xor(rs, 2);
    rs += __shfl_xor(rs, 4);
    __syncthreads();
    am = wave_max(am);
    if ((tid & 63) == 0) lds_fmax(&s_max, am);
    if ((tid & 7) == 0) s_rs[tid >> 7][(tid >> 3) & 15] = rs;  // tid bits 7-8: the four k quarters
    __syncthreads();
    const Scale S = scale_for(__uint_as_float(s_max));
#pragma unroll
    for (int k = 0; k < PACK_MAXK; k++) {
        if (k >= u.y) break;
        const float x = v[k] * S.s;
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        _Float16 *d = img + (size_t)(u.x + k) * 1536 + tid;  // k-slot: hi, lo, scale plane of 512 f16
        d[0] = hi;
        d[512] = lo;
    }
    if (tid == 0) {
        float m = 0.f;
        for (int r = 0; r < 16; r++) m = fmaxf(m, (s_rs[0][r] + s_rs[1][r]) + (s_rs[2][r] + s_rs[3][r]));
        float *t = reinterpret_cast<float *>(img + (size_t)u.x * 1536 + 1024);
        t[0] = S.inv;
        t[1] = m;
    }
}

static std::vector<int> build_pack_map(const Plan &P) {
    const size_t nimg = (size_t)P.nslots * 512;
    std::vector<int> map(nimg + P.nf32, -1);
    for (const Img &j : P.imgs) {
        int r, c;
        param_shape(P.F, P, j.src, r, c);
        for (int idx = 0; idx < j.ntiles * j.nk * 512; idx++) {
            const int e = idx & 7, lane = (idx >> 3) & 63, slot = idx >> 9;
            const int k = slot % j.nk, ntile = slot / j.nk;
            const int n = ntile * 16 + (lane & 15);  // v_mfma_f32_16x16x32_f16 A map
            const int f = 32 * k + 8 * (lane >> 4) + e;
            const int sn = seg_lookup(j.segn, j.nseg_n, n);
            const int sf = seg_lookup(j.segf, j.nseg_f, f);
            if (sn >= 0 && sf >= 0)
                map[(size_t)j.slot * 512 + idx] = (j.src << PACK_SHIFT) | (j.transpose ? sf * c + sn : sn * c + sf);
        }
    }
    for (const F32Job &j : P.f32) {
        int r, c;
        param_shape(P.F, P, j.src, r, c);
        for (int rr = 0; rr < j.rpad; rr++)
            for (int cc = 0; cc < j.cpad; cc++) {
                const int sr = seg_lookup(j.segr, j.nseg_r, rr), sc = seg_lookup(j.segc, j.nseg_c, cc);
                if (sr >= 0 && sc >= 0) map[nimg + j.off + rr * j.cpad + cc] = (j.src << PACK_SHIFT) | (c ? sr * c + sc : sr);
            }
    }
    return map;
}

static std::mutex g_map_mu;
static std::map<std::pair<int, int>, int *> g_pack_maps;  // (device, flags) -> device map
static std::map<std::pair<int, int>, int2 *> g_pack_units;  // (device, flags) -> n-tile table

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

static const int2 *pack_units_for(const Plan &P, int flags) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_map_mu);
    auto it = g_pack_units.find({dev, flags});
    if (it != g_pack_units.end()) return it->second;
    int2 *d = nullptr;
    const size_t bytes = P.units.size() * sizeof(int2);
    if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
    if (hipMemcpy(d, P.units.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    g_pack_units[{dev, flags}] = d;
    return d;
}

}  // namespace mlps
}  // namespace dgs
