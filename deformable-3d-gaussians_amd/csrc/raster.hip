// Differentiable tile rasterizer for MI355X (gfx950): the host side (context pool, toggles, binning
// driver, render workspace) and the C ABI entry points dgs_raster_forward / dgs_raster_backward /
// dgs_raster_ctx_free / dgs_mark_visible. The kernels live in the headers this one translation unit
// includes, by stage: raster_preprocess.h (k_preprocess, k_preprocess_bwd, k_mark_visible), raster_bin.h
// (the tile lists: k_rect_*, k_tile_sort, sort binning), raster_blend.h (every blend kernel and the shared
// blend core), over the per-Gaussian math of raster_kernels.h.
//
// Replaces diff_gaussian_rasterization._C (un-vendored submodule, .gitmodules:4-7) behind the call
// contract of gaussian_renderer/__init__.py:53-124.
//
// Pipeline (one HIP stream, all buffers in HBM, SoA per-Gaussian geometry). The default path:
//   k_preprocess     1 thread / Gaussian: cull, Sigma3D, EWA Sigma2D, conic, radius, tile rect, SH->RGB,
//                    depth key (float bits; culled -> all-ones); zeroes the backward's accumulators
//   k_rect_count     rect binning, Gaussians in index order: per (256-Gaussian block, tile) pair counts
//   k_rect_colscan   column scan of the count matrix -> tile starts and ranges; stores the pair count into
//                    a pinned host word the host polls (speculative binning, below: no event, no copy)
//   k_rect_place     every block writes its Gaussians' ids into its slice of each tile's list
//   k_tile_sort      per-tile stable sort of the list by depth key (LDS; global scratch for long lists)
//   k_blend_fwd      1 workgroup (4 waves) / 16x16 tile, LDS-staged 256-Gaussian batches, block-wide
//                    early exit; writes colour, depth, final T, last contributor
//   k_blend_bwd2     back-to-front replay from the block's max contributor, two pixels per lane; the 12
//                    per-Gaussian gradient sums reduced across the wave and added with float atomics
//   k_preprocess_bwd 1 thread / Gaussian: conic->Sigma2D->(Sigma3D, mean), projection, SH, Sigma3D->(s,q)
// dgs_render_frames (render_raster_frame) runs the same stages up to the tile lists, forward only, and
// blends with k_blend_img (+ k_depth8).
// The other paths, by the environment variable (or dgs_debug_set_* call) that selects them:
//   DGS_BINNING=sort     sort binning, also taken past rect binning's tile / cell limits: global depth
//                        order, hipcub inclusive scan of tiles_touched in that order (pair count copied to
//                        the pinned word behind an event), k_duplicate emits (tile, id) pairs, stable radix
//                        sort on the tile bits, k_ranges
//   DGS_TILE_SORT=0      global depth order: radix sort of the Gaussians by depth key (radix.hip), then
//                        rect binning over that order and no k_tile_sort
//   DGS_DETERMINISTIC=1  k_blend_bwd2<.., true> + k_rect_gather: per-pair slots summed in a fixed order
#include <hip/hip_runtime.h>

#include <chrono>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "radix.h"
#include "raster_kernels.h"
#include "raster_preprocess.h"
#include "raster_bin.h"
#include "raster_blend.h"
#include "render.h"

// ================================================================================================
// host side: context pool and C ABI
// ================================================================================================
using namespace dgs;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) DGS_HIP_CHECK(hipFree(p));
        size_t nb = bytes + bytes / 4 + 4096;
        p = nullptr;
        DGS_HIP_CHECK(hipMalloc(&p, nb));
        cap = nb;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct dgs_raster_ctx {
    int device = 0;
    dgs_raster_settings s{};
    int P = 0, M = 0, H = 0, W = 0, gx = 0, gy = 0, num_rendered = 0;
    const float *means3D = nullptr, *shs = nullptr, *colors = nullptr, *opac = nullptr, *scales = nullptr,
                *rots = nullptr, *cov = nullptr;
    const float *shs_rest = nullptr;  // split SH rows (dgs_raster_forward_split_sh): shs = features_dc
    DevBuf geom, bin, img, acc, rect;
    // k_rect_colscan's generation-tagged tile totals: a buffer of their own, zeroed whenever it is
    // (re)allocated, so it only ever holds 0 or words a colscan launch wrote (never stale count-matrix
    // data whose upper half could equal the current generation)
    DevBuf rtot;
    // deterministic blend backward (dgs_raster_set_deterministic): [tile_todo (T, padded) | per-pair slots]
    DevBuf det;
    bool bwd_done = false;  // a backward already consumed the accumulators (a second one re-zeroes them)
    // carved views
    float2 *xy = nullptr;
    float4 *conic_o = nullptr, *rgbd = nullptr;
    uint32_t *tiles = nullptr, *offsets = nullptr;  // offsets: inclusive scan in depth order
    uint32_t *dkey = nullptr, *dkey_alt = nullptr, *gid = nullptr, *order = nullptr, *tiles_sorted = nullptr;
    uint8_t *clamped = nullptr;
    uint32_t *vals = nullptr;
    bool rect_mode = false;  // rect binning (k_rect_*) instead of duplicate + tile sort
    bool tsort = false;      // rect binning in index order + per-tile depth sort (k_tile_sort), no global depth sort
    bool det_fwd = false;    // deterministic mode at the forward: the det buffer holds the tile sort's position map
    int det_cap = 0;         // the pair capacity the det buffer was laid out for
    uint32_t *rect_cnt = nullptr, *rect_start = nullptr, *rect_total = nullptr;
    unsigned long long *rect_tot = nullptr;  // tile totals tagged with a launch generation (k_rect_colscan)
    uint2 *ranges = nullptr;
    float *final_T = nullptr;
    uint32_t *n_contrib = nullptr;
    int *radii = nullptr;
    hipEvent_t released = nullptr;
    hipStream_t last_stream = nullptr;
    bool pending_release = false;
    uint32_t *h_total = nullptr;  // pinned host word: the num_rendered read-back (no staging copy)
    uint32_t *d_total = nullptr;  // its device address (k_rect_colscan writes the count there)
    bool count_pending = false;   // deferred count: num_rendered not read yet (resolve_count)
    int spec_cap = 0;              // the speculative capacity the binning ran with
    hipEvent_t count_ev = nullptr;  // recorded after the read-back copy
};

namespace {
std::mutex g_pool_mu;
std::vector<dgs_raster_ctx *> g_pool;

size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// DGS_DETERMINISTIC=1 / dgs_raster_set_deterministic(1): the blend backward (rect binning) writes per-pair
// slots that k_rect_gather sums in a fixed order instead of float atomics into acc: bitwise reproducible
// gradients at the cost of the slot traffic (96 B per pair written and read)
Toggle g_det{[] { return env_starts("DGS_DETERMINISTIC", '1'); }};

// DGS_TILE_SORT=0 / dgs_debug_set_tile_sort(0): rect binning over the global depth sort's order (k_rect_*
// on depth-ordered Gaussians) instead of index order + the per-tile depth sort (k_tile_sort, the default)
Toggle g_tile_sort{[] { return !env_starts("DGS_TILE_SORT", '0'); }};

// DGS_BINNING=sort / dgs_debug_set_binning(1): duplicate + tile-key radix sort + ranges for every image,
// instead of rect binning up to RECT_MAX_TILES tiles and RECT_MAX_CELLS count-matrix cells (the default)
Toggle g_sort_binning{[] {
    const char *e = getenv("DGS_BINNING");
    return e && strcmp(e, "sort") == 0;
}};

// process-wide launch generations of k_rect_colscan: a tag never repeats across contexts whose
// buffers may be recycled
uint32_t next_rect_gen() {
    static std::atomic<uint32_t> g{0};
    uint32_t v = ++g;
    if (v == 0) v = ++g;
    return v;
}

bool rect_binning(int gx, int gy, int P) {
    const int T = gx * gy;
    return !g_sort_binning.get() && T <= RECT_MAX_TILES && rect_place_lds(gx, gy, false) <= 65536 &&
           (long long)div_up(P, 256) * T <= RECT_MAX_CELLS;
}

// The hipcub scan's temp-storage size (sort binning), cached per (device, size class): the size query
// costs tens of us of host time inside the num_rendered sync window. Sizes are queried for the class's
// upper end (temp storage grows monotonically with the item count).
std::mutex g_tmp_mu;
std::map<std::pair<int, int>, size_t> g_tmp_sizes;  // (device, class)

int size_class(int n) {  // 1/16-octave classes
    if (n <= 4096) return 0;
    int hb = 31 - __builtin_clz((unsigned)n);
    int frac = (int)(((unsigned long long)n << 4 >> hb) & 15);
    return hb * 16 + frac + 1;
}
int class_upper(int cls) {
    if (cls == 0) return 4096;
    int hb = (cls - 1) / 16, frac = (cls - 1) % 16;
    unsigned long long v = ((16ull + frac + 1) << hb) >> 4;
    return v > 0x7fffffffull ? 0x7fffffff : (int)v;
}

// Speculative pair capacity per device: binning is launched for this many pairs before the host
// knows num_rendered, so the CPU does not drain the GPU queue at the read-back (it waits on an
// event recorded right after the scan while duplicate/sort/blend run). A count above the capacity
// re-runs binning with a grown capacity (results are always exact).
std::mutex g_cap_mu;
std::map<int, int> g_pair_cap;
long long g_redos = 0;  // overflowing speculative launches redone at the exact size (debug counter)

int grown_cap(long long nr) {
    long long c = nr + nr / 8 + 65536;
    return (int)std::min<long long>(c, 0x7fffffffLL);
}

int pair_cap_get(int device) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    auto it = g_pair_cap.find(device);
    return it == g_pair_cap.end() ? 0 : it->second;
}

void pair_cap_observe(int device, int nr) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    int &c = g_pair_cap[device];
    const int want = grown_cap(nr);
    if (want > c || (long long)nr * 2 < c) c = want;  // grow at once; shrink when far above
}

hipError_t scan_tmp_bytes(int device, int P, hipStream_t stream, size_t &bytes) {
    const int cls = size_class(P);
    std::lock_guard<std::mutex> lk(g_tmp_mu);
    const auto key = std::make_pair(device, cls);
    auto it = g_tmp_sizes.find(key);
    if (it != g_tmp_sizes.end()) { bytes = it->second; return hipSuccess; }
    hipError_t e = hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                    class_upper(cls), stream);
    if (e == hipSuccess) g_tmp_sizes[key] = bytes;
    return e;
}

int bits_for(uint32_t n) {
    int b = 0;
    while (n) {
        b++;
        n >>= 1;
    }
    return b;
}

dgs_raster_ctx *ctx_acquire(int device, hipStream_t stream) {
    dgs_raster_ctx *c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t k = 0; k < g_pool.size(); k++) {
            if (g_pool[k]->device == device) {
                c = g_pool[k];
                g_pool.erase(g_pool.begin() + k);
                break;
            }
        }
    }
    if (!c) {
        c = new dgs_raster_ctx();
        c->device = device;
    }
    if (c->pending_release) {
        // the previous user's work on its stream precedes this one in stream order when the stream
        // is the same (the training loop): no marker at all (each costs ~6 us of GPU idle);
        // otherwise order this stream after everything queued on that stream so far
        if (c->last_stream != stream) {
            if (!c->released) (void)hipEventCreateWithFlags(&c->released, hipEventDisableTiming);
            (void)hipEventRecord(c->released, c->last_stream);
            (void)hipStreamWaitEvent(stream, c->released, 0);
        }
        c->pending_release = false;
    }
    return c;
}
}  // namespace

// The pair count of this frame on the host. Sort binning: the pinned word behind count_ev. Rect
// binning: k_rect_colscan stores the count into the coherent pinned word itself, so the host polls
// the word (no event record in the stream: one costs ~6 us of GPU idle). Only a wait longer than
// 20 ms queries the stream (then every 1024 polls), so a failed launch cannot spin forever: a query
// of a busy stream appends a completion marker at its tail, which cost ~6 us of GPU idle before the
// next launch (the optimizer's, when the native step waits for its own count at its end) on every step
// when the stream was queried every 1024 polls (profiles/r5ts_trace_summary.txt).
constexpr uint32_t COUNT_PENDING = 0xffffffffu;
std::atomic<long long> g_count_wait_ns{0}, g_count_waits{0};  // host time spent waiting for num_rendered

static int wait_count_impl(dgs_raster_ctx *c, hipStream_t stream, int &nr);
static int wait_count(dgs_raster_ctx *c, hipStream_t stream, int &nr) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = wait_count_impl(c, stream, nr);
    g_count_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    g_count_waits++;
    return rc;
}

static int wait_count_impl(dgs_raster_ctx *c, hipStream_t stream, int &nr) {
    if (!c->rect_mode) {
        DGS_HIP_CHECK(hipEventSynchronize(c->count_ev));
        nr = (int)*c->h_total;
        return DGS_OK;
    }
    volatile uint32_t *w = c->h_total;
    const auto t0 = std::chrono::steady_clock::now();
    bool slow = false;
    for (uint32_t i = 1;; i++) {
        uint32_t v = *w;
        if (v == COUNT_PENDING && (i & 1023) == 0 && !slow)
            slow = std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20);
        if (v == COUNT_PENDING && (i & 1023) == 0 && slow) {
            const hipError_t e = hipStreamQuery(stream);
            if (e == hipSuccess) {
                v = *w;
                if (v == COUNT_PENDING) {
                    set_error("dgs_raster_forward: pair count not written by k_rect_colscan");
                    return DGS_ERR_HIP;
                }
            } else if (e != hipErrorNotReady) {
                DGS_HIP_CHECK(e);
            }
        }
        if (v != COUNT_PENDING) {
            std::atomic_thread_fence(std::memory_order_acquire);
            nr = (int)v;
            return DGS_OK;
        }
        __builtin_ia32_pause();
    }
}

// Binning for `cap` pairs (>= num_rendered, or the speculative capacity) + the blend: the key
// buffer is pre-filled with all-ones (past every tile id, so the unused tail sorts last and leaves
// the stable order of the real pairs untouched), bounded duplicate in depth order, stable radix sort
// of cap items on the tile bits, ranges from the device-side count, forward blend.
template <class KT>
static int bin_tiles(dgs_raster_ctx *c, int cap, int P, hipStream_t stream, bool dbg) {
    const int T = c->gx * c->gy;
    const int end_bit = bits_for((uint32_t)T);
    size_t o_k0 = 0, o_k1 = align_up(sizeof(KT) * cap), o_v0 = align_up(o_k1 + sizeof(KT) * cap),
           o_v1 = align_up(o_v0 + 4ull * cap);
    if (int rc = c->bin.ensure(align_up(o_v1 + 4ull * cap) + 256)) return rc;
    char *b = (char *)c->bin.p;
    KT *k0 = (KT *)(b + o_k0), *k1 = (KT *)(b + o_k1);
    uint32_t *v0 = (uint32_t *)(b + o_v0), *v1 = (uint32_t *)(b + o_v1);
    {
        ScopedTimer tm("duplicate", stream);
        hipLaunchKernelGGL(k_duplicate<KT>, dim3(div_up(P, 256)), dim3(256), 0, stream, P, c->order, c->xy, c->radii,
                           c->offsets, c->gx, c->gy, k0, v0, (uint32_t)cap, c->ranges, c->gx * c->gy);
    }
    DGS_LAUNCH_CHECK("k_duplicate", dbg, stream);
    KT *ksorted = k0;
    {
        ScopedTimer tm("sort", stream);
        int alt = 0;
        if (int rc = radix::sort_pairs<KT>(k0, k1, v0, v1, cap, end_bit, stream, &alt)) return rc;
        c->vals = alt ? v1 : v0;
        ksorted = alt ? k1 : k0;
    }
    {
        ScopedTimer tm("ranges", stream);
        hipLaunchKernelGGL(k_ranges<KT>, dim3(div_up(cap, 256)), dim3(256), 0, stream, c->offsets + (P - 1),
                           (uint32_t)cap, ksorted, c->ranges);
    }
    DGS_LAUNCH_CHECK("k_ranges", dbg, stream);
    return DGS_OK;
}

// The deterministic mode's buffer for a pair capacity: [tile end (T, padded) | per-pair slots (12 floats)
// | the tile sort's position map (1 word per pair)], laid out for the capacity the forward binned with
static int det_layout(dgs_raster_ctx *c, int cap, uint32_t **tile_end, float **slot, uint32_t **pre) {
    const size_t T = (size_t)c->gx * c->gy, tpad = (T + 63) & ~(size_t)63, n = (size_t)std::max(cap, 1);
    if (int rc = c->det.ensure(4ull * tpad + 52ull * n)) return rc;
    c->det_cap = cap;
    uint32_t *te = (uint32_t *)c->det.p;
    float *sl = (float *)(te + tpad);
    if (tile_end) *tile_end = te;
    if (slot) *slot = sl;
    if (pre) *pre = (uint32_t *)(sl + 12 * n);
    return DGS_OK;
}

// The tile lists (c->ranges, c->vals) for `cap` pairs: shared by the training forward and dgs_render_frames
static int bin_lists(dgs_raster_ctx *c, int cap, int P, hipStream_t stream, bool dbg) {
    const int T = c->gx * c->gy;
    if (c->rect_mode) {
        // tile sort: the lists, then 8 + 4 (+ 4: the deterministic mode's copy) bytes of scratch per pair for
    // lists longer than k_tile_sort's LDS
        const size_t vbytes = align_up(4ull * std::max(cap, 1) + 256);
        if (int rc = c->bin.ensure(vbytes + (c->tsort ? 16ull * std::max(cap, 1) + 256 : 0))) return rc;
        c->vals = (uint32_t *)c->bin.p;
        const int nb = div_up(P, 256);
        if (cap > 0) {
            ScopedTimer tm("place", stream);
            const bool stage = rect_place_stage(c->gx, c->gy);
            hipLaunchKernelGGL(k_rect_place, dim3(nb), dim3(256), rect_place_lds(c->gx, c->gy, stage), stream, P,
                               c->tsort ? nullptr : c->order, c->xy, c->radii, c->gx, c->gy, c->rect_cnt, c->rect_start,
                               (uint32_t)cap, c->vals, (int)stage);
        }
        DGS_LAUNCH_CHECK("k_rect_place", dbg, stream);
        if (cap > 0 && c->tsort) {
            ScopedTimer tm("tile_sort", stream);
            unsigned long long *scr = (unsigned long long *)((char *)c->bin.p + vbytes);
            uint32_t *spos = (uint32_t *)(scr + std::max(cap, 1)), *vorig = spos + std::max(cap, 1);
            if (c->det_fwd) {
                uint32_t *pre = nullptr;
                if (int rc = det_layout(c, cap, nullptr, nullptr, &pre)) return rc;
                hipLaunchKernelGGL(k_tile_sort<true>, dim3(T), dim3(TS_THR), 0, stream, c->ranges, (uint32_t)cap, c->dkey,
                                   c->vals, scr, spos, pre, vorig);
            } else {
                hipLaunchKernelGGL(k_tile_sort<false>, dim3(T), dim3(TS_THR), 0, stream, c->ranges, (uint32_t)cap, c->dkey,
                                   c->vals, scr, spos, nullptr, nullptr);
            }
            DGS_LAUNCH_CHECK("k_tile_sort", dbg, stream);
        }
    } else if (cap > 0) {  // k_duplicate clears c->ranges
        // 16-bit tile keys up to 65535 tiles (4080 x 4080 pixels), 32-bit beyond
        const int rc = T < 65535 ? bin_tiles<uint16_t>(c, cap, P, stream, dbg) : bin_tiles<uint32_t>(c, cap, P, stream, dbg);
        if (rc) return rc;
    } else {
        DGS_HIP_CHECK(hipMemsetAsync(c->ranges, 0, 8ull * T, stream));
        c->vals = nullptr;
    }
    return DGS_OK;
}

static int bin_and_blend(dgs_raster_ctx *c, int cap, int P, hipStream_t stream, bool dbg, float *out_color,
                         float *out_depth) {
    if (int rc = bin_lists(c, cap, P, stream, dbg)) return rc;
    {
        ScopedTimer tm("blend_fwd", stream);
        hipLaunchKernelGGL(k_blend_fwd, dim3(c->gx * c->gy), dim3(TILE_PIX), 0, stream, c->ranges, c->vals, (uint32_t)cap,
                           c->W, c->H, c->gx, c->xy, c->conic_o, c->rgbd, c->s.bg, c->final_T, c->n_contrib, out_color,
                           out_depth);
    }
    DGS_LAUNCH_CHECK("k_blend_fwd", dbg, stream);
    return DGS_OK;
}

// Deferred pair count (dgs_raster_set_deferred_count): the forward returns without waiting for
// num_rendered; the count is read when the backward starts (the GPU is long past the scan by then)
// or when the context is freed. An overflow of the speculative capacity is then too late to redo the
// forward, so it is counted (dgs_raster_deferred_overflows) and the caller redoes the whole training
// step synchronously (deformgs/train_step.py); the backward runs on ranges clipped to the capacity
// so it stays in bounds.
std::atomic<int> g_deferred{0};
// dL/dscales: the upstream CUDA op returns the gradient w.r.t. the modified scale (scale_modifier * s),
// i.e. without the scale_modifier factor; dgs_raster_set_exact_scale_grad(1) applies the chain rule
// (identical whenever scale_modifier = 1, as in every training call)
std::atomic<int> g_exact_scale_grad{0};
std::atomic<long long> g_deferred_overflows{0};

static int resolve_count(dgs_raster_ctx *c, hipStream_t stream) {
    if (!c->count_pending) return DGS_OK;
    c->count_pending = false;
    int nr = 0;
    if (int rc = wait_count(c, stream, nr)) return rc;
    pair_cap_observe(c->device, nr);
    if (nr > c->spec_cap) {
        g_deferred_overflows++;
        const int T = c->gx * c->gy;
        hipLaunchKernelGGL(k_clip_ranges, dim3(div_up(T, 256)), dim3(256), 0, stream, T, c->ranges, (uint32_t)c->spec_cap);
        DGS_LAUNCH_CHECK("k_clip_ranges", false, stream);
        c->num_rendered = c->spec_cap;
    } else {
        c->num_rendered = nr;
    }
    return DGS_OK;
}

// ------------------------------------------------------------------------------------------------
// frame setup: the stages up to the pair count, one copy for the training forward (raster_forward) and
// dgs_render_frames (render_raster_frame)
// ------------------------------------------------------------------------------------------------
// the hipcub scan's scratch (sort binning) at the end of the geometry buffer
struct GeomScratch {
    char *p = nullptr;
    size_t scan_bytes = 0;
};

// Size and carve c->geom for P Gaussians. The slot after `offsets` holds the forward's clamped flags
// (P bytes), or with own_radii the radii (4 P bytes) of a caller that has no array of its own for them.
static int carve_geom(dgs_raster_ctx *c, int P, bool own_radii, hipStream_t stream, GeomScratch *scr) {
    size_t off_xy = 0, off_co = align_up(off_xy + 8ull * P), off_cd = align_up(off_co + 16ull * P),
           off_t = align_up(off_cd + 16ull * P), off_o = align_up(off_t + 4ull * P), off_slot = align_up(off_o + 4ull * P);
    size_t off_dk = align_up(off_slot + (own_radii ? 4ull : 1ull) * P), off_dk2 = align_up(off_dk + 4ull * P),
           off_gid = align_up(off_dk2 + 4ull * P), off_ord = align_up(off_gid + 4ull * P), off_ts = align_up(off_ord + 4ull * P);
    if (P > 0) DGS_HIP_CHECK(scan_tmp_bytes(c->device, P, stream, scr->scan_bytes));
    const size_t off_st = align_up(off_ts + 4ull * P);
    if (int rc = c->geom.ensure(off_st + scr->scan_bytes + 256)) return rc;
    char *g = (char *)c->geom.p;
    c->xy = (float2 *)(g + off_xy);
    c->conic_o = (float4 *)(g + off_co);
    c->rgbd = (float4 *)(g + off_cd);
    c->tiles = (uint32_t *)(g + off_t);
    c->offsets = (uint32_t *)(g + off_o);
    c->clamped = own_radii ? nullptr : (uint8_t *)(g + off_slot);
    if (own_radii) c->radii = (int *)(g + off_slot);
    c->dkey = (uint32_t *)(g + off_dk);
    c->dkey_alt = (uint32_t *)(g + off_dk2);
    c->gid = (uint32_t *)(g + off_gid);
    c->order = (uint32_t *)(g + off_ord);
    c->tiles_sorted = (uint32_t *)(g + off_ts);
    scr->p = g + off_st;
    return DGS_OK;
}

// The frame's binning path (c->rect_mode, c->tsort) and, for rect binning, c->rect carved into the count
// matrix [blocks][tiles], the tile starts and the pair count, plus the tile totals in c->rtot
static int carve_rect(dgs_raster_ctx *c, int P, hipStream_t stream) {
    const int T = c->gx * c->gy;
    c->rect_mode = P > 0 && rect_binning(c->gx, c->gy, P);
    c->tsort = c->rect_mode && g_tile_sort.get();
    if (!c->rect_mode) return DGS_OK;
    const size_t nb = div_up(P, 256);
    size_t o_cnt = 0, o_st = align_up(4ull * nb * T), o_n = align_up(o_st + 4ull * T);
    if (int rc = c->rect.ensure(o_n + 256)) return rc;
    char *r = (char *)c->rect.p;
    c->rect_cnt = (uint32_t *)(r + o_cnt);
    c->rect_start = (uint32_t *)(r + o_st);
    c->rect_total = (uint32_t *)(r + o_n);
    const size_t tot_cap = c->rtot.cap;
    if (int rc = c->rtot.ensure(8ull * T)) return rc;
    if (c->rtot.cap != tot_cap) DGS_HIP_CHECK(hipMemsetAsync(c->rtot.p, 0, c->rtot.cap, stream));
    c->rect_tot = (unsigned long long *)c->rtot.p;
    return DGS_OK;
}

// Without the per-tile sort: the Gaussians by depth (stable on the index) into c->order, and for sort
// binning tiles[order[j]] (the scan input) into c->tiles_sorted
static int depth_order(dgs_raster_ctx *c, int P, hipStream_t stream, bool dbg) {
    if (!c->tsort) {
        ScopedTimer tm("depth_sort", stream);
        // the last pass also gathers tiles[order[j]] into tiles_sorted
        int alt = 0;
        uint32_t *gid = c->gid, *ord = c->order;
        if (int rc = radix::sort_pairs<uint32_t>(c->dkey, c->dkey_alt, gid, ord, P, 32, stream, &alt,
                                                 c->rect_mode ? nullptr : c->tiles,
                                                 c->rect_mode ? nullptr : c->tiles_sorted))
            return rc;
        c->order = alt ? ord : gid;
    }
    DGS_LAUNCH_CHECK("depth_sort", dbg, stream);
    return DGS_OK;
}

// The frame's pair count. Rect binning: k_rect_count + k_rect_colscan, which stores it through c->d_total.
// Sort binning: the inclusive scan of tiles_sorted into c->offsets, and with `readback` its last element
// copied to c->h_total with c->count_ev recorded behind the copy.
static int count_pairs(dgs_raster_ctx *c, int P, GeomScratch &scr, bool readback, hipStream_t stream, bool dbg) {
    if (!c->rect_mode) {
        DGS_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(scr.p, scr.scan_bytes, c->tiles_sorted, c->offsets, P, stream));
        if (readback) {
            DGS_HIP_CHECK(hipMemcpyAsync(c->h_total, c->offsets + (P - 1), 4, hipMemcpyDeviceToHost, stream));
            DGS_HIP_CHECK(hipEventRecord(c->count_ev, stream));  // wait_count waits on the latest record
        }
        return DGS_OK;
    }
    const int nb = div_up(P, 256), T = c->gx * c->gy;
    {
        ScopedTimer tm("count", stream);
        hipLaunchKernelGGL(k_rect_count, dim3(nb), dim3(256), 4ull * T, stream, P, c->tsort ? nullptr : c->order, c->xy,
                           c->radii, c->gx, c->gy, c->rect_cnt, c->rect_total);
    }
    DGS_LAUNCH_CHECK("k_rect_count", dbg, stream);
    {
        ScopedTimer tm("scan", stream);
        hipLaunchKernelGGL(k_rect_colscan, dim3(div_up(T, 64)), dim3(1024), 0, stream, nb, T, c->rect_cnt, c->rect_tot,
                           next_rect_gen(), c->rect_total, c->rect_total + 1, c->rect_start, c->ranges, c->d_total);
    }
    DGS_LAUNCH_CHECK("k_rect_colscan", dbg, stream);
    return DGS_OK;
}

// Hands a context back: to the pool, its buffers kept for the next forward on the device (an acquirer on
// another stream is ordered after the stream that last used them, ctx_acquire), or freed when the pool is full
static void ctx_release(dgs_raster_ctx *c) {
    c->pending_release = true;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool.size() < 64) {
        g_pool.push_back(c);
    } else {
        c->geom.release(); c->bin.release(); c->img.release(); c->acc.release(); c->rect.release();
        c->rtot.release(); c->det.release();
        if (c->h_total) (void)hipHostFree(c->h_total);
        delete c;
    }
}

// raster_forward's failing returns give the context back (the caller never sees the pointer): whatever
// the forward enqueued before it failed is on `stream`
struct CtxGuard {
    dgs_raster_ctx *c;
    hipStream_t stream;
    ~CtxGuard() {
        if (!c) return;
        c->last_stream = stream;
        ctx_release(c);
    }
};

static int raster_forward(const dgs_raster_settings *s, int P, int M, const float *means3D, const float *shs,
                          const float *shs_rest, const float *colors_precomp, const float *opacities,
                          const float *scales, const float *rotations, const float *cov3D_precomp, float *out_color,
                          float *out_depth, int *out_radii, dgs_raster_ctx **ctx_out, int *num_rendered,
                          void *stream_, uint8_t *out_visible = nullptr) {
    hipStream_t stream = (hipStream_t)stream_;
    if (shs_rest && (M * 3 != SH_ROW || !shs || ((reinterpret_cast<uintptr_t>(shs) | reinterpret_cast<uintptr_t>(shs_rest)) & 15))) {
        set_error("dgs_raster_forward_split_sh: needs M = 16 and 16-byte aligned features_dc / features_rest");
        return DGS_ERR_ARGS;
    }
    if (!s || !ctx_out || P < 0 || !out_color || !out_depth || (P > 0 && (!means3D || !opacities || !out_radii))) {
        set_error("dgs_raster_forward: null argument");
        return DGS_ERR_ARGS;
    }
    // (an empty point set has null data pointers everywhere: nothing to validate)
    if (P > 0 && (shs == nullptr) == (colors_precomp == nullptr)) {
        set_error("Please provide exactly one of either SHs or precomputed colors!");
        return DGS_ERR_ARGS;
    }
    if (P > 0 && cov3D_precomp == nullptr && (scales == nullptr || rotations == nullptr)) {
        set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
        return DGS_ERR_ARGS;
    }
    if (P > 0 && shs && (M < 1 || M < (s->sh_degree + 1) * (s->sh_degree + 1) || s->sh_degree > 3)) {
        set_error("dgs_raster_forward: SH degree/coefficient count unsupported (degree <= 3, M >= (D+1)^2)");
        return DGS_ERR_ARGS;
    }
    if (s->image_height <= 0 || s->image_width <= 0) {
        set_error("dgs_raster_forward: empty image");
        return DGS_ERR_ARGS;
    }
    int device = 0;
    DGS_HIP_CHECK(hipGetDevice(&device));
    dgs_raster_ctx *c = ctx_acquire(device, stream);
    *ctx_out = nullptr;
    CtxGuard guard{c, stream};  // disarmed where the forward succeeds
    c->s = *s;
    c->P = P;
    c->M = M;
    c->H = s->image_height;
    c->W = s->image_width;
    c->gx = div_up(c->W, TILE_X);
    c->gy = div_up(c->H, TILE_Y);
    c->means3D = means3D; c->shs = shs; c->shs_rest = shs_rest; c->colors = colors_precomp; c->opac = opacities;
    c->scales = scales; c->rots = rotations; c->cov = cov3D_precomp;
    c->radii = out_radii;
    c->last_stream = stream;
    c->bwd_done = false;
    const int T = c->gx * c->gy;
    const int HW = c->H * c->W;
    const bool dbg = s->debug != 0;
    GeomScratch scr;
    if (int rc = carve_geom(c, P, false, stream, &scr)) return rc;
    // image state
    size_t off_r = 0, off_T = align_up(off_r + 8ull * T), off_n = align_up(off_T + 4ull * HW);
    if (int rc = c->img.ensure(off_n + 4ull * HW)) return rc;
    char *im = (char *)c->img.p;
    c->ranges = (uint2 *)(im + off_r);
    c->final_T = (float *)(im + off_T);
    c->n_contrib = (uint32_t *)(im + off_n);
    if (int rc = carve_rect(c, P, stream)) return rc;
    c->det_fwd = c->rect_mode && g_det.get();

    const float fx = c->W / (2.f * s->tanfovx), fy = c->H / (2.f * s->tanfovy);
    int nr = 0;
    // backward accumulators [P][12] (zeroed by k_preprocess)
    if (P > 0)
        if (int rc = c->acc.ensure(4ull * ACC_STRIDE * P)) return rc;
    if (P > 0) {
        {
            ScopedTimer tm("preprocess_fwd", stream);
            const bool stage = shs && M * 3 == SH_ROW && (reinterpret_cast<uintptr_t>(shs) & 15) == 0;
            hipLaunchKernelGGL(stage ? k_preprocess<true> : k_preprocess<false>, dim3(div_up(P, 256)), dim3(256), 0, stream,
                               P, s->sh_degree, M, means3D, scales,
                               s->scale_modifier, rotations, cov3D_precomp, opacities, shs, shs_rest, colors_precomp, s->viewmatrix,
                               s->projmatrix, s->campos, c->W, c->H, s->tanfovx, s->tanfovy, fx, fy, c->gx, c->gy, out_radii,
                               c->xy, c->conic_o, c->rgbd, c->tiles, c->clamped, c->dkey, c->gid, (float4 *)c->acc.p,
                               out_visible);
        }
        DGS_LAUNCH_CHECK("k_preprocess", dbg, stream);
        if (int rc = depth_order(c, P, stream, dbg)) return rc;
        if (!c->h_total) {  // coherent + mapped: k_rect_colscan stores the count into it directly
            DGS_HIP_CHECK(hipHostMalloc((void **)&c->h_total, sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));
            DGS_HIP_CHECK(hipHostGetDevicePointer((void **)&c->d_total, c->h_total, 0));
        }
        if (!c->count_ev) DGS_HIP_CHECK(hipEventCreateWithFlags(&c->count_ev, hipEventDisableTiming));
        if (c->rect_mode) *(volatile uint32_t *)c->h_total = COUNT_PENDING;  // k_rect_colscan overwrites it
        if (int rc = count_pairs(c, P, scr, true, stream, dbg)) return rc;
        int cap = pair_cap_get(device);
        const bool speculative = cap > 0 && !dbg;
        if (!speculative) {
            if (int rc = wait_count(c, stream, nr)) return rc;
            cap = nr;
        }
        if (int rc = bin_and_blend(c, cap, P, stream, dbg, out_color, out_depth)) return rc;
        if (speculative && g_deferred.load()) {  // num_rendered read by the backward (resolve_count)
            c->count_pending = true;
            c->spec_cap = cap;
            c->num_rendered = cap;
            guard.c = nullptr;
            *ctx_out = c;
            if (num_rendered) *num_rendered = -1;
            return DGS_OK;
        }
        if (speculative) {
            if (int rc = wait_count(c, stream, nr)) return rc;
            if (nr > cap) {  // overflow: redo binning + blend at the exact size
                {
                    std::lock_guard<std::mutex> lk(g_cap_mu);
                    g_redos++;
                }
                if (int rc = bin_and_blend(c, nr, P, stream, dbg, out_color, out_depth)) return rc;
            }
        }
        pair_cap_observe(device, nr);
    } else {
        if (int rc = bin_and_blend(c, 0, P, stream, dbg, out_color, out_depth)) return rc;
    }
    c->num_rendered = nr;
    guard.c = nullptr;
    *ctx_out = c;
    if (num_rendered) *num_rendered = nr;
    return DGS_OK;
}

static int raster_backward(dgs_raster_ctx *c, const float *dL_dcolor, const float *dL_ddepth, float *dL_dmeans3D,
                           float *dL_dmeans2D, float *dL_dmeans2D_densify, float *dL_dcolors, float *dL_dopacity,
                           float *dL_dcov3D, float *dL_dshs, float *dL_dshs_rest, float *dL_dscales,
                           float *dL_drotations, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (c && (c->shs_rest != nullptr) != (dL_dshs_rest != nullptr)) {
        set_error("dgs_raster_backward: split SH gradients go with a split SH forward");
        return DGS_ERR_ARGS;
    }
    if (c && dL_dshs_rest && ((reinterpret_cast<uintptr_t>(dL_dshs) | reinterpret_cast<uintptr_t>(dL_dshs_rest)) & 15)) {
        set_error("dgs_raster_backward_split_sh: SH gradients must be 16-byte aligned");
        return DGS_ERR_ARGS;
    }
    if (!c || !dL_dcolor) {
        set_error("dgs_raster_backward: null argument");
        return DGS_ERR_ARGS;
    }
    if (c->P == 0) return DGS_OK;
    if (!dL_dmeans3D || !dL_dmeans2D || !dL_dmeans2D_densify || !dL_dopacity) {
        set_error("dgs_raster_backward: null argument");
        return DGS_ERR_ARGS;
    }
    if ((c->shs && !dL_dshs) || (c->colors && !dL_dcolors) || (c->cov && !dL_dcov3D) ||
        (!c->cov && (!dL_dscales || !dL_drotations))) {
        set_error("dgs_raster_backward: missing gradient buffer for the forward's input combination");
        return DGS_ERR_ARGS;
    }
    const int P = c->P;
    c->last_stream = stream;
    if (P == 0) return DGS_OK;
    // A deferred pair count stays unresolved here (the host does not wait mid-step): the blend
    // backward clips the tile ranges to the speculative capacity the binning ran with, which is exact
    // unless it overflowed; dgs_raster_ctx_free resolves the count and counts an overflow (the
    // caller then redoes the step).
    const uint32_t cap = c->count_pending ? (uint32_t)c->spec_cap : (uint32_t)c->num_rendered;
    const bool dbg = c->s.debug != 0;
    const int T = c->gx * c->gy;
    float *acc = (float *)c->acc.p;  // [P][12], zeroed by the forward's k_preprocess
    // deterministic mode: k_rect_gather writes every row of acc (no zeroing needed)
    // deterministic: asked for at this forward too (the tile sort then left the position map)
    const bool det = g_det.get() && c->rect_mode && c->det_fwd;
    // a second backward through the same forward (retain_graph, or a context kept alive): the blend
    // backward adds into the accumulators, so they are cleared first instead of doubling the gradients
    if (c->bwd_done && !det) DGS_HIP_CHECK(hipMemsetAsync(acc, 0, 4ull * ACC_STRIDE * P, stream));
    c->bwd_done = true;
    if (cap > 0 && det) {
        uint32_t *todo = nullptr, *pre = nullptr;
        float *slot = nullptr;
        // with the tile sort, the forward laid the buffer out (its position map is in it)
        if (int rc = det_layout(c, c->tsort ? c->det_cap : (int)cap, &todo, &slot, &pre)) return rc;
        if (!c->tsort) pre = nullptr;  // lists placed in depth order: the slot index is the list position
        {
            ScopedTimer tm("blend_bwd", stream);
            hipLaunchKernelGGL((dL_ddepth ? k_blend_bwd2<true, true> : k_blend_bwd2<false, true>), dim3(T), dim3(B2), 0,
                               stream, c->ranges, c->vals, cap, c->W, c->H, c->gx, c->s.bg, c->xy, c->conic_o, c->rgbd,
                               c->final_T, c->n_contrib, dL_dcolor, dL_ddepth, acc, slot, todo, pre);
        }
        DGS_LAUNCH_CHECK("k_blend_bwd2<det>", dbg, stream);
        ScopedTimer tm("blend_gather", stream);
        const bool stage = rect_place_stage(c->gx, c->gy);
        hipLaunchKernelGGL(k_rect_gather, dim3(div_up(P, 256)), dim3(256), rect_place_lds(c->gx, c->gy, stage), stream, P,
                           c->tsort ? nullptr : c->order, c->xy, c->radii, c->gx, c->gy, c->rect_cnt, c->rect_start,
                           cap, (const float4 *)slot, acc, (int)stage);
    } else if (cap > 0) {
        ScopedTimer tm("blend_bwd", stream);
        hipLaunchKernelGGL((dL_ddepth ? k_blend_bwd2<true, false> : k_blend_bwd2<false, false>), dim3(T), dim3(B2), 0,
                           stream, c->ranges, c->vals, cap, c->W, c->H, c->gx, c->s.bg, c->xy, c->conic_o, c->rgbd,
                           c->final_T, c->n_contrib, dL_dcolor, dL_ddepth, acc, (float *)nullptr, (uint32_t *)nullptr,
                           (const uint32_t *)nullptr);
    }
    DGS_LAUNCH_CHECK("k_blend_bwd2", dbg, stream);
    const float fx = c->W / (2.f * c->s.tanfovx), fy = c->H / (2.f * c->s.tanfovy);
    {
        ScopedTimer tm("preprocess_bwd", stream);
        const bool stage = c->shs_rest || (c->shs && c->M * 3 == SH_ROW &&
                           ((reinterpret_cast<uintptr_t>(c->shs) | reinterpret_cast<uintptr_t>(dL_dshs)) & 15) == 0);
        hipLaunchKernelGGL(stage ? k_preprocess_bwd<true> : k_preprocess_bwd<false>, dim3(div_up(P, 256)), dim3(256), 0,
                           stream, P, c->s.sh_degree, c->M, c->means3D,
                           c->scales, c->s.scale_modifier, c->rots, c->cov, c->shs, c->s.viewmatrix, c->s.projmatrix,
                           c->s.campos, c->W, c->H, c->s.tanfovx, c->s.tanfovy, fx, fy, c->radii, c->clamped, acc,
                           dL_dmeans3D, dL_dmeans2D, dL_dmeans2D_densify, dL_dcolors, dL_dopacity, dL_dcov3D, dL_dshs,
                           dL_dscales, dL_drotations, c->shs_rest, dL_dshs_rest,
                           g_exact_scale_grad.load() ? c->s.scale_modifier : 1.f);
    }
    DGS_LAUNCH_CHECK("k_preprocess_bwd", dbg, stream);
    return DGS_OK;
}

extern "C" int dgs_raster_forward(const dgs_raster_settings *s, int P, int M, const float *means3D,
                                  const float *shs, const float *colors_precomp, const float *opacities,
                                  const float *scales, const float *rotations, const float *cov3D_precomp,
                                  float *out_color, float *out_depth, int *out_radii, dgs_raster_ctx **ctx_out,
                                  int *num_rendered, void *stream) {
    return raster_forward(s, P, M, means3D, shs, nullptr, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                          out_color, out_depth, out_radii, ctx_out, num_rendered, stream);
}

extern "C" int dgs_raster_forward_split_sh(const dgs_raster_settings *s, int P, const float *means3D,
                                           const float *features_dc, const float *features_rest,
                                           const float *opacities, const float *scales, const float *rotations,
                                           float *out_color, float *out_depth, int *out_radii,
                                           uint8_t *out_visible, dgs_raster_ctx **ctx_out, int *num_rendered,
                                           void *stream) {
    if (P > 0 && (!features_dc || !features_rest)) {
        set_error("dgs_raster_forward_split_sh: null SH argument");
        return DGS_ERR_ARGS;
    }
    return raster_forward(s, P, SH_ROW / 3, means3D, features_dc, P > 0 ? features_rest : nullptr, nullptr, opacities,
                          scales, rotations, nullptr, out_color, out_depth, out_radii, ctx_out, num_rendered, stream,
                          out_visible);
}

extern "C" int dgs_raster_backward(dgs_raster_ctx *c, const float *dL_dcolor, const float *dL_ddepth,
                                   float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dmeans2D_densify,
                                   float *dL_dcolors, float *dL_dopacity, float *dL_dcov3D, float *dL_dshs,
                                   float *dL_dscales, float *dL_drotations, void *stream) {
    return raster_backward(c, dL_dcolor, dL_ddepth, dL_dmeans3D, dL_dmeans2D, dL_dmeans2D_densify, dL_dcolors,
                           dL_dopacity, dL_dcov3D, dL_dshs, nullptr, dL_dscales, dL_drotations, stream);
}

extern "C" int dgs_raster_backward_split_sh(dgs_raster_ctx *c, const float *dL_dcolor, const float *dL_ddepth,
                                            float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dmeans2D_densify,
                                            float *dL_dopacity, float *dL_dfeatures_dc, float *dL_dfeatures_rest,
                                            float *dL_dscales, float *dL_drotations, void *stream) {
    if (c && c->P > 0 && (!dL_dfeatures_dc || !dL_dfeatures_rest)) {
        set_error("dgs_raster_backward_split_sh: null SH gradient");
        return DGS_ERR_ARGS;
    }
    return raster_backward(c, dL_dcolor, dL_ddepth, dL_dmeans3D, dL_dmeans2D, dL_dmeans2D_densify, nullptr,
                           dL_dopacity, nullptr, dL_dfeatures_dc, c && c->P > 0 ? dL_dfeatures_rest : nullptr,
                           dL_dscales, dL_drotations, stream);
}

extern "C" int dgs_raster_ctx_num_rendered(dgs_raster_ctx *c) {
    if (!c) return -1;
    if (resolve_count(c, c->last_stream)) return -1;
    return c->num_rendered;
}

extern "C" void dgs_raster_ctx_free(dgs_raster_ctx *c) {
    if (!c) return;
    (void)resolve_count(c, c->last_stream);  // a deferred count nobody read (forward without backward)
    ctx_release(c);
}

extern "C" void dgs_raster_set_deferred_count(int on) { g_deferred.store(on ? 1 : 0); }

extern "C" void dgs_raster_set_exact_scale_grad(int on) { g_exact_scale_grad.store(on ? 1 : 0); }

extern "C" long long dgs_raster_deferred_overflows(void) { return g_deferred_overflows.load(); }

extern "C" void dgs_debug_set_pair_cap(int device, int cap) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    g_pair_cap[device] = cap < 0 ? 0 : cap;
}

extern "C" int dgs_debug_pair_cap(int device) { return pair_cap_get(device); }

extern "C" void dgs_raster_set_deterministic(int on) { g_det.set(on); }
extern "C" void dgs_debug_set_tile_sort(int on) { g_tile_sort.set(on); }
extern "C" int dgs_debug_get_tile_sort(void) { return g_tile_sort.get() ? 1 : 0; }
extern "C" int dgs_raster_get_deterministic(void) { return g_det.get() ? 1 : 0; }

extern "C" void dgs_debug_set_binning(int mode) { g_sort_binning.set(mode == 1); }

extern "C" long long dgs_debug_count_wait_ns(long long *waits) {
    if (waits) *waits = g_count_waits.load();
    return g_count_wait_ns.load();
}

extern "C" long long dgs_debug_binning_redos(void) {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    return g_redos;
}

// ================================================================================================
// dgs_render_frames (render.hip): the forward-only rasterizer of one frame on a per-device workspace
// ================================================================================================
// The workspace reuses dgs_raster_ctx as the container of the geometry / binning buffers and their carved
// views (so bin_lists and the count wait are the training forward's own), but it never enters the
// context pool and nothing of the backward's lives in it: acc and det stay unallocated, img
// holds the tile ranges only, clamped / final_T / n_contrib are null.
namespace dgs {
struct RenderWs {
    std::mutex mu;  // held for the duration of a call
    dgs_raster_ctx c;
    DevBuf dev;                    // [depth maxima (F words) | dummy count word | depth scratch (H W floats)]
    uint32_t *h_counts = nullptr;  // mapped + coherent host array, one pair count per frame
    uint32_t *d_counts = nullptr;
    int counts_cap = 0;
    std::vector<int> caps;         // the capacity every frame was binned with
    std::vector<char> observed;    // the frame's count already went to pair_cap_observe (a synchronous first frame)
    int F = 0, last = -1;          // last: the last frame whose count goes to its host slot
    uint32_t *dmax = nullptr, *dummy = nullptr;
    float *depth_scratch = nullptr;
    bool used = false;
};
namespace {
std::mutex g_rws_mu;
std::map<int, RenderWs *> g_rws;
}  // namespace

int render_ws_acquire(int F, int H, int W, bool need_depth, hipStream_t stream, RenderWs **out) {
    int device = 0;
    DGS_HIP_CHECK(hipGetDevice(&device));
    RenderWs *ws = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_rws_mu);
        RenderWs *&slot = g_rws[device];
        if (!slot) {
            slot = new RenderWs();
            slot->c.device = device;
        }
        ws = slot;
    }
    ws->mu.lock();
    auto fail = [&](int rc) {
        ws->mu.unlock();
        return rc;
    };
    dgs_raster_ctx *c = &ws->c;
    if (ws->used && c->last_stream != stream) {  // order this stream after the previous call's work
        if (!c->released && hipEventCreateWithFlags(&c->released, hipEventDisableTiming) != hipSuccess) {
            set_error("dgs_render_frames: hipEventCreateWithFlags failed");
            return fail(DGS_ERR_HIP);
        }
        if (hipEventRecord(c->released, c->last_stream) != hipSuccess || hipStreamWaitEvent(stream, c->released, 0) != hipSuccess) {
            set_error("dgs_render_frames: could not order the stream after the workspace's previous user");
            return fail(DGS_ERR_HIP);
        }
    }
    ws->used = true;
    c->last_stream = stream;
    if (F > ws->counts_cap) {
        // (the previous array has no writer in flight: every call, a failed one included, waits for the last
        // count it enqueued before it releases the workspace, and redone frames write theirs to the
        // device-side dummy word)
        if (ws->h_counts) (void)hipHostFree(ws->h_counts);
        ws->h_counts = ws->d_counts = nullptr;
        ws->counts_cap = 0;
        const int n = F + F / 2 + 16;
        if (hipHostMalloc((void **)&ws->h_counts, 4ull * n, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void **)&ws->d_counts, ws->h_counts, 0) != hipSuccess) {
            set_error("dgs_render_frames: could not allocate the mapped pair-count array");
            return fail(DGS_ERR_OOM);
        }
        ws->counts_cap = n;
    }
    for (int f = 0; f < F; f++) ((volatile uint32_t *)ws->h_counts)[f] = COUNT_PENDING;
    ws->F = F;
    ws->last = -1;
    ws->caps.assign((size_t)F, 0);
    ws->observed.assign((size_t)F, 0);
    const size_t o_dummy = 4ull * F, o_depth = align_up(o_dummy + 4);
    if (int rc = ws->dev.ensure(o_depth + (need_depth ? 4ull * H * W : 0) + 256)) return fail(rc);
    ws->dmax = (uint32_t *)ws->dev.p;
    ws->dummy = ws->dmax + F;
    ws->depth_scratch = need_depth ? (float *)((char *)ws->dev.p + o_depth) : nullptr;
    if (hipMemsetAsync(ws->dmax, 0, 4ull * F + 4, stream) != hipSuccess) {
        set_error("dgs_render_frames: hipMemsetAsync failed");
        return fail(DGS_ERR_HIP);
    }
    if (!c->count_ev && hipEventCreateWithFlags(&c->count_ev, hipEventDisableTiming) != hipSuccess) {
        set_error("dgs_render_frames: hipEventCreateWithFlags failed");
        return fail(DGS_ERR_HIP);
    }
    *out = ws;
    return DGS_OK;
}

void render_ws_release(RenderWs *ws, hipStream_t stream) {
    ws->c.last_stream = stream;
    ws->mu.unlock();
}

int render_frame_count(const RenderWs *ws, int f) { return (int)((volatile uint32_t *)ws->h_counts)[f]; }
int render_frame_cap(const RenderWs *ws, int f) { return ws->caps[(size_t)f]; }
void render_observe_count(const RenderWs *ws, int f, int nr) {
    if (!ws->observed[(size_t)f]) pair_cap_observe(ws->c.device, nr);
}

int render_wait_counts(RenderWs *ws, hipStream_t stream) {
    if (ws->last < 0) return DGS_OK;  // no frame wrote a count (P = 0)
    dgs_raster_ctx *c = &ws->c;
    c->h_total = ws->h_counts + ws->last;  // counts arrive in stream order: the last one is the latest
    int nr = 0;
    return wait_count(c, stream, nr);
}

int render_raster_frame(RenderWs *ws, const RenderRasterIn &in, int f, int known_count, hipStream_t stream) {
    dgs_raster_ctx *c = &ws->c;
    const int P = in.P, device = c->device;
    c->P = P;
    c->M = SH_ROW / 3;
    c->H = in.H;
    c->W = in.W;
    c->gx = div_up(c->W, TILE_X);
    c->gy = div_up(c->H, TILE_Y);
    c->s.bg = in.bg;
    const int T = c->gx * c->gy, HW = c->H * c->W;
    const bool redo = known_count >= 0;
    GeomScratch scr;
    if (int rc = carve_geom(c, P, true, stream, &scr)) return rc;  // the radii in place of the clamped bytes
    if (int rc = c->img.ensure(8ull * T)) return rc;  // the tile ranges only
    c->ranges = (uint2 *)c->img.p;
    c->final_T = nullptr;
    c->n_contrib = nullptr;
    if (int rc = carve_rect(c, P, stream)) return rc;
    c->det_fwd = false;
    if (redo && in.depth8) DGS_HIP_CHECK(hipMemsetAsync(ws->dmax + f, 0, 4, stream));
    int cap = 0;
    if (P > 0) {
        const float fx = c->W / (2.f * in.tanfovx), fy = c->H / (2.f * in.tanfovy);
        {
            ScopedTimer tm("preprocess_img", stream);
            hipLaunchKernelGGL((k_preprocess<true, true>), dim3(div_up(P, 256)), dim3(256), 0, stream, P, in.sh_degree,
                               SH_ROW / 3, in.means3D, in.scales, in.scale_modifier, in.rotations, (const float *)nullptr,
                               in.opacities, in.f_dc, in.f_rest, (const float *)nullptr, in.viewmatrix, in.projmatrix,
                               in.campos, c->W, c->H, in.tanfovx, in.tanfovy, fx, fy, c->gx, c->gy, c->radii, c->xy,
                               c->conic_o, c->rgbd, c->tiles, (uint8_t *)nullptr, c->dkey, c->gid, (float4 *)nullptr,
                               (uint8_t *)nullptr);
        }
        DGS_LAUNCH_CHECK("k_preprocess", false, stream);
        if (int rc = depth_order(c, P, stream, false)) return rc;
        // the frame's pair count: its own host word (a redo already knows it: the device-side dummy word)
        c->h_total = ws->h_counts + f;
        c->d_total = redo ? ws->dummy : ws->d_counts + f;
        if (int rc = count_pairs(c, P, scr, !redo, stream, false)) return rc;
        if (!redo) ws->last = f;
        cap = redo ? known_count : pair_cap_get(device);
        if (!redo && cap <= 0) {  // no learned capacity: this frame waits for its own count, as the forward does
            int nr = 0;
            if (int rc = wait_count(c, stream, nr)) return rc;
            cap = nr;
            pair_cap_observe(device, nr);
            ws->observed[(size_t)f] = 1;
        }
    }
    ws->caps[(size_t)f] = cap;
    if (int rc = bin_lists(c, cap, P, stream, false)) return rc;
    const bool want8 = in.depth8 != nullptr;
    float *depth = in.depth ? in.depth : (want8 ? ws->depth_scratch : nullptr);
    const int pack_rgb = in.rgb8 && c->W % 4 == 0 && (reinterpret_cast<uintptr_t>(in.rgb8) & 3) == 0;
    {
        ScopedTimer tm("blend_img", stream);
        hipLaunchKernelGGL(k_blend_img, dim3(T), dim3(TILE_PIX), 0, stream, c->ranges, c->vals, (uint32_t)cap, c->W, c->H,
                           c->gx, c->xy, c->conic_o, c->rgbd, in.bg, in.color, depth, in.alpha, in.rgb8, pack_rgb,
                           want8 ? ws->dmax + f : (uint32_t *)nullptr);
    }
    DGS_LAUNCH_CHECK("k_blend_img", false, stream);
    if (want8) {
        const int pack_d = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(depth) & 15) == 0 &&
                           (reinterpret_cast<uintptr_t>(in.depth8) & 3) == 0;
        ScopedTimer tm("depth8", stream);
        hipLaunchKernelGGL(k_depth8, dim3(div_up(div_up(HW, 4), 256)), dim3(256), 0, stream, HW, depth, ws->dmax + f,
                           in.depth8, pack_d);
        DGS_LAUNCH_CHECK("k_depth8", false, stream);
    }
    return DGS_OK;
}
}  // namespace dgs

extern "C" int dgs_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                                uint8_t *visible, void *stream_) {
    (void)projmatrix;
    if (P <= 0) return DGS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_mark_visible, dim3(div_up(P, 256)), dim3(256), 0, stream, P, means3D, viewmatrix, visible);
    DGS_LAUNCH_CHECK("k_mark_visible", false, stream);
    return DGS_OK;
}
