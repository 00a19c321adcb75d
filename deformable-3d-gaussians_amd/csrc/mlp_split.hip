// Fused deformation MLP (positional encoding + timenet + 8x256 trunk with skip + heads) on f16 MFMA
// with a scaled two-piece operand split: the default path of dgs_deform_* (the fp32-MFMA kernels of
// mlp.hip / mlp_fp32_*.h run instead under DGS_MLP_EXACT_FP32).
//
// Replaces DeformNetworkBaseline.forward and its autograd backward (utils/time_utils.py:56-127;
// DeformNetwork :129-201 via DGS_MLP_NO_ROTSCALE; 6-DoF heads :114-121 emitted raw, exp_se3 stays in
// the host glue).
//
// Numerics ("f16x3", round 6; rounds 1-5 ran a three-piece bf16 split with six products per fp32
// product). Every fp32 operand x is multiplied by a power of two S (exact) that puts its group's
// magnitude bound into [2^14, 2^15), then split into two f16 values
//   hi = f16(S x), lo = f16(S x - hi)                           (round to nearest)
// (S x - hi is exact in fp32; |S x - hi| <= 2^-11 |hi|, so lo carries the next 11 bits: S x = hi + lo
// to 2^-22 relative; below the f16 normal range the pieces keep 2^-25 absolute, i.e. 2^-39 of the
// group's bound). A product a*b is accumulated as the three f16 x f16 products hh + hl + lh, each
// exact in the fp32 accumulator of the MFMA (hl, lh <= 2^-11 |hh|; the dropped ll <= 2^-22 |ab|),
// hh in the running accumulator and hl + lh in their own (an MFMA aligns its terms and C to the
// largest within a limited window, tools/mfma_round_probe.hip), added once per GEMM. The scales are
// undone in fp32 (powers of two: exact) in the epilogue. F16 MFMA forms run at the bf16 rate
// (MI355X_MICROARCH: 'the F16 forms take the same cycles'), so the GEMMs issue half the MFMAs of the
// bf16x6 split (16/3 = 5.3x the fp32-MFMA rate), read two operand planes instead of three, and split
// in 5 VALU per two values instead of 11. Accuracy: tests/test_gpu_mlp.py holds every output and
// parameter gradient to 2x the exact-fp32 path's error against float64, including the bench step's
// own near-cancelling upstream gradient at 100k points (test_split_accuracy_bench_regime).
//   Scales. A (weights): one per (image, 16-row n-tile) over the whole K, from the tile's max |w|
// (k_pack, written into every k-slot of the tile). B (activations / dZ in LDS): one per layer, the
// same on every wave without any synchronisation: the writers of layer L's output all evaluate the
// bound  max_rows sum_k |W_L[row, k]| * max|input of L| + max|b_L|  (>= every output; the row abs
// sums are per-image statistics k_pack computes, the input maximum is the maximum of the ACTUAL
// maxima the previous layer's writers published in LDS before their hand-off signal, so the bound is
// loose by ~sqrt(K) at most, never compounding over layers). Inputs staged from memory (x_emb, t
// encodings, dOut) and the narrow per-point timenet outputs take their block's actual maximum behind
// the workgroup barrier their staging already has. A GEMM whose K spans two scale groups (x_emb |
// h of linear.5, x_emb | t_emb of linear.0) rescales its accumulators once at the boundary.
//
// Layout ("transposed" formulation, Y^T = W X^T: features on MFMA rows, points on MFMA columns),
// v_mfma_f32_16x16x32_f16:
//  * One workgroup = 64 points x 16 waves (4 per SIMD); wave r owns output rows 16r..16r+15 of every
//    256-wide layer for all four 16-point column tiles, so each 2 KiB weight fragment (16 rows x 32
//    features x 2 splits) fetched from L2 feeds 4 x 3 MFMAs. The training forward / dX chain run as
//    8 waves of two n-tiles (k_fwd8 / k_bwd8).
//  * Activations live in LDS split into hi/lo f16 images of 16-byte units (8 features x 1 point),
//    [8-feature group][split][64 points]: the B operand of a k-step (32 features) is one ds_read_b128
//    per split and column tile, and an accumulator's 4 rows are one 8-byte store per split into the
//    next layer's image. XE | TE | H groups are contiguous, so cat(x_emb, t_emb) and cat(x_emb, t_emb,
//    h) are plain group ranges.
//  * Narrow layers (timenet.2, heads, the t_emb rows of the backward) run as full-K 16x16 tiles on a
//    subset of the waves: no partial sums.
//  * Weights are packed every call (they change every optimizer step) by one gather + scale + split
//    launch into A-fragment images [n-tile][k-step][split][64 lanes][8 f16] (k-slot stride 3 KiB: hi,
//    lo, and the tile's inverse scale).
//  * Saved activations / dZ stay fp32 feature-major [rows][Ns] (mlp_shared.h row map; the dW GEMM
//    reads them), written in each layer's epilogue; relu' masks are one u16 per lane and 16-row
//    tile ([64-point block][row / 16][64 lanes]). Every reduction has a fixed order: bitwise
//    deterministic.
#include <hip/hip_runtime.h>

#include <atomic>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "dgs_common.h"
#include "mlp_shared.h"
#include "mlp_split_core.h"
#include "mlp_split_fwd.h"
#include "mlp_split_bwd.h"
#include "mlp_split_dw.h"
#include "mlp_split_pack.h"
#include "mlp_active.h"

namespace dgs {
namespace mlps {

// dW split plan: one 8-wave workgroup per CU (LDS 144 KiB); per-chunk cost in MFMA tiles + staging
// k_dws per-chunk cost by job shape (dw_shape: COL 256x256, COL 32-row head, ROW 96-col, ROW 16-col,
// ROW 64-col),
// relative to the full tile, from the per-workgroup durations of tools/mlp_clock.py at 100k points
// (profiles/r3p_mlp_clock_before.json: a full-tile chunk 4.5 us, a 96-col chunk 2.6 us, a head chunk
// 1.5 us; the MFMA-tile model gave the narrow jobs too few workgroups, which then finished 25 % after
// the rest. With these costs every job's workgroups end within 4 %: profiles/r3p_mlp_clock.json)
// (the folded t_emb's 64-column ROW shape: 1.89 us per chunk vs 4.64 for a full tile, the head 1.59:
// profiles/r3s_mlp_clock_fold.json)
static const double kDwsShapeCost[5] = {1.0, 0.34, 0.58, 0.30, 0.41};
// target: workgroups of the plan (256, one per CU; the slab scratch is sized for it; fewer with
// reserved CUs)
static WPlan split_wplan(const Flags &F, int target = 256) {
    static const bool model = env_starts("DGS_DWS_TILE_MODEL", '1');  // A/B only: the MFMA-tile cost model
    return make_wplan(F, target, 1.5, 4.0, model ? nullptr : kDwsShapeCost);
}


static size_t padded_points(int N) { return (size_t)div_up(N, BM) * BM; }

static int cu_count() {
    static std::mutex mu;
    static std::map<int, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cache[dev] = v;
    return v;
}
// CUs the MLP kernels leave free for concurrent work (the data-parallel step's gradient all-reduce runs
// on its own stream under the network backward): the persistent k_fwd / k_bwd grids
// launch cu_count() - reserve workgroups (one per CU) and k_dws's plan spans 256 - reserve workgroups.
// dgs_mlp_set_reserved_cus / DGS_MLP_RESERVE_CUS; default 0.
static std::atomic<int> g_reserve_cus{-1};
static int reserved_cus() {
    int v = g_reserve_cus.load();
    if (v < 0) {
        const char *e = getenv("DGS_MLP_RESERVE_CUS");
        int want = e ? atoi(e) : 0;
        want = want < 0 ? 0 : want > 64 ? 64 : want;
        g_reserve_cus.compare_exchange_strong(v, want);
        v = g_reserve_cus.load();
    }
    return v;
}
static int mlp_cus() { return std::max(1, cu_count() - reserved_cus()); }
// the CUs split_blocks spreads a sparse last round over (0: DGS_MLP_NO_TAIL=1 keeps 64-point blocks)
static int tail_cus() {
    static const bool off = env_starts("DGS_MLP_NO_TAIL", '1');
    return off ? 0 : mlp_cus();
}
static Blocks block_split(int N) { return split_blocks(N, tail_cus()); }
// Block-queue counters of the persistent k_fwd / k_bwd, one zeroed pair per (device, stream, kernel)
// (two launches in flight on two streams must not share one). DGS_MLP_STATIC=1: one launch block per
// block, no queue (A/B).
static uint32_t *block_queue(hipStream_t stream, int kernel) {
    static const bool off = env_starts("DGS_MLP_STATIC", '1');
    if (off) return nullptr;
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, uint32_t *> words;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    uint32_t *&w = words[{dev, stream}];
    if (!w) {
        if (hipMalloc(&w, 4 * sizeof(uint32_t)) != hipSuccess) {
            w = nullptr;
            return nullptr;
        }
        if (hipMemset(w, 0, 4 * sizeof(uint32_t)) != hipSuccess) return nullptr;
    }
    return w + 2 * kernel;
}
// k_timenet's output for a forward without saved activations (inference with a uniform t), one
// TC_FLOATS buffer per (device, stream)
static float *timenet_scratch(hipStream_t stream) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, float *> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    float *&b = bufs[{dev, stream}];
    if (!b && hipMalloc(&b, TC_FLOATS * sizeof(float)) != hipSuccess) b = nullptr;
    return b;
}
static int persistent_grid(int nblk, const uint32_t *queue) { return queue ? std::min(nblk, mlp_cus()) : nblk; }

static size_t mask_words(const Flags &F, size_t Ns) {
    const size_t nb = Ns / BM;
    return (size_t)F.nmask * 2 * (nb + 3 * std::min<size_t>(nb, TAIL_MAX_LAST));
}

size_t saved_floats(int flags, int N) {
    const Flags F = make_flags(flags);
    const size_t Ns = padded_points(N);
    return (size_t)F.nsaved * Ns + mask_words(F, Ns) + TC_FLOATS;
}

// dW arithmetic (DGS_MLP_SPLIT_DW): 3 (default) = the split-f16 k_dws (private / shared operands, every
// value split once), 0 = the fp32-input MFMA k_dw (mlp_dw_fp32.h, via mlp::dw_fp32), both on the same [rows][Ns] arrays (the
// bf16 k_dw / k_dwg variants, modes 1 and 2, were removed with the bf16x6 arithmetic in round 6)
static int dw_mode() {
    static const int m = env_starts("DGS_MLP_SPLIT_DW", '0') ? 0 : 3;
    return m;
}
size_t scratch_floats(int flags, int N) {
    const Flags F = make_flags(flags);
    const size_t slabs = std::max((size_t)split_wplan(F).nblocks * SLAB, mlp::dw_fp32_slab_floats(flags));
    return (size_t)F.nz * padded_points(N) + slabs;
}

int pack(int flags, const float *const *params, float *packed, hipStream_t stream) {
    const Plan P = make_plan(flags);
    if (!P.fits) {
        set_error("dgs_deform_pack: an A-image n-tile exceeds PACK_MAXK k-slots");
        return DGS_ERR_ARGS;
    }
    if (P.nparams > PACK_MAXP) {
        set_error("dgs_deform_pack: too many parameters");
        return DGS_ERR_ARGS;
    }
    PackPtrs src{};
    for (int k = 0; k < P.nparams; k++) {
        if (!params[k]) {
            set_error("dgs_deform_pack: null parameter pointer");
            return DGS_ERR_ARGS;
        }
        src.p[k] = params[k];
    }
    const int *map = pack_map_for(P, flags);
    const int2 *units = pack_units_for(P, flags);
    if (!map || !units) {
        set_error("dgs_deform_pack: could not allocate the pack map");
        return DGS_ERR_HIP;
    }
    const int nimg = P.nslots * 512, nunits = (int)P.units.size();
    hipLaunchKernelGGL(k_pack, dim3(nunits + div_up(P.nf32, 512)), dim3(512), 0, stream, map, src, units, nunits,
                       reinterpret_cast<_Float16 *>(packed), packed + P.img_floats(), nimg, P.nf32);
    DGS_LAUNCH_CHECK("k_pack", false, stream);
    return DGS_OK;
}

static void fwd_args(const Plan &P, int flags, int N, const float *xyz, const float *t, const float *packed, float *out,
                     float *saved, FwdArgs &a, hipStream_t stream);

// nosave: the training forward (saved given, frame-uniform t) with its saved-row and mask stores compiled
// out (k_fwd8_nosave); `saved` still receives k_timenet's constants, which backward_active() reads
int forward(int flags, int N, const float *xyz, const float *t, const float *packed, float *out, float *saved,
            hipStream_t stream, bool nosave) {
    const Plan P = make_plan(flags);
    FwdArgs a{};
    fwd_args(P, flags, N, xyz, t, packed, out, saved, a, stream);
    const int grid = persistent_grid(a.nblk, a.queue);
    if (nosave && !(saved && P.F.uniform_t)) {
        set_error("dgs_deform_forward: DGS_MLP_NO_SAVE needs DGS_MLP_UNIFORM_T and the saved buffer");
        return DGS_ERR_ARGS;
    }
    if (P.F.blender && (saved || P.F.uniform_t)) {
        // the folded biases (uniform t) are needed without saved activations too (inference)
        if (!a.tc) {
            set_error("dgs_deform_forward: could not allocate the timenet scratch");
            return DGS_ERR_HIP;
        }
        hipLaunchKernelGGL(k_timenet, dim3(1), dim3(256), 0, stream, a);
    }
    {
        ScopedTimer tm("mlp_fwd", stream);  // k_fwd only: the class's FLOP count is the trunk's + heads'
        const bool fold = P.F.uniform_t;  // t_emb folded into the biases (a.tc is set above)
        if (nosave)
            hipLaunchKernelGGL(k_fwd8_nosave, dim3(grid), dim3(NTHR8), 0, stream, a);
        else if (saved && fold)  // every training step: 8 waves of two n-tiles (DESIGN.md §"k_fwd8")
            hipLaunchKernelGGL(k_fwd8, dim3(grid), dim3(NTHR8), 0, stream, a);
        else if (saved)
            hipLaunchKernelGGL((k_fwd<true, false>), dim3(grid), dim3(NTHR), 0, stream, a);
        else if (fold)
            hipLaunchKernelGGL((k_fwd<false, true>), dim3(grid), dim3(NTHR), 0, stream, a);
        else
            hipLaunchKernelGGL((k_fwd<false, false>), dim3(grid), dim3(NTHR), 0, stream, a);
    }
    DGS_LAUNCH_CHECK("k_fwd", false, stream);
    return DGS_OK;
}

// The training step's pack + forward: pack() then forward() (k_pack, k_timenet, k_fwd). Round 5 tried
// the timenet inside the pack launch (one extra workgroup gathering its weights through the pack map):
// 59 us for that launch against 9 + 7 us for the two (rocprofv3, profiles/r5b_pack_tn_regression.txt;
// the map double-indirection serialised the timenet's loads and its registers lowered the pack's
// occupancy), so the two launches stay.
int pack_forward(int flags, const float *const *params, int N, const float *xyz, const float *t, float *packed,
                 float *out, float *saved, hipStream_t stream, bool nosave) {
    if (int rc = pack(flags, params, packed, stream)) return rc;
    return forward(flags, N, xyz, t, packed, out, saved, stream, nosave);
}

static void fwd_args(const Plan &P, int flags, int N, const float *xyz, const float *t, const float *packed, float *out,
                     float *saved, FwdArgs &a, hipStream_t stream) {
    a.N = N;
    a.Ns = padded_points(N);
    a.xyz = xyz; a.t = t; a.out = out; a.saved = saved;
    a.img = reinterpret_cast<const h16x8 *>(packed);
    a.fp = packed + P.img_floats();
    a.mask = saved ? reinterpret_cast<uint32_t *>(saved + (size_t)P.F.nsaved * a.Ns) : nullptr;
    a.fT1 = P.fT1; a.fT2 = P.fT2; a.fHd = P.fHd;
    a.bT1 = P.bT1; a.bT2 = P.bT2; a.bHd = P.bHd; a.wT1 = P.wT1; a.wT2 = P.wT2;
    a.w0te = P.w0te; a.w5te = P.w5te;
    for (int i = 0; i < 8; i++) { a.fL[i] = P.fL[i]; a.bL[i] = P.bL[i]; }
    a.flags = flags;
    const Blocks bs = block_split(N);
    a.nfull = bs.nfull;
    const int nblk = bs.nfull + bs.ntail;
    a.nblk = nblk;
    a.queue = nblk > 0 ? block_queue(stream, 0) : nullptr;
    a.n_dev = nullptr;
    a.ncu = tail_cus();
    a.tc = nullptr;
    if (P.F.blender && (saved || P.F.uniform_t))
        a.tc = saved ? saved + (size_t)P.F.nsaved * a.Ns + mask_words(P.F, a.Ns) : timenet_scratch(stream);
}

static int dw_split_once(const Flags &F, size_t Ns, int N, const int *n_dev, const float *dz, const float *saved,
                         float *slabs, float *const *grads, hipStream_t stream);

// n_dev: the point count in device memory (<= N: the active set) or nullptr: the N rows of dout
static int backward_n(int flags, int N, const int *n_dev, const float *packed, const float *saved, const float *dout,
                      float *scratch, float *const *grads, hipStream_t stream) {
    const Plan P = make_plan(flags);
    const Flags &F = P.F;
    const size_t Ns = padded_points(N);
    float *dz = scratch;
    float *slabs = scratch + (size_t)F.nz * Ns;
    BwdArgs b{};
    b.N = N; b.Ns = Ns; b.dout = dout; b.dz = dz;
    b.img = reinterpret_cast<const h16x8 *>(packed);
    b.mask = reinterpret_cast<const uint32_t *>(saved + (size_t)F.nsaved * Ns);
    b.tHd = P.tHd; b.tT2 = P.tT2;
    for (int i = 0; i < 8; i++) b.tL[i] = P.tL[i];
    b.flags = flags;
    const Blocks bs = block_split(N);
    b.nfull = bs.nfull;
    const int nblk = bs.nfull + bs.ntail;
    b.nblk = nblk;
    b.queue = nblk > 0 ? block_queue(stream, 1) : nullptr;
    b.n_dev = n_dev;
    b.ncu = tail_cus();
    const int grid = persistent_grid(nblk, b.queue);
    {
        ScopedTimer tm("mlp_bwd", stream);
        if (F.blender && !F.uniform_t)
            hipLaunchKernelGGL(k_bwd<true>, dim3(grid), dim3(NTHR), 0, stream, b);
        else
            // the 8-wave k_bwd8 (bitwise equal to the 16-wave form of the same block): neutral on the bf16x6
            // split (r5u), +0.5 % steps/s on the f16 split (mlp_bwd 0.333 -> 0.325 ms,
            // profiles/r6f_mlp_variants_ab.txt)
            hipLaunchKernelGGL(k_bwd8, dim3(grid), dim3(NTHR8), 0, stream, b);
    }
    DGS_LAUNCH_CHECK("k_bwd", false, stream);
    int rc;
    if (dw_mode() == 0 && !n_dev)
        rc = mlp::dw_fp32(F, Ns, dz, saved, slabs, grads, stream);
    else
        rc = dw_split_once(F, Ns, N, n_dev, dz, saved, slabs, grads, stream);
    if (rc != DGS_OK || !F.uniform_t) return rc;
    TGradArgs g{};
    g.fp = packed + P.img_floats();
    g.w0te = P.w0te; g.w5te = P.w5te; g.wT2 = P.wT2;
    g.tc = saved + (size_t)F.nsaved * Ns + mask_words(F, Ns);
    g.gb0 = grads[P.pLb[0]]; g.gb5 = grads[P.pLb[5]];
    g.gT0w = grads[P.pT0w]; g.gT0b = grads[P.pT0b]; g.gT2w = grads[P.pT2w]; g.gT2b = grads[P.pT2b];
    g.gW0 = grads[P.pLw[0]]; g.gW5 = grads[P.pLw[5]];
    g.tin = F.tin;
    {
        ScopedTimer tm("mlp_tgrad", stream);
        hipLaunchKernelGGL(k_tgrad, dim3(TG_WG), dim3(1024), 0, stream, g);
    }
    DGS_LAUNCH_CHECK("k_tgrad", false, stream);
    return DGS_OK;
}

// dW launches handed to the fp32 k_dw because a 256-row operand exceeds k_dws's 32-bit byte offsets
// (N > ~2.1 M points; dgs_debug_dw_fallbacks)
static std::atomic<long long> g_dw_fallbacks{0};
static bool dws_offsets_fit(size_t Ns) { return (size_t)WT * Ns * 4 < 0x7fffffffull; }
static int dw_split_once(const Flags &F, size_t Ns, int N, const int *n_dev, const float *dz, const float *saved,
                         float *slabs, float *const *grads, hipStream_t stream) {
    if (!dws_offsets_fit(Ns)) {  // 32-bit byte offsets of a 256-row operand
        if (n_dev) {  // active_supported() keeps such launches on the full path
            set_error("dgs_deform_backward_active: too many points for k_dws");
            return DGS_ERR_ARGS;
        }
        g_dw_fallbacks.fetch_add(1);
        return mlp::dw_fp32(F, Ns, dz, saved, slabs, grads, stream);
    }
    const WPlan W = split_wplan(F, std::max(32, 256 - reserved_cus()));
    for (int q = 0; q < W.jobs.n; q++) {  // the shapes k_dws instantiates
        const WJob &j = W.jobs.j[q];
        const bool ok = (j.krows == 256 && (j.nrows == 256 || j.nrows == 32)) ||
                        (j.nrows == 256 && (j.krows == 96 || j.krows == 64 || j.krows == 16));
        if (!ok) {
            set_error("dgs_deform_backward: dW job shape outside k_dws's instantiations");
            return DGS_ERR_ARGS;
        }
    }
    {
        if (int rc = ensure_dynamic_lds((const void *)k_dws, S_LDS)) return rc;
        ScopedTimer tm("mlp_dw", stream);
        hipLaunchKernelGGL(k_dws, dim3(W.nblocks), dim3(DW_THREADS), S_LDS, stream, W.jobs, Ns, N, n_dev, dz, saved,
                           slabs);
    }
    DGS_LAUNCH_CHECK("k_dws", false, stream);
    return launch_dw_reduce(F, W, slabs, grads, stream);
}

int backward(int flags, int N, const float *packed, const float *saved, const float *dout, float *scratch,
             float *const *grads, hipStream_t stream) {
    return backward_n(flags, N, nullptr, packed, saved, dout, scratch, grads, stream);
}

// ---- the active set (mlp_active.h). Scratch: M | the count kernel's per-workgroup counts | xyz_c | dout_c ----
struct ActiveBufs {
    int *m, *counts;
    float *xyz_c, *dout_c;
    size_t total;
};
static ActiveBufs active_bufs(const Flags &F, int N, float *base) {
    auto pad4 = [](size_t n) { return (n + 3) / 4 * 4; };
    ActiveBufs b{};
    size_t o = 4;
    b.m = reinterpret_cast<int *>(base);
    b.counts = reinterpret_cast<int *>(base + o);
    o += pad4(div_up(std::max(N, 1), ACT_ROWS));
    b.xyz_c = base + o;
    o += pad4((size_t)3 * N);
    b.dout_c = base + o;
    o += pad4((size_t)F.nout * N);
    b.total = o;
    return b;
}
size_t active_floats(int flags, int N) { return active_bufs(make_flags(flags), N, nullptr).total; }

// the recompute path runs the kernels that take a device point count: k_fwd8 / k_bwd8 (a frame-uniform
// t) and the split k_dws within its 32-bit offsets
bool active_supported(int flags, int N) {
    return make_flags(flags).uniform_t && dw_mode() == 3 && dws_offsets_fit(padded_points(N));
}

static ActiveArgs active_args(const Flags &F, int N, const float *xyz, const float *dout, const ActiveBufs &B,
                              uint32_t *m_host) {
    ActiveArgs g{};
    g.N = N; g.nout = F.nout; g.xyz = xyz; g.dout = dout;
    g.xyz_c = B.xyz_c; g.dout_c = B.dout_c; g.counts = B.counts; g.m_dev = B.m; g.m_host = m_host;
    return g;
}

// M only (a step on the full path: the active fraction is still measured)
int active_count(int flags, int N, const float *dout, float *active, uint32_t *m_host, hipStream_t stream) {
    const Flags F = make_flags(flags);
    const ActiveArgs g = active_args(F, N, nullptr, dout, active_bufs(F, N, active), m_host);
    ScopedTimer tm("mlp_active", stream);
    hipLaunchKernelGGL(k_active_count, dim3(div_up(N, ACT_ROWS)), dim3(ACT_ROWS), 0, stream, g);
    hipLaunchKernelGGL(k_active_gather, dim3(1), dim3(ACT_ROWS), 0, stream, g, 0);
    DGS_LAUNCH_CHECK("k_active_count", false, stream);
    return DGS_OK;
}

// The backward of a forward(nosave) launch with the same packed / saved buffers: compact the rows of
// dout with a nonzero element, rerun the saving forward on their xyz (k_timenet's constants of the
// first forward are in `saved`; no output rows), then the dX chain and dW on those M points.
int backward_active(int flags, int N, const float *xyz, const float *packed, float *saved, const float *dout,
                    float *scratch, float *active, uint32_t *m_host, float *const *grads, hipStream_t stream) {
    const Plan P = make_plan(flags);
    if (!active_supported(flags, N)) {
        set_error("dgs_deform_backward_active: not available for these flags / this size (dgs_deform_active_supported)");
        return DGS_ERR_ARGS;
    }
    const ActiveBufs B = active_bufs(P.F, N, active);
    const ActiveArgs g = active_args(P.F, N, xyz, dout, B, m_host);
    {
        ScopedTimer tm("mlp_active", stream);
        hipLaunchKernelGGL(k_active_count, dim3(div_up(N, ACT_ROWS)), dim3(ACT_ROWS), 0, stream, g);
        hipLaunchKernelGGL(k_active_gather, dim3(div_up(N, ACT_ROWS)), dim3(ACT_ROWS), 0, stream, g, 1);
    }
    DGS_LAUNCH_CHECK("k_active_gather", false, stream);
    FwdArgs a{};
    fwd_args(P, flags, N, B.xyz_c, nullptr, packed, nullptr, saved, a, stream);
    a.n_dev = B.m;
    {
        ScopedTimer tm("mlp_fwd_active", stream);
        hipLaunchKernelGGL(k_fwd8, dim3(persistent_grid(a.nblk, a.queue)), dim3(NTHR8), 0, stream, a);
    }
    DGS_LAUNCH_CHECK("k_fwd8", false, stream);
    return backward_n(flags, N, B.m, packed, saved, B.dout_c, scratch, grads, stream);
}

}  // namespace mlps
}  // namespace dgs

#ifdef DGS_MLP_PROFILE
extern "C" void dgs_mlps_set_prof(unsigned long long *p) {
    (void)hipMemcpyToSymbol(HIP_SYMBOL(dgs::mlps::dgs_mlps_prof), &p, sizeof(p));
}
#endif

// ------------------------------------------------------------------------------------------------
// C ABI (include/dgs.h): the f16-split path unless DGS_MLP_EXACT_FP32 is set in the flags
// ------------------------------------------------------------------------------------------------
using namespace dgs;

static bool exact_fp32(int flags) { return (flags & DGS_MLP_EXACT_FP32) != 0; }
static int net_flags(int flags) {
    return exact_fp32(flags) ? flags & (DGS_MLP_BLENDER | DGS_MLP_6DOF | DGS_MLP_NO_ROTSCALE)
                             : flags & (DGS_MLP_BLENDER | DGS_MLP_6DOF | DGS_MLP_NO_ROTSCALE | DGS_MLP_UNIFORM_T);
}

#ifdef DGS_CLOCK_STAMPS
// kernel k (0 k_fwd, 1 k_bwd, 2 k_dws): the last launch's per-workgroup stamps, out[6 b ..] =
// (shader clock start, end, 100 MHz real time start, end, HW_ID | XCC_ID << 32, 0) for b < n
// (diagnostic builds only)
extern "C" int dgs_debug_clock(int k, int n, unsigned long long *out) {
    static unsigned long long h[mlps::CLK_BLOCKS][6];
    if (k < 0 || k > 2 || n > mlps::CLK_BLOCKS) return -1;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(dgs::mlps::dgs_clk), sizeof(h), sizeof(h) * k) != hipSuccess) return -1;
    for (int b = 0; b < n; b++)
        for (int q = 0; q < 6; q++) out[6 * b + q] = h[b][q];
    return 0;
}
#endif

extern "C" void dgs_mlp_set_reserved_cus(int k) { mlps::g_reserve_cus.store(k < 0 ? 0 : k > 64 ? 64 : k); }
extern "C" int dgs_mlp_reserved_cus(void) { return mlps::reserved_cus(); }

extern "C" long long dgs_debug_dw_fallbacks(void) { return mlps::g_dw_fallbacks.load(); }

extern "C" long long dgs_debug_guard_expiries(void) {
    uint32_t v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(dgs::mlps::dgs_mlps_guard_expired), sizeof(v)) != hipSuccess) return -1;
    return (long long)v;
}

extern "C" int dgs_deform_outputs(int flags) { return mlpc::make_flags(flags).nout; }
extern "C" int dgs_deform_num_params(int flags) { return mlpc::make_params(mlpc::make_flags(flags)).nparams; }

extern "C" size_t dgs_deform_packed_floats(int flags) {
    return exact_fp32(flags) ? mlp::packed_floats(net_flags(flags)) : mlps::make_plan(net_flags(flags)).total();
}

extern "C" size_t dgs_deform_saved_floats(int flags, int N) {
    return exact_fp32(flags) ? mlp::saved_floats(net_flags(flags), N) : mlps::saved_floats(net_flags(flags), N);
}

extern "C" size_t dgs_deform_scratch_floats(int flags, int N) {
    return exact_fp32(flags) ? mlp::scratch_floats(net_flags(flags), N) : mlps::scratch_floats(net_flags(flags), N);
}

extern "C" int dgs_deform_pack(int flags, const float *const *params, float *packed, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!params || !packed) {
        set_error("dgs_deform_pack: null argument");
        return DGS_ERR_ARGS;
    }
    return exact_fp32(flags) ? mlp::pack(net_flags(flags), params, packed, stream)
                             : mlps::pack(net_flags(flags), params, packed, stream);
}

extern "C" int dgs_deform_forward(int flags, int N, const float *xyz, const float *t, const float *packed, float *out,
                                  float *saved, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0 || (N > 0 && (!xyz || !t || !packed || !out))) {
        set_error("dgs_deform_forward: null argument");
        return DGS_ERR_ARGS;
    }
    if (N == 0) return DGS_OK;
    if (exact_fp32(flags) && (flags & DGS_MLP_NO_SAVE)) {
        set_error("dgs_deform_forward: DGS_MLP_NO_SAVE is the split path's");
        return DGS_ERR_ARGS;
    }
    return exact_fp32(flags) ? mlp::forward(net_flags(flags), N, xyz, t, packed, out, saved, stream)
                             : mlps::forward(net_flags(flags), N, xyz, t, packed, out, saved, stream,
                                             (flags & DGS_MLP_NO_SAVE) != 0);
}

extern "C" int dgs_deform_pack_forward(int flags, const float *const *params, int N, const float *xyz, const float *t,
                                       float *packed, float *out, float *saved, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!params || !packed || N < 0 || (N > 0 && (!xyz || !t || !out))) {
        set_error("dgs_deform_pack_forward: null argument");
        return DGS_ERR_ARGS;
    }
    if (exact_fp32(flags) || N == 0) {
        if (int rc = dgs_deform_pack(flags, params, packed, stream_)) return rc;
        return dgs_deform_forward(flags, N, xyz, t, packed, out, saved, stream_);
    }
    return mlps::pack_forward(net_flags(flags), params, N, xyz, t, packed, out, saved, stream,
                              (flags & DGS_MLP_NO_SAVE) != 0);
}

extern "C" int dgs_deform_backward(int flags, int N, const float *packed, const float *saved, const float *dout,
                                   float *scratch, float *const *grads, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0 || (N > 0 && (!packed || !saved || !dout || !scratch || !grads))) {
        set_error("dgs_deform_backward: null argument");
        return DGS_ERR_ARGS;
    }
    const mlpc::Flags F = mlpc::make_flags(flags);
    const mlpc::Params P = mlpc::make_params(F);
    if (N == 0) {
        for (int k = 0; k < P.nparams; k++) {
            int r, c;
            mlpc::param_shape(F, P, k, r, c);
            DGS_HIP_CHECK(hipMemsetAsync(grads[k], 0, sizeof(float) * r * (c ? c : 1), stream));
        }
        return DGS_OK;
    }
    return exact_fp32(flags) ? mlp::backward(net_flags(flags), N, packed, saved, dout, scratch, grads, stream)
                             : mlps::backward(net_flags(flags), N, packed, saved, dout, scratch, grads, stream);
}

extern "C" int dgs_deform_active_supported(int flags, int N) {
    return !exact_fp32(flags) && N > 0 && mlps::active_supported(net_flags(flags), N);
}

extern "C" size_t dgs_deform_active_floats(int flags, int N) { return mlps::active_floats(net_flags(flags), N < 0 ? 0 : N); }

extern "C" int dgs_deform_active_count(int flags, int N, const float *dout, float *active, unsigned *count_host,
                                       void *stream_) {
    if (N <= 0 || !dout || !active) {
        set_error("dgs_deform_active_count: bad argument");
        return DGS_ERR_ARGS;
    }
    return mlps::active_count(net_flags(flags), N, dout, active, count_host, (hipStream_t)stream_);
}

extern "C" int dgs_deform_backward_active(int flags, int N, const float *xyz, const float *packed, float *saved,
                                          const float *dout, float *scratch, float *active, unsigned *count_host,
                                          float *const *grads, void *stream_) {
    if (N <= 0 || !xyz || !packed || !saved || !dout || !scratch || !active || !grads) {
        set_error("dgs_deform_backward_active: bad argument");
        return DGS_ERR_ARGS;
    }
    if (!dgs_deform_active_supported(flags, N)) {
        set_error("dgs_deform_backward_active: not available for these flags / this size (dgs_deform_active_supported)");
        return DGS_ERR_ARGS;
    }
    return mlps::backward_active(net_flags(flags), N, xyz, packed, saved, dout, scratch, active, count_host, grads,
                                 (hipStream_t)stream_);
}

extern "C" int dgs_mapped_word_alloc(unsigned **host, unsigned **dev) {
    if (!host || !dev) {
        set_error("dgs_mapped_word_alloc: null argument");
        return DGS_ERR_ARGS;
    }
    DGS_HIP_CHECK(hipHostMalloc((void **)host, sizeof(unsigned), hipHostMallocCoherent | hipHostMallocMapped));
    **host = 0xffffffffu;
    DGS_HIP_CHECK(hipHostGetDevicePointer((void **)dev, *host, 0));
    return DGS_OK;
}

extern "C" void dgs_mapped_word_free(unsigned *host) {
    if (host) (void)hipHostFree(host);
}
