// Batched image metrics for MI355X: PSNR, SSIM and MS-SSIM of F frame pairs in one call, forward only.
//   PSNR    utils/image_utils.py:19-21 per frame: 20 log10(1 / sqrt(mean (I-G)^2)).
//   SSIM    utils/loss_utils.py:41-73: the quantity k_ssim_fwd (ssim.hip) sums, with its window taps,
//           its tile load and its per-pixel expression (ssim_tile.h), without the three backward maps.
//   MS-SSIM pytorch_msssim.ms_ssim(data_range=1): five levels of a *valid* (unpadded) 11x11 sigma-1.5
//           filter, avg_pool2d(2, 2, padding = side mod 2, zeros counted) between levels,
//           prod_l relu(cs_l)^w_l * relu(ssim_4)^w_4 per channel, mean over channels.
// Every kernel has the frame (times channel) in blockIdx.z, so a call is a fixed number of launches:
// one zero-padded tile pass (squared error + SSIM), five valid tile passes and four pools for the
// pyramid (scratch), one final reduction. Tiles write partial sums; k_final adds them in a fixed order
// in double: no atomics, results are bitwise reproducible and a frame's sums see only its own tiles.
//
// Tile pass = k_ssim_fwd's structure on ssim_tile.h's pieces: 32x32 outputs per 256-thread workgroup from
// a 42x42 LDS tile, separable 11-tap row pass (18 inputs in registers for 8 outputs) and column pass (14
// for 4), written out here as in k_ssim_fwd (why: ssim_tile.h).
// The valid pass differs in the tile's origin (outputs (x, y) read inputs x..x+10, y..y+10) and in the
// outputs that exist (w-10 by h-10). It also filters x - cx and y - cy, cx / cy = the tile's centre
// pixel of each image: variances and the covariance do not change under a shift, and g*x^2 - mu^2 then
// cancels at the size of the local contrast, not of the brightness (at level 4 one pixel is the whole
// mean, so nothing averages the rounding out). mu gets the constant back. The five filtered sums run
// the same taps in the same order and the epilogue rounds every product on its own, so x == y gives
// cs == 1 and ssim == 1 exactly.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dgs_common.h"
#include "ssim_tile.h"

namespace dgs {
namespace metrics {

using namespace ssim;  // ssim_tile.h: the tile constants, Win, load_tile, ssim_pixel, tile_sums

constexpr int LEVELS = 5;
constexpr int MIN_SIDE = (11 - 1) * 16;  // MS-SSIM needs min(H, W) > 160

// a product the compiler may not contract into the add or subtract that uses it
__device__ __forceinline__ float rounded(float v) {
    asm("" : "+v"(v));
    return v;
}

// cs and luminance * cs of one pixel of a valid level from the five filtered sums of (x - cx, y - cy).
// With x == y the operands of each quotient must be bitwise equal (both are then exactly 1): every
// product is rounded on its own, since a*a + b*b as fma(a, a, round(b*b)) is not 2 round(a*b).
// (2 s + C as an fma rounds once either way: 2 s is exact.)
__device__ __forceinline__ void level_terms(float m0, float m1, float e00, float e11, float e01, float cx, float cy,
                                            float &cs, float &sv) {
    const float s11 = e00 - rounded(m0 * m0), s22 = e11 - rounded(m1 * m1), s12 = e01 - rounded(m0 * m1);
    const float mu1 = m0 + cx, mu2 = m1 + cy;
    const float n1 = 2.f * rounded(mu1 * mu2) + C1, d1 = (rounded(mu1 * mu1) + rounded(mu2 * mu2)) + C1;
    const float n2 = 2.f * s12 + C2, d2 = (s11 + s22) + C2;
    cs = __fdiv_rn(n2, d2);
    sv = __fdiv_rn(n1, d1) * cs;
}

// One 32x32 tile of one plane. VALID = false: zero-padded 'same' filter (the loss's SSIM) ->
// partial = (sum (x-y)^2, sum ssim). VALID = true: unpadded filter of an MS-SSIM level ->
// partial = (sum cs, sum ssim) over the (h-10) x (w-10) outputs. partial: [plane][tile y][tile x][2].
// The tap sums are explicit fmaf, as k_ssim_fwd's (ssim.hip says why): the two stay bit for bit alike.
template <bool VALID>
__global__ __launch_bounds__(256) void k_tile(int h, int w, const float *__restrict__ X, const float *__restrict__ Y,
                                              Win win, float *__restrict__ partial) {
    __shared__ float sx[2][S][SP];
    __shared__ float hq[5][S][HP];
    __shared__ float red[2][4];
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int tid = threadIdx.x;
    const size_t plane = (size_t)h * w;
    const float *px = X + blockIdx.z * plane, *py = Y + blockIdx.z * plane;
    const int ox = VALID ? x0 : x0 - R, oy = VALID ? y0 : y0 - R;  // origin of the input tile
    float cx = 0.f, cy = 0.f;
    if (VALID) {
        const size_t pc = (size_t)min(oy + S / 2, h - 1) * w + min(ox + S / 2, w - 1);
        cx = px[pc];
        cy = py[pc];
    }
    const float *src[2] = {px, py};
    const float centre[2] = {cx, cy};
    load_tile<2, VALID>(sx, src, h, w, ox, oy, centre);
    __syncthreads();
    if (tid < S * (T / HX)) {
        const int ly = tid / (T / HX), lx0 = (tid % (T / HX)) * HX;
        float a[HX + 10], b[HX + 10];
#pragma unroll
        for (int k = 0; k < HX + 10; k++) {
            a[k] = sx[0][ly][lx0 + k];
            b[k] = sx[1][ly][lx0 + k];
        }
#pragma unroll
        for (int j = 0; j < HX; j++) {
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float i = a[j + k], g = b[j + k], wk = win.w[k];
                m0 = fmaf(wk, i, m0);
                m1 = fmaf(wk, g, m1);
                m2 = fmaf(wk, i * i, m2);
                m3 = fmaf(wk, g * g, m3);
                m4 = fmaf(wk, i * g, m4);
            }
            hq[0][ly][lx0 + j] = m0; hq[1][ly][lx0 + j] = m1; hq[2][ly][lx0 + j] = m2;
            hq[3][ly][lx0 + j] = m3; hq[4][ly][lx0 + j] = m4;
        }
    }
    __syncthreads();
    const int lx = tid % T, ly0 = (tid / T) * VY;
    const int x = x0 + lx;
    float mu[5][VY];
#pragma unroll
    for (int m = 0; m < 5; m++) {
        float v[VY + 10];
#pragma unroll
        for (int k = 0; k < VY + 10; k++) v[k] = hq[m][ly0 + k][lx];
#pragma unroll
        for (int j = 0; j < VY; j++) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) acc = fmaf(win.w[k], v[j + k], acc);
            mu[m][j] = acc;
        }
    }
    const int ow = VALID ? w - 2 * R : w, oh = VALID ? h - 2 * R : h;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < VY; j++) {
        const int y = y0 + ly0 + j;
        if (x < ow && y < oh) {
            if (VALID) {
                float cs, sv;
                level_terms(mu[0][j], mu[1][j], mu[2][j], mu[3][j], mu[4][j], cx, cy, cs, sv);
                s0 += cs;
                s1 += sv;
            } else {
                // the loss's expression, so that this is the value fused_ssim returns
                const float d = sx[0][ly0 + j + R][lx + R] - sx[1][ly0 + j + R][lx + R];
                s0 += d * d;
                s1 += ssim_pixel(mu[0][j], mu[1][j], mu[2][j], mu[3][j], mu[4][j]).sv;
            }
        }
    }
    tile_sums(s0, s1, red, partial);
}

// avg_pool2d(kernel 2, stride 2, padding (h & 1, w & 1), count_include_pad) of both images' planes:
// (h, w) -> (ph, pw); 64 x 4 outputs per workgroup
__global__ __launch_bounds__(256) void k_pool(int h, int w, int ph, int pw, const float *__restrict__ X,
                                              const float *__restrict__ Y, float *__restrict__ PX,
                                              float *__restrict__ PY) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= pw || oy >= ph) return;
    const size_t src = blockIdx.z * ((size_t)h * w), dst = blockIdx.z * ((size_t)ph * pw) + (size_t)oy * pw + ox;
    const int ix = 2 * ox - (w & 1), iy = 2 * oy - (h & 1);
    float a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gx = ix + (k & 1), gy = iy + (k >> 1);
        const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
        const size_t p = in ? src + (size_t)gy * w + gx : 0;
        a[k] = in ? X[p] : 0.f;
        b[k] = in ? Y[p] : 0.f;
    }
    PX[dst] = 0.25f * ((a[0] + a[1]) + (a[2] + a[3]));
    PY[dst] = 0.25f * ((b[0] + b[1]) + (b[2] + b[3]));
}

// where the tile passes left their partial sums (float offsets into scratch) and what they count
struct Geo {
    size_t off_same, off[LEVELS];
    int nt_same, nt[LEVELS];  // tiles per plane
    double n_same, n[LEVELS];  // pixels per plane
};

// sums of n (a, b) pairs, in a fixed order, in double; every thread returns the totals
__device__ inline void block_sum2(const float *__restrict__ p, int n, double (*red)[4], double &a, double &b) {
    a = 0.0;
    b = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        a += (double)p[2 * (size_t)i];
        b += (double)p[2 * (size_t)i + 1];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    __syncthreads();  // the previous call's reads of red
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// one workgroup per frame: out[f] = psnr, ssim, ms_ssim, cs[5][C], ssim[5][C]; unrequested slots NaN
__global__ __launch_bounds__(256) void k_final(int C, unsigned what, Geo g, const float *__restrict__ scratch,
                                               float *__restrict__ out) {
    __shared__ double red[2][4];
    const int f = blockIdx.x;
    const bool lead = threadIdx.x == 0;
    float *o = out + (size_t)f * (3 + 2 * LEVELS * C);
    const float nan = __builtin_nanf("");
    float psnr = nan, ss = nan, ms = nan;
    if (what & (DGS_METRIC_PSNR | DGS_METRIC_SSIM)) {
        double se, sv;
        block_sum2(scratch + g.off_same + 2 * ((size_t)f * C * g.nt_same), C * g.nt_same, red, se, sv);
        const double n = g.n_same * C;
        if (what & DGS_METRIC_PSNR) psnr = (float)(20.0 * log10(1.0 / sqrt(se / n)));
        if (what & DGS_METRIC_SSIM) ss = (float)(sv / n);
    }
    if (what & DGS_METRIC_MS_SSIM) {
        const double wl[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        double acc = 0.0;
        for (int c = 0; c < C; c++) {
            double prod = 1.0;
            for (int l = 0; l < LEVELS; l++) {
                double cs, sv;
                block_sum2(scratch + g.off[l] + 2 * (((size_t)f * C + c) * g.nt[l]), g.nt[l], red, cs, sv);
                cs /= g.n[l];
                sv /= g.n[l];
                if (lead) {
                    o[3 + l * C + c] = (float)cs;
                    o[3 + (LEVELS + l) * C + c] = (float)sv;
                }
                prod *= pow(fmax(l < LEVELS - 1 ? cs : sv, 0.0), wl[l]);
            }
            acc += prod;
        }
        ms = (float)(acc / C);
    } else if (lead) {
        for (int i = 0; i < 2 * LEVELS * C; i++) o[3 + i] = nan;
    }
    if (lead) {
        o[0] = psnr;
        o[1] = ss;
        o[2] = ms;
    }
}

// side of the next pyramid level: floor((s + 2 (s mod 2) - 2) / 2) + 1
inline int pooled(int s) { return (s + 2 * (s & 1) - 2) / 2 + 1; }

inline int tiles(int h, int w) { return div_up(h, T) * div_up(w, T); }

// scratch, in floats: same-pass partials | level partials 0..4 | pooled img levels 1..4 | pooled gt 1..4
struct Layout {
    Geo g;
    int h[LEVELS], w[LEVELS];
    size_t pyr_x[LEVELS], pyr_y[LEVELS];  // [0] unused: level 0 is the input
    size_t floats;
};

Layout make_layout(int F, int C, int H, int W, unsigned what) {
    Layout L{};
    const size_t planes = (size_t)F * C;
    size_t at = 0;
    if (what & (DGS_METRIC_PSNR | DGS_METRIC_SSIM)) {
        L.g.off_same = at;
        L.g.nt_same = tiles(H, W);
        L.g.n_same = (double)H * W;
        at += 2 * planes * L.g.nt_same;
    }
    if (what & DGS_METRIC_MS_SSIM) {
        L.h[0] = H;
        L.w[0] = W;
        for (int l = 1; l < LEVELS; l++) {
            L.h[l] = pooled(L.h[l - 1]);
            L.w[l] = pooled(L.w[l - 1]);
        }
        for (int l = 0; l < LEVELS; l++) {
            L.g.off[l] = at;
            L.g.nt[l] = tiles(L.h[l] - 2 * R, L.w[l] - 2 * R);
            L.g.n[l] = (double)(L.h[l] - 2 * R) * (L.w[l] - 2 * R);
            at += 2 * planes * L.g.nt[l];
        }
        for (int l = 1; l < LEVELS; l++) {
            L.pyr_x[l] = at;
            at += planes * L.h[l] * L.w[l];
            L.pyr_y[l] = at;
            at += planes * L.h[l] * L.w[l];
        }
    }
    L.floats = at;
    return L;
}

// pytorch_msssim's 1-D window: exp(-(k-5)^2 / (2 * 1.5^2)) over its sum, as fp32 taps
Win ms_window() {
    double g[11], sum = 0.0;
    for (int k = 0; k < 11; k++) {
        g[k] = std::exp(-(double)((k - R) * (k - R)) / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    Win w;
    for (int k = 0; k < 11; k++) w.w[k] = (float)(g[k] / sum);
    return w;
}

constexpr unsigned ALL = DGS_METRIC_PSNR | DGS_METRIC_SSIM | DGS_METRIC_MS_SSIM;

// 0 = fine; else the reason (set_error text)
const char *bad_shape(int F, int C, int H, int W, unsigned what) {
    if (F <= 0 || C <= 0 || H <= 0 || W <= 0) return "F, C, H and W must be positive";
    if (!(what & ALL) || (what & ~ALL)) return "`what` must be a non-empty set of DGS_METRIC_PSNR | _SSIM | _MS_SSIM";
    if ((what & DGS_METRIC_MS_SSIM) && (H < W ? H : W) <= MIN_SIDE)
        return "MS-SSIM needs min(H, W) > 160 (five levels of an unpadded 11-tap filter: (11 - 1) * 2^4)";
    return nullptr;
}

}  // namespace metrics
}  // namespace dgs

using namespace dgs;

extern "C" size_t dgs_image_metrics_scratch_bytes(int F, int C, int H, int W, unsigned what) {
    if (metrics::bad_shape(F, C, H, W, what)) return 0;
    return sizeof(float) * metrics::make_layout(F, C, H, W, what).floats;
}

extern "C" int dgs_image_metrics(int F, int C, int H, int W, const float *img, const float *gt, unsigned what,
                                 float *out, void *scratch_, void *stream_) {
    using namespace metrics;
    hipStream_t stream = (hipStream_t)stream_;
    if (!img || !gt || !out || !scratch_) {
        set_error("dgs_image_metrics: null pointer");
        return DGS_ERR_ARGS;
    }
    if (const char *why = bad_shape(F, C, H, W, what)) {
        set_error(std::string("dgs_image_metrics: ") + why);
        return DGS_ERR_ARGS;
    }
    // the plane index is blockIdx.z, tile rows blockIdx.y
    if ((long long)F * C > 65535 || H > (1 << 18)) {
        set_error("dgs_image_metrics: more than 65535 planes (F * C) or H above 262144");
        return DGS_ERR_UNSUPPORTED;
    }
    float *scratch = (float *)scratch_;
    const Layout L = make_layout(F, C, H, W, what);
    const int planes = F * C;
    if (what & (DGS_METRIC_PSNR | DGS_METRIC_SSIM)) {
        hipLaunchKernelGGL(k_tile<false>, dim3(div_up(W, T), div_up(H, T), planes), dim3(256), 0, stream, H, W, img, gt,
                           ssim::make_window(), scratch + L.g.off_same);
    }
    if (what & DGS_METRIC_MS_SSIM) {
        const Win win = ms_window();
        const float *x = img, *y = gt;
        for (int l = 0; l < LEVELS; l++) {
            const int h = L.h[l], w = L.w[l];
            hipLaunchKernelGGL(k_tile<true>, dim3(div_up(w - 2 * R, T), div_up(h - 2 * R, T), planes), dim3(256), 0,
                               stream, h, w, x, y, win, scratch + L.g.off[l]);
            if (l + 1 < LEVELS) {
                const int ph = L.h[l + 1], pw = L.w[l + 1];
                float *nx = scratch + L.pyr_x[l + 1], *ny = scratch + L.pyr_y[l + 1];
                hipLaunchKernelGGL(k_pool, dim3(div_up(pw, 64), div_up(ph, 4), planes), dim3(256), 0, stream, h, w, ph, pw,
                                   x, y, nx, ny);
                x = nx;
                y = ny;
            }
        }
    }
    hipLaunchKernelGGL(k_final, dim3(F), dim3(256), 0, stream, C, what, L.g, scratch, out);
    DGS_LAUNCH_CHECK("image_metrics", false, stream);
    return DGS_OK;
}
