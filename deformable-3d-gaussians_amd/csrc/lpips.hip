// LPIPS-VGG (lpips.LPIPS(net='vgg'), version 0.1) of F image pairs on MI355X, forward only.
//   scaling layer (v - shift) / scale  ->  VGG16 features, 13 convolutions 3x3 / stride 1 / zero pad 1 + bias
//   + ReLU, 2x2 max pools (floor) after conv 2, 4, 7, 10  ->  taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
//   ->  per tap: channel vector / (sqrt(sum_c f^2) + 1e-10), squared difference, lin weights, spatial mean
//   ->  out[f] = five layer terms and their sum.
// The 2F images (img frames, then gt frames) run through the same launches with the same tiling, so equal
// images give bitwise equal taps: (fx - fy)^2 is exactly 0 for them and exactly symmetric otherwise.
//
// Activations are channel-innermost, [image][y][x][c], in two scratch buffers used in turn.
// k_conv: implicit GEMM on v_mfma_f32_32x32x2_f32, rows = output channels, columns = pixels, K = 9 * Cin walked
// in chunks of 16 input channels. A 256-thread workgroup owns 16 x 16 pixels x 64 output channels of one image;
// per chunk it stages the 18 x 18 x 16 input patch (zero outside the image by predicate) and the 64 x 9 x 16
// weights in LDS, then each wave runs 4 rows of pixels (2 groups of 32) x 2 groups of 32 channels: four
// accumulators, 16 MFMAs per pair of 128-bit LDS reads of each operand. A lane's float4 is four k steps
// (channels 8c + 4h + j of tap t for lane half h), the same for both operands, so a chunk's 144 products are one
// fp32 fma chain in a fixed order; the chunks' sums are added up in a second accumulator, which keeps the rounding
// error of K = 4608 near that of its 32 chunk sums instead of one 4608-long chain (measured: DESIGN.md section 4).
// Bias and ReLU in the epilogue; a lane stores 4 consecutive channels of a pixel.
// The first layer is the same kernel with another loader: it reads the caller's planar (F, 3, H, W) floats,
// applies the optional 2v - 1 and the scaling layer, and fills channels 3..15 of its one chunk with zeros
// (its packed weights hold zeros there: K = 27 padded to 144).
// k_pool: 2x2 max, channel-innermost. k_tail: 16 lanes per pixel, 256 pixels per workgroup, one partial sum per
// workgroup; k_final: one workgroup per frame adds the partials of each tap in a fixed order in double. No
// atomics: results are bitwise reproducible and a frame's partials do not depend on the frames around it.
#include <hip/hip_runtime.h>

#include "dgs_common.h"

namespace dgs {
namespace lpips {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NCONV = 13, NTAP = 5;
constexpr int KC = 16;                  // input channels per K chunk
constexpr int TP = 16;                  // pixel tile side
constexpr int PW = TP + 2;              // patch side
constexpr int PS = KC + 4;              // LDS floats per patch pixel (padded: 16 lanes hit 16 bank groups)
constexpr int TN = 64;                  // output channels per workgroup
constexpr int WROW = 9 * KC;            // weights per output channel and chunk
constexpr int WS = WROW + 4;            // LDS floats per weight row (padded likewise)
constexpr int TAIL_PIX = 256;           // pixels per k_tail workgroup

// VGG16 feature stack: channels of conv l, whether a pool follows it, whether its output is a tap
constexpr int CIN[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int COUT[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr bool TAP_AFTER[NCONV] = {false, true, false, true, false, false, true, false, false, true, false, false, true};
constexpr int TAPC[NTAP] = {64, 128, 256, 512, 512};

inline int cin_padded(int l) { return l == 0 ? KC : CIN[l]; }

// packed weights, in floats: per conv [Cin_padded / 16][Cout][9][16] then bias[Cout]; then lin0..lin4
struct WeightMap {
    size_t w[NCONV], b[NCONV], lin[NTAP], floats;
};

inline WeightMap weight_map() {
    WeightMap m{};
    size_t at = 0;
    for (int l = 0; l < NCONV; l++) {
        m.w[l] = at;
        at += (size_t)cin_padded(l) * COUT[l] * 9;
        m.b[l] = at;
        at += COUT[l];
    }
    for (int k = 0; k < NTAP; k++) {
        m.lin[k] = at;
        at += TAPC[k];
    }
    m.floats = at;
    return m;
}

__device__ __forceinline__ void mfma4(f32x16 &acc, const float4 &a, const float4 &b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// FIRST: in0 / in1 are the caller's planar img / gt (F, 3, H, W), image n < F from in0, else from in1;
// otherwise in0 is [N][H][W][Cin] and in1 unused. wpk: this layer's packed weights, bias: its Cout biases.
// grid (tiles x, tiles y, N * Cout / 64).
template <bool FIRST>
__global__ __launch_bounds__(256) void k_conv(int F, int H, int W, int Cin, int Cout, const float *__restrict__ in0,
                                              const float *__restrict__ in1, int normalize,
                                              const float *__restrict__ wpk, const float *__restrict__ bias,
                                              float *__restrict__ out) {
    __shared__ float4 patch[PW * PW * PS / 4];
    __shared__ float4 wl[TN * WS / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, m = lane & 31;
    const int ntn = Cout / TN;
    const int n = blockIdx.z / ntn, co0 = (blockIdx.z % ntn) * TN;
    const int x0 = blockIdx.x * TP, y0 = blockIdx.y * TP;

    // acc: the running chunk's 144 k steps; tot: the chunks' sums (FIRST has one chunk and no tot)
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[a][b][i] = tot[a][b][i] = 0.f;

    // this lane's pixel in the two pixel groups of its wave: tile row 4 wave + 2 g + (m >> 4), column m & 15
    const int prow = 4 * wave + (m >> 4), pcol = m & 15;
    const int nchunk = FIRST ? 1 : Cin / KC;
    for (int c = 0; c < nchunk; c++) {
        if (c) __syncthreads();  // the previous chunk's reads
        if (FIRST) {
            for (int e = tid; e < PW * PW; e += 256) {
                const int gy = y0 - 1 + e / PW, gx = x0 - 1 + e % PW;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const float *src = (n < F ? in0 + (size_t)n * 3 * H * W : in1 + (size_t)(n - F) * 3 * H * W) +
                                       (size_t)gy * W + gx;
                    float r = src[0], g = src[(size_t)H * W], b = src[2 * (size_t)H * W];
                    if (normalize) {
                        r = 2.f * r - 1.f;
                        g = 2.f * g - 1.f;
                        b = 2.f * b - 1.f;
                    }
                    v.x = __fdiv_rn(r - -0.030f, 0.458f);
                    v.y = __fdiv_rn(g - -0.088f, 0.448f);
                    v.z = __fdiv_rn(b - -0.188f, 0.450f);
                }
                patch[e * (PS / 4)] = v;
                patch[e * (PS / 4) + 1] = patch[e * (PS / 4) + 2] = patch[e * (PS / 4) + 3] =
                    make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            const float *src = in0 + (size_t)n * H * W * Cin + c * KC;
            for (int e = tid; e < PW * PW * (KC / 4); e += 256) {
                const int pix = e >> 2, q = e & 3;
                const int gy = y0 - 1 + pix / PW, gx = x0 - 1 + pix % PW;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < H && gx >= 0 && gx < W)
                    v = *reinterpret_cast<const float4 *>(src + ((size_t)gy * W + gx) * Cin + 4 * q);
                patch[pix * (PS / 4) + q] = v;
            }
        }
        {
            const float4 *src = reinterpret_cast<const float4 *>(wpk + ((size_t)c * Cout + co0) * WROW);
            for (int e = tid; e < TN * (WROW / 4); e += 256) wl[(e / (WROW / 4)) * (WS / 4) + e % (WROW / 4)] = src[e];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int pi = (prow + t / 3) * PW + pcol + t % 3;
#pragma unroll
            for (int c8 = 0; c8 < KC / 8; c8++) {
                const int ko = 2 * c8 + h;  // float4 index inside a 16-channel run
                const float4 a0 = wl[m * (WS / 4) + t * (KC / 4) + ko];
                const float4 a1 = wl[(32 + m) * (WS / 4) + t * (KC / 4) + ko];
                const float4 b0 = patch[pi * (PS / 4) + ko];
                const float4 b1 = patch[(pi + 2 * PW) * (PS / 4) + ko];
                mfma4(acc[0][0], a0, b0);
                mfma4(acc[0][1], a0, b1);
                mfma4(acc[1][0], a1, b0);
                mfma4(acc[1][1], a1, b1);
            }
        }
        if (!FIRST) {
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    tot[a][b] += acc[a][b];
#pragma unroll
                    for (int i = 0; i < 16; i++) acc[a][b][i] = 0.f;
                }
        }
    }
    if (!FIRST) {
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) acc[a][b] = tot[a][b];
    }
    // accumulator register 4 j + i of lane (h, m): channel 32 a + 8 j + 4 h + i, pixel m of group b
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int y = y0 + prow + 2 * b, x = x0 + pcol;
        if (y >= H || x >= W) continue;
        float *dst = out + (((size_t)n * H + y) * W + x) * Cout + co0;
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int ch = 32 * a + 8 * j + 4 * h;
                const float4 bv = *reinterpret_cast<const float4 *>(bias + co0 + ch);
                float4 v;
                v.x = fmaxf(acc[a][b][4 * j] + bv.x, 0.f);
                v.y = fmaxf(acc[a][b][4 * j + 1] + bv.y, 0.f);
                v.z = fmaxf(acc[a][b][4 * j + 2] + bv.z, 0.f);
                v.w = fmaxf(acc[a][b][4 * j + 3] + bv.w, 0.f);
                *reinterpret_cast<float4 *>(dst + ch) = v;
            }
    }
}

// 2x2 max, stride 2, floor: [N][h][w][C] -> [N][h/2][w/2][C]; one thread per 4 channels of an output pixel
__global__ __launch_bounds__(256) void k_pool(size_t total, int h, int w, int C, const float *__restrict__ in,
                                              float *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c4 = C / 4, ph = h / 2, pw = w / 2;
    const int q = (int)(e % c4);
    size_t p = e / c4;
    const int ox = (int)(p % pw);
    p /= pw;
    const int oy = (int)(p % ph);
    const size_t n = p / ph;
    const float *src = in + ((n * h + 2 * oy) * w + 2 * ox) * C + 4 * q;
    const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + C);
    const float4 c = *reinterpret_cast<const float4 *>(src + (size_t)w * C);
    const float4 d = *reinterpret_cast<const float4 *>(src + (size_t)w * C + C);
    float4 r;
    r.x = fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x));
    r.y = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y));
    r.z = fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z));
    r.w = fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w));
    *reinterpret_cast<float4 *>(out + e * 4) = r;
}

// sum over the 16 lanes of a pixel's group; every lane gets the same bits
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One tap of frame blockIdx.y, pixels [256 blockIdx.x, +256): sum over them of
// sum_c lin[c] (fx[c] / (|fx| + 1e-10) - fy[c] / (|fy| + 1e-10))^2 -> partial[frame * np + blockIdx.x].
// act: [2F][hw][C], image F + f is frame f's gt.
__global__ __launch_bounds__(256) void k_tail(int F, int hw, int C, const float *__restrict__ act,
                                              const float *__restrict__ lin, double *__restrict__ partial, int np) {
    __shared__ double red[16];
    const int f = blockIdx.y, g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const float *X = act + (size_t)f * hw * C, *Y = act + (size_t)(F + f) * hw * C;
    double s = 0.0;  // pixels add up in double: fp32 would lose what the per-pixel sums still carry
    for (int it = 0; it < TAIL_PIX / 16; it++) {
        const int p = blockIdx.x * TAIL_PIX + it * 16 + g;
        const bool valid = p < hw;
        const size_t at = (size_t)(valid ? p : hw - 1) * C;
        float sx = 0.f, sy = 0.f;
        for (int c = 4 * l; c < C; c += 64) {
            const float4 a = *reinterpret_cast<const float4 *>(X + at + c);
            const float4 b = *reinterpret_cast<const float4 *>(Y + at + c);
            sx = fmaf(a.x, a.x, sx); sx = fmaf(a.y, a.y, sx); sx = fmaf(a.z, a.z, sx); sx = fmaf(a.w, a.w, sx);
            sy = fmaf(b.x, b.x, sy); sy = fmaf(b.y, b.y, sy); sy = fmaf(b.z, b.z, sy); sy = fmaf(b.w, b.w, sy);
        }
        const float nx = __fsqrt_rn(sum16(sx)) + 1e-10f, ny = __fsqrt_rn(sum16(sy)) + 1e-10f;
        float d = 0.f;
        for (int c = 4 * l; c < C; c += 64) {
            const float4 a = *reinterpret_cast<const float4 *>(X + at + c);
            const float4 b = *reinterpret_cast<const float4 *>(Y + at + c);
            const float4 w = *reinterpret_cast<const float4 *>(lin + c);
            // (w u) u: the same bits for u and -u, and 0 for u == 0
            float u = __fdiv_rn(a.x, nx) - __fdiv_rn(b.x, ny);
            d = fmaf(w.x * u, u, d);
            u = __fdiv_rn(a.y, nx) - __fdiv_rn(b.y, ny);
            d = fmaf(w.y * u, u, d);
            u = __fdiv_rn(a.z, nx) - __fdiv_rn(b.z, ny);
            d = fmaf(w.z * u, u, d);
            u = __fdiv_rn(a.w, nx) - __fdiv_rn(b.w, ny);
            d = fmaf(w.w * u, u, d);
        }
        d = sum16(d);
        if (valid) s += (double)d;
    }
    if (l == 0) red[g] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 16; i++) t += red[i];
        partial[(size_t)f * np + blockIdx.x] = t;
    }
}

// where k_tail left each tap's partial sums inside a frame's np doubles, and how many pixels they cover
struct Geo {
    int off[NTAP], n[NTAP], hw[NTAP], np;
};

// one workgroup per frame: out[f] = five layer terms (mean over pixels), then their sum
__global__ __launch_bounds__(256) void k_final(Geo g, const double *__restrict__ partial, float *__restrict__ out) {
    __shared__ double red[NTAP][4];
    const int f = blockIdx.x;
    const double *p = partial + (size_t)f * g.np;
    for (int k = 0; k < NTAP; k++) {
        double a = 0.0;
        for (int i = threadIdx.x; i < g.n[k]; i += 256) a += p[g.off[k] + i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < NTAP; k++) {
            const double term = ((red[k][0] + red[k][1]) + (red[k][2] + red[k][3])) / (double)g.hw[k];
            out[(size_t)f * 6 + k] = (float)term;
            total += term;
        }
        out[(size_t)f * 6 + 5] = (float)total;
    }
}

// scratch: partials [F][np] doubles | buffer 0 [2F][64 H W] | buffer 1 likewise. Every part is a multiple
// of F, so dgs_lpips_scratch_bytes(F) = F * dgs_lpips_scratch_bytes(1).
struct Layout {
    Geo g;
    int h[NTAP], w[NTAP];
    size_t buf;  // floats of one buffer per frame pair
};

Layout make_layout(int H, int W) {
    Layout L{};
    int at = 0, h = H, w = W;
    for (int k = 0; k < NTAP; k++) {
        L.h[k] = h;
        L.w[k] = w;
        L.g.off[k] = at;
        L.g.hw[k] = h * w;
        L.g.n[k] = div_up(h * w, TAIL_PIX);
        at += L.g.n[k];
        h /= 2;
        w /= 2;
    }
    L.g.np = (at + 3) & ~3;
    L.buf = 2 * (size_t)64 * H * W;
    return L;
}

const char *bad_shape(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0) return "F, H and W must be positive";
    if ((H < W ? H : W) < 16) return "LPIPS-VGG needs min(H, W) >= 16 (four 2x2 pools)";
    return nullptr;
}

}  // namespace lpips
}  // namespace dgs

using namespace dgs;

extern "C" size_t dgs_lpips_weight_floats(void) { return lpips::weight_map().floats; }

extern "C" size_t dgs_lpips_scratch_bytes(int F, int H, int W) {
    if (lpips::bad_shape(F, H, W)) return 0;
    const lpips::Layout L = lpips::make_layout(H, W);
    return (size_t)F * (sizeof(double) * L.g.np + sizeof(float) * 2 * L.buf);
}

extern "C" int dgs_lpips(int F, int H, int W, const float *img, const float *gt, const float *weights, unsigned flags,
                         float *out, float *taps, void *scratch_, void *stream_) {
    using namespace lpips;
    hipStream_t stream = (hipStream_t)stream_;
    if (!img || !gt || !weights || !out || !scratch_) {
        set_error("dgs_lpips: null pointer");
        return DGS_ERR_ARGS;
    }
    if (const char *why = bad_shape(F, H, W)) {
        set_error(std::string("dgs_lpips: ") + why);
        return DGS_ERR_ARGS;
    }
    if (flags & ~DGS_LPIPS_NORMALIZE) {
        set_error("dgs_lpips: unknown flag");
        return DGS_ERR_ARGS;
    }
    // blockIdx.z = image * Cout / 64, blockIdx.y = tile row; pixel counts are ints
    if (F > 4095 || H > (1 << 19) || (long long)H * W > (1ll << 30)) {
        set_error("dgs_lpips: more than 4095 frames, H above 524288 or more than 2^30 pixels (score in chunks)");
        return DGS_ERR_UNSUPPORTED;
    }
    const Layout L = make_layout(H, W);
    const WeightMap wm = weight_map();
    double *partial = (double *)scratch_;
    float *buf0 = (float *)(partial + (size_t)F * L.g.np);
    float *buf[2] = {buf0, buf0 + (size_t)F * L.buf};
    const int N = 2 * F;
    int cur = 1, h = H, w = W, tap = 0;  // conv l reads buf[cur] and writes buf[cur ^ 1]
    for (int l = 0; l < NCONV; l++) {
        const dim3 grid(div_up(w, TP), div_up(h, TP), N * (COUT[l] / TN));
        float *dst = buf[cur ^ 1];
        if (l == 0)
            hipLaunchKernelGGL(k_conv<true>, grid, dim3(256), 0, stream, F, h, w, 3, COUT[l], img, gt,
                               (int)(flags & DGS_LPIPS_NORMALIZE), weights + wm.w[l], weights + wm.b[l], dst);
        else
            hipLaunchKernelGGL(k_conv<false>, grid, dim3(256), 0, stream, F, h, w, CIN[l], COUT[l], buf[cur],
                               (const float *)nullptr, 0, weights + wm.w[l], weights + wm.b[l], dst);
        cur ^= 1;
        if (!TAP_AFTER[l]) continue;
        const int C = COUT[l];
        hipLaunchKernelGGL(k_tail, dim3(L.g.n[tap], F), dim3(256), 0, stream, F, h * w, C, buf[cur],
                           weights + wm.lin[tap], partial + L.g.off[tap], L.g.np);
        if (taps) {
            const size_t nf = (size_t)F * h * w * C;
            DGS_HIP_CHECK(hipMemcpyAsync(taps, buf[cur], nf * sizeof(float), hipMemcpyDeviceToDevice, stream));
            taps += nf;
        }
        if (++tap < NTAP) {
            const size_t total = (size_t)N * (h / 2) * (w / 2) * (C / 4);
            hipLaunchKernelGGL(k_pool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, h, w, C,
                               buf[cur], buf[cur ^ 1]);
            cur ^= 1;
            h /= 2;
            w /= 2;
        }
    }
    hipLaunchKernelGGL(k_final, dim3(F), dim3(256), 0, stream, L.g, partial, out);
    DGS_LAUNCH_CHECK("lpips", false, stream);
    return DGS_OK;
}
