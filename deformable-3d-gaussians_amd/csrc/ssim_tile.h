// What the SSIM tile kernels of the training loss (ssim.hip) and of the batched image metrics
// (metrics.hip) share, written once: the tile geometry (one 256-thread workgroup filters a 42x42 LDS
// input tile = 32x32 outputs + the 11-tap window's halo), the tile load, the per-pixel expression of
// the zero-padded SSIM and the block sums. image_metrics' "ssim" is the loss's SSIM bit for bit because
// both translation units run the functions below between the same filter passes.
// The row and column passes stay written out in each kernel: as functions taking the window they moved
// the tap loads to the kernel's entry, which changed the generated code of all four kernels (k_ssim_fwd
// 156 -> 105 VGPRs) and the last bits of k_ssim_bwd's gradient (profiles/ssim_tile_resources.txt).
// tools/ssim_index_audit.cpp replays the index expressions of this file and of the kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace dgs {
namespace ssim {

constexpr int T = 32;            // output tile (32 x 32 pixels per 256-thread workgroup)
constexpr int R = 5;             // window radius
constexpr int S = T + 2 * R;     // 42: input tile with halo
constexpr int SP = S + 1;        // padded LDS row of the input tile
constexpr int HP = T + 1;        // padded LDS row of the row-filtered maps
constexpr int HX = 8;            // row pass: outputs per thread (one row, 8 columns: 168 items)
constexpr int VY = 4;            // column pass: outputs per thread (one column, 4 rows: 256 items)
constexpr float C1 = 0.01f * 0.01f;
constexpr float C2 = 0.03f * 0.03f;

struct Win {
    float w[11];
};
Win make_window();  // ssim.hip: the loss's taps

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// NM maps of the 42 x 42 input tile with origin (ox, oy) (zero outside the image) from `src` planes
// into LDS; with SUB, map q is stored minus sub[q]. Every load of the thread is issued before the first
// LDS store (unrolled: a rolled loop waited out one HBM round trip per 256 elements, 7 in a row)
template <int NM, bool SUB = false>
__device__ __forceinline__ void load_tile(float (*sm)[S][SP], const float *const src[NM], int H, int W, int ox,
                                          int oy, const float *sub = nullptr) {
    constexpr int NIT = (S * S + 255) / 256;
    float v[NIT][NM];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int e = threadIdx.x + 256 * it;
        const int ly = e / S, lx = e - ly * S;
        const int gy = oy + ly, gx = ox + lx;
        const bool in = e < S * S && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t p = in ? (size_t)gy * W + gx : 0;
#pragma unroll
        for (int q = 0; q < NM; q++) v[it][q] = in ? src[q][p] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int e = threadIdx.x + 256 * it;
        const int ly = e / S, lx = e - ly * S;
        if (e < S * S)
#pragma unroll
            for (int q = 0; q < NM; q++) sm[q][ly][lx] = SUB ? v[it][q] - sub[q] : v[it][q];
    }
}

// SSIM of one pixel of the zero-padded filter from its five filtered maps: sv = n1 n2 / (d1 d2), with
// the factors the loss's backward coefficients are built from. Every operation is rounded on its own
// (no contraction: mu1^2 + mu2^2 as fma(mu1, mu1, round(mu2^2)) is not 2 round(mu1 mu2)) and sv is one
// correctly rounded division of the two products, as the reference evaluates it, not n1 n2 inv: with
// identical inputs (and the kernels' five sums formed alike, by explicit fmaf) n1 == d1 and n2 == d2
// bit for bit, every pixel is exactly 1.0, the tile sums are exact and the mean SSIM is 1.0, as the
// reference's (tests/test_gpu_loss_parity.py, `identical`; it was 2-3 ulps below)
struct Pixel {
    float n1, n2, d1, d2, inv, sv;
};
__device__ __forceinline__ Pixel ssim_pixel(float mu1, float mu2, float e11, float e22, float e12) {
#pragma clang fp contract(off)
    const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
    const float s11 = e11 - mu1s, s22 = e22 - mu2s, s12 = e12 - mu12;
    Pixel p;
    p.n1 = 2.f * mu12 + C1, p.n2 = 2.f * s12 + C2;
    p.d1 = mu1s + mu2s + C1, p.d2 = s11 + s22 + C2;
    const float d12 = p.d1 * p.d2;
    p.inv = 1.f / d12;
    p.sv = (p.n1 * p.n2) / d12;
    return p;
}

// the workgroup's sums of (a, b) in a fixed order -> partial[2 * block], [2 * block + 1], block =
// (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x
__device__ __forceinline__ void tile_sums(float a, float b, float (*red)[4], float *__restrict__ partial) {
    const int tid = threadIdx.x;
    a = wave_sum(a);
    b = wave_sum(b);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = a;
        red[1][tid >> 6] = b;
    }
    __syncthreads();
    if (tid == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * blk] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[2 * blk + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

}  // namespace ssim
}  // namespace dgs
