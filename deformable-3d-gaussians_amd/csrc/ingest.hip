// Image ingest for the dataset reader (scene/dataset_readers.py:223-266 + utils/general_utils.py:23-29):
// PNG scanline unfiltering, the reader's alpha composite, PIL's default resize and the /255 float image, on
// the device. The host only parses chunks and inflates (zlib); the still-filtered scanlines of a batch of
// same-sized images arrive in one copy.
//
// k_unfilter: one wave per image, 64 rows in flight as a row-skewed pipeline. Lane l owns row r0 + l and at
// step s handles pixel x = s - l, so it trails the row above by exactly one pixel: what the lane above wrote
// in the previous step is this pixel's "up" neighbour b, and the b of the step before is its upper-left
// neighbour c. The hand-down is one lane shuffle per step (no LDS, no barrier: the wave runs in lock step).
// Bands of 64 rows follow one another; the last row of a band reaches lane 0 of the next band through a
// W-pixel LDS row, which lane 63 refills 63 pixels behind lane 0's reads. A pixel is one packed dword;
// None / Sub / Up / Average are byte-parallel integer tricks on it, Paeth is done per channel, and the
// filter type selects among the predictions without a branch, so rows of different types do not diverge.
// The raw bytes of the next 8 steps are loaded while the current 8 are computed (the recurrence, not the
// load, is then the critical path). Every address comes from (W, H, bpp) and the thread index; the only index
// taken from file content is (colour << 8 | alpha) into the 65536-byte composite table.
// k_resample: one pass of PIL's two-pass antialiased resize (ImagingResample*_8bpc): host-built bounds and
// 22-bit fixed-point coefficients, integer multiply-accumulate from 2^21, clip8(acc >> 22).
// k_to_float: (B,h,w,3) bytes -> (B,3,h,w) float32 = byte / 255 (Camera.original_image layout).
#include <hip/hip_runtime.h>

#include "dgs_common.h"

namespace dgs {

constexpr int INGEST_MAX_W = 8192;  // the band-to-band LDS row: 32 KiB
constexpr int INGEST_AHEAD = 8;     // pixels loaded ahead of the recurrence

__device__ inline uint32_t add_bytes(uint32_t x, uint32_t p) {
    return ((x & 0x7f7f7f7fu) + (p & 0x7f7f7f7fu)) ^ ((x ^ p) & 0x80808080u);
}

__device__ inline uint32_t avg_bytes(uint32_t a, uint32_t b) {  // floor((a + b) / 2) per byte
    return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1);
}

template <int BPP>
__device__ inline uint32_t paeth_bytes(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < BPP; k++) {
        const int ia = (a >> (8 * k)) & 255, ib = (b >> (8 * k)) & 255, ic = (c >> (8 * k)) & 255;
        const int pa = abs(ib - ic), pb = abs(ia - ic), pc = abs(ia + ib - 2 * ic);
        const int pr = (pa <= pb && pa <= pc) ? ia : (pb <= pc ? ib : ic);
        r |= (uint32_t)pr << (8 * k);
    }
    return r;
}

template <int BPP>
__device__ inline uint32_t load_px(const uint8_t *p) {
    if (BPP == 4) {
        uint32_t v;
        __builtin_memcpy(&v, p, 4);  // rows start at an odd offset (the filter byte): unaligned
        return v;
    }
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// scan: B x H x (1 + W*BPP) filtered bytes. out: B x H x W x OC bytes, OC = 3 when lut (BPP 4 only:
// composite over the background, alpha dropped) else BPP.
template <int BPP>
__global__ __launch_bounds__(64) void k_unfilter(int W, int H, const uint8_t *__restrict__ scan,
                                                 const uint8_t *__restrict__ lut, uint8_t *__restrict__ out) {
    __shared__ uint32_t carry[INGEST_MAX_W];
    const int lane = threadIdx.x;
    const size_t stride = 1 + (size_t)W * BPP;
    const uint8_t *src = scan + (size_t)blockIdx.x * H * stride;
    const bool comp = BPP == 4 && lut != nullptr;
    const int OC = comp ? 3 : BPP;
    uint8_t *dst = out + (size_t)blockIdx.x * H * W * OC;
    for (int x = lane; x < W; x += 64) carry[x] = 0;  // row 0 has a zero previous row
    __syncthreads();
    const int steps = W + 63;
    for (int r0 = 0; r0 < H; r0 += 64) {
        const int r = r0 + lane;
        const bool live = r < H;
        const uint8_t *row = src + (size_t)(live ? r : r0) * stride;
        const int ft = row[0];
        const uint8_t *px = row + 1;
        uint8_t *drow = dst + (size_t)(live ? r : r0) * W * OC;
        uint32_t a = 0, c = 0, cur = 0;
        uint32_t nxt[INGEST_AHEAD];
#pragma unroll
        for (int k = 0; k < INGEST_AHEAD; k++) nxt[k] = load_px<BPP>(px + (size_t)min(max(k - lane, 0), W - 1) * BPP);
        for (int s0 = 0; s0 < steps; s0 += INGEST_AHEAD) {
            uint32_t raw[INGEST_AHEAD];
#pragma unroll
            for (int k = 0; k < INGEST_AHEAD; k++) raw[k] = nxt[k];
#pragma unroll
            for (int k = 0; k < INGEST_AHEAD; k++)  // clamped: always a pixel of this lane's own row
                nxt[k] = load_px<BPP>(px + (size_t)min(max(s0 + INGEST_AHEAD + k - lane, 0), W - 1) * BPP);
#pragma unroll
            for (int k = 0; k < INGEST_AHEAD; k++) {
                const int s = s0 + k;
                // the lane above finished pixel x of its row in the previous step
                uint32_t b = __shfl_up(cur, 1);
                if (lane == 0) b = s < W ? carry[s] : 0u;
                const int x = s - lane;
                if (live && x >= 0 && x < W) {
                    const uint32_t avg = avg_bytes(a, b), pae = paeth_bytes<BPP>(a, b, c);
                    const uint32_t pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? avg : ft == 4 ? pae : 0u;
                    cur = add_bytes(raw[k], pred);
                    if (comp) {
                        const uint32_t al = cur >> 24;
                        uint8_t *o = drow + (size_t)x * 3;
                        o[0] = lut[((cur & 255u) << 8) | al];
                        o[1] = lut[(((cur >> 8) & 255u) << 8) | al];
                        o[2] = lut[(((cur >> 16) & 255u) << 8) | al];
                    } else if (BPP == 4) {
                        __builtin_memcpy(drow + (size_t)x * 4, &cur, 4);
                    } else {
                        uint8_t *o = drow + (size_t)x * 3;
                        o[0] = (uint8_t)cur;
                        o[1] = (uint8_t)(cur >> 8);
                        o[2] = (uint8_t)(cur >> 16);
                    }
                    a = cur;
                    c = b;
                    if (lane == 63) carry[x] = cur;  // 63 pixels behind lane 0's reads of this band
                }
            }
        }
        __syncthreads();
    }
}

// One resize pass along the middle axis: in (outer, n_in, inner) -> out (outer, n_out, inner) bytes.
// bounds: (n_out, 2) = first input index, tap count; coef: (n_out, ksize) 22-bit fixed point.
__global__ __launch_bounds__(256) void k_resample(long long total, int n_in, int n_out, int inner,
                                                  const uint8_t *__restrict__ in, const int *__restrict__ bounds,
                                                  const int *__restrict__ coef, int ksize, uint8_t *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int ii = (int)(t % inner);
    const int o = (int)((t / inner) % n_out);
    const long long ou = t / ((long long)inner * n_out);
    const int first = min(max(bounds[2 * o], 0), n_in);
    const int cnt = min(min(max(bounds[2 * o + 1], 0), ksize), n_in - first);
    const uint8_t *p = in + (ou * n_in + first) * inner + ii;
    const int *k = coef + (size_t)o * ksize;
    int acc = 1 << 21;
    for (int j = 0; j < cnt; j++) acc += (int)p[(size_t)j * inner] * k[j];
    out[t] = (uint8_t)min(max(acc >> 22, 0), 255);
}

__global__ __launch_bounds__(256) void k_to_float(long long total, int hw, const uint8_t *__restrict__ in,
                                                  float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long b = t / (3LL * hw);
    const int c = (int)((t / hw) % 3);
    const int p = (int)(t % hw);
    out[t] = (float)in[(b * hw + p) * 3 + c] / 255.0f;
}

}  // namespace dgs

static const long long INGEST_MAX_ELEMS = 2147483647LL * 256;

extern "C" int dgs_ingest_unfilter(int B, int W, int H, int bpp, const uint8_t *scanlines, const uint8_t *lut,
                                   uint8_t *out, void *stream_) {
    if (B < 0 || W < 1 || H < 1 || (bpp != 3 && bpp != 4) || (B > 0 && (!scanlines || !out)) || (lut && bpp != 4)) {
        dgs::set_error("dgs_ingest_unfilter: bad argument (bpp 3 or 4, a composite table only with bpp 4)");
        return DGS_ERR_ARGS;
    }
    if (W > dgs::INGEST_MAX_W) {
        dgs::set_error("dgs_ingest_unfilter: images wider than " + std::to_string(dgs::INGEST_MAX_W) + " pixels");
        return DGS_ERR_UNSUPPORTED;
    }
    if (B == 0) return DGS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (bpp == 4)
        hipLaunchKernelGGL(dgs::k_unfilter<4>, dim3(B), dim3(64), 0, stream, W, H, scanlines, lut, out);
    else
        hipLaunchKernelGGL(dgs::k_unfilter<3>, dim3(B), dim3(64), 0, stream, W, H, scanlines, lut, out);
    DGS_LAUNCH_CHECK("k_unfilter", false, stream);
    return DGS_OK;
}

extern "C" int dgs_ingest_resample(int64_t outer, int n_in, int n_out, int inner, const uint8_t *in,
                                   const int *bounds, const int *coef, int ksize, uint8_t *out, void *stream_) {
    if (outer < 0 || n_in < 1 || n_out < 1 || inner < 1 || ksize < 1 || !bounds || !coef ||
        (outer > 0 && (!in || !out))) {
        dgs::set_error("dgs_ingest_resample: bad argument");
        return DGS_ERR_ARGS;
    }
    const long long total = (long long)outer * n_out * inner;
    if (total > INGEST_MAX_ELEMS) {
        dgs::set_error("dgs_ingest_resample: batch too large for one launch");
        return DGS_ERR_UNSUPPORTED;
    }
    if (total == 0) return DGS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(dgs::k_resample, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, n_in, n_out,
                       inner, in, bounds, coef, ksize, out);
    DGS_LAUNCH_CHECK("k_resample", false, stream);
    return DGS_OK;
}

extern "C" int dgs_ingest_to_float(int B, int H, int W, const uint8_t *rgb8, float *out, void *stream_) {
    if (B < 0 || H < 1 || W < 1 || (B > 0 && (!rgb8 || !out))) {
        dgs::set_error("dgs_ingest_to_float: bad argument");
        return DGS_ERR_ARGS;
    }
    const long long total = 3LL * B * H * W;
    if (total > INGEST_MAX_ELEMS) {
        dgs::set_error("dgs_ingest_to_float: batch too large for one launch");
        return DGS_ERR_UNSUPPORTED;
    }
    if (total == 0) return DGS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(dgs::k_to_float, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, H * W, rgb8,
                       out);
    DGS_LAUNCH_CHECK("k_to_float", false, stream);
    return DGS_OK;
}
