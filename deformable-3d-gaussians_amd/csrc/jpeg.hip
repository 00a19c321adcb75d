// Baseline JPEG ingest for the dataset reader: the host front end (jpeg_decode.h: markers + Huffman decoding
// down to quantised coefficients) behind two C entries, and the per-pixel rest on the device, reproducing
// libjpeg-turbo's default decompressor (what PIL's Image.open gives) in integers, bit for bit:
//
// k_jpeg_idct: dequantise + the "islow" 8x8 inverse DCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2). Its FIX_*
// constants and its layout (eight lanes per block, padded LDS rows) are jpeg_tables.h's, shared with
// k_jpeg_transform of jpeg_encode.hip. A lane loads one row of coefficients and of the quantisation table (16
// bytes each: a wave reads 1 KiB of coefficients contiguously), writes the products to LDS, takes a column back
// for pass 1, writes the workspace, takes a row back for pass 2 and stores its 8 output bytes as one 8-byte
// word into the component's block-padded sample plane. The arithmetic wraps in 32 bits (unsigned adds and multiplies, an arithmetic shift of the int): on any file libjpeg decodes
// without overflow this is its result, and on hostile coefficients it is defined and equals
// deformgs/jpeg.py. The zero-AC shortcuts of jidctint.c give the numbers of the full path: no branch.
// Output: clamp(s + 128, 0, 255) with s the descaled value as a signed 10-bit number, the effect of
// libjpeg's wrap-around range-limit table.
//
// k_jpeg_color: one pixel per thread: the luma sample, the two chroma samples through jdsample.c's fancy
// upsampling (h2v1: 3:1 taps along the row; h2v2: 3:1 column sums of the near and the far row, then 3:1
// along the row, with its +8 / +7 rounding pair; a downsampled width <= 2 takes plain doubling; the row
// above the first and below the last real chroma row, ceil(H/2) - 1, is that row itself; no column at or
// past the downsampled width is read), then jdcolor.c's 16-bit fixed-point YCbCr -> RGB. Lanes write
// adjacent 3-byte pixels: (B, H, W, 3) bytes, the layout k_resample and k_to_float consume.
//
// Every address comes from (B, W, H, hs, vs) and the thread index; no index is taken from file content.
// Traffic per pixel at 4:2:0: 3 bytes of coefficients + 1.5 of planes written (k_jpeg_idct), then 1 luma +
// up to 8 chroma bytes read, mostly from cache (each chroma byte is shared by up to 16 pixels; 1.5 bytes per
// pixel reach memory once) + 3 written (k_jpeg_color): about 3 in, 3 out, and the planes once each way.
#include <hip/hip_runtime.h>

#include "dgs_common.h"
#include "jpeg_decode.h"

static_assert(sizeof(dgs_jpeg_info) == sizeof(dgs_jpeg::Info), "dgs_jpeg_info and dgs_jpeg::Info must agree");
static_assert(offsetof(dgs_jpeg_info, qt) == offsetof(dgs_jpeg::Info, qt), "dgs_jpeg_info layout");

namespace dgs {

using dgs_jpeg::LDS_ROW;
using dgs_jpeg::WG_BLOCKS;
constexpr int LDS_BLOCK = 8 * LDS_ROW;  // dwords between two blocks in LDS

// One 8-point pass of jpeg_idct_islow; the sums wrap in 32 bits, the descale is an arithmetic shift.
template <int SHIFT>
__device__ inline void idct8(const int (&in)[8], int (&out)[8]) {
    using namespace dgs_jpeg;  // FIX_*
    typedef uint32_t u;
    const u x0 = (u)in[0], x1 = (u)in[1], x2 = (u)in[2], x3 = (u)in[3], x4 = (u)in[4], x5 = (u)in[5], x6 = (u)in[6],
            x7 = (u)in[7];
    u z1 = (x2 + x6) * (u)FIX_0_541196100;
    const u e2 = z1 - x6 * (u)FIX_1_847759065;
    const u e3 = z1 + x2 * (u)FIX_0_765366865;
    const u e0 = (x0 + x4) << 13, e1 = (x0 - x4) << 13;
    const u t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    u t0 = x7, t1 = x5, t2 = x3, t3 = x1;
    z1 = t0 + t3;
    u z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const u z5 = (z3 + z4) * (u)FIX_1_175875602;
    t0 *= (u)FIX_0_298631336;
    t1 *= (u)FIX_2_053119869;
    t2 *= (u)FIX_3_072711026;
    t3 *= (u)FIX_1_501321110;
    z1 = 0u - z1 * (u)FIX_0_899976223;
    z2 = 0u - z2 * (u)FIX_2_562915447;
    z3 = z5 - z3 * (u)FIX_1_961570560;
    z4 = z5 - z4 * (u)FIX_0_390180644;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const u r = 1u << (SHIFT - 1);
    out[0] = (int)(t10 + t3 + r) >> SHIFT;
    out[7] = (int)(t10 - t3 + r) >> SHIFT;
    out[1] = (int)(t11 + t2 + r) >> SHIFT;
    out[6] = (int)(t11 - t2 + r) >> SHIFT;
    out[2] = (int)(t12 + t1 + r) >> SHIFT;
    out[5] = (int)(t12 - t1 + r) >> SHIFT;
    out[3] = (int)(t13 + t0 + r) >> SHIFT;
    out[4] = (int)(t13 - t0 + r) >> SHIFT;
}

// coef: per image [Y blocks | Cb blocks | Cr blocks] x 64 int16, natural order, block-row-major.
// qt: (B, 3, 64) uint16. planes: per image [Y | Cb | Cr] sample planes of (blocks_h * 8) x (blocks_w * 8) bytes.
__global__ __launch_bounds__(256) void k_jpeg_idct(long long total_blocks, int per_image, int nbY, int nbC, int bwY,
                                                   int bwC, const int16_t *__restrict__ coef,
                                                   const uint16_t *__restrict__ qt, uint8_t *__restrict__ planes) {
    __shared__ int lds[WG_BLOCKS * LDS_BLOCK];
    const int lb = threadIdx.x >> 3, l = threadIdx.x & 7;
    long long g = (long long)blockIdx.x * WG_BLOCKS + lb;
    const bool live = g < total_blocks;
    if (!live) g = total_blocks - 1;  // clamped: the loads stay inside the buffers, nothing is stored
    const long long img = g / per_image;
    const int r = (int)(g % per_image);
    const int c = r < nbY ? 0 : (r < nbY + nbC ? 1 : 2);
    const int first = c == 0 ? 0 : (c == 1 ? nbY : nbY + nbC);
    const int bw = c == 0 ? bwY : bwC;
    const int by = (r - first) / bw, bx = (r - first) % bw;
    const int4 cv = *reinterpret_cast<const int4 *>(coef + g * 64 + l * 8);
    const int4 qv = *reinterpret_cast<const int4 *>(qt + (img * 3 + c) * 64 + l * 8);
    const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
    int *blk = lds + lb * LDS_BLOCK;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        blk[l * LDS_ROW + 2 * j] = (int)((uint32_t)(int)(int16_t)(cw[j] & 0xffff) * ((uint32_t)qw[j] & 0xffffu));
        blk[l * LDS_ROW + 2 * j + 1] = (int)((uint32_t)(cw[j] >> 16) * ((uint32_t)qw[j] >> 16));
    }
    __syncthreads();
    int x[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = blk[k * LDS_ROW + l];  // column l
    idct8<13 - 2>(x, o);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) blk[k * LDS_ROW + l] = o[k];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = blk[l * LDS_ROW + j];  // row l
    idct8<13 + 2 + 3>(x, o);
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int s = ((o[j] & 1023) ^ 512) - 512;  // signed 10 bits: the wrap-around range-limit table
        w[j >> 2] |= (uint32_t)min(max(s + 128, 0), 255) << (8 * (j & 3));
    }
    if (live) {
        uint8_t *plane = planes + (size_t)img * per_image * 64 + (size_t)first * 64;
        *reinterpret_cast<uint2 *>(plane + ((size_t)by * 8 + l) * ((size_t)bw * 8) + (size_t)bx * 8) = make_uint2(w[0], w[1]);
    }
}

// One upsampled chroma sample at (x, y). p: the block-padded plane, pw its row pitch; cw x ch its real size.
__device__ inline int chroma_at(const uint8_t *__restrict__ p, size_t pw, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pw + x];
    const int i = x >> 1;
    if (vs == 1) {
        const uint8_t *row = p + (size_t)y * pw;
        const int v = row[i];
        if (cw <= 2) return v;
        if (x & 1) return i == cw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
        return i == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
    }
    const int j = y >> 1;
    const uint8_t *near = p + (size_t)j * pw;
    if (cw <= 2) return near[i];
    const int jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const uint8_t *far = p + (size_t)jf * pw;
    const int cur = 3 * near[i] + far[i];
    if (x & 1) {
        if (i == cw - 1) return (4 * cur + 7) >> 4;
        return (3 * cur + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    }
    if (i == 0) return (4 * cur + 8) >> 4;
    return (3 * cur + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void k_jpeg_color(long long total, int W, int H, int hs, int vs, size_t image_bytes,
                                                    size_t pwY, size_t pwC, size_t off_cb, size_t off_cr,
                                                    const uint8_t *__restrict__ planes, uint8_t *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int x = (int)(t % W);
    const int y = (int)((t / W) % H);
    const long long b = t / ((long long)W * H);
    const uint8_t *base = planes + (size_t)b * image_bytes;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const int Y = base[(size_t)y * pwY + x];
    const int cb = chroma_at(base + off_cb, pwC, cw, ch, hs, vs, x, y) - 128;
    const int cr = chroma_at(base + off_cr, pwC, cw, ch, hs, vs, x, y) - 128;
    // jdcolor.c: FIX(x) = int(x * 65536 + 0.5)
    const int R = Y + ((91881 * cr + 32768) >> 16);
    const int Bl = Y + ((116130 * cb + 32768) >> 16);
    const int G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    uint8_t *o = out + (size_t)t * 3;
    o[0] = (uint8_t)min(max(R, 0), 255);
    o[1] = (uint8_t)min(max(G, 0), 255);
    o[2] = (uint8_t)min(max(Bl, 0), 255);
}

}  // namespace dgs

extern "C" int dgs_jpeg_header(const uint8_t *bytes, size_t len, dgs_jpeg_info *info, char *err, size_t err_len) {
    return dgs_jpeg::header(bytes, len, reinterpret_cast<dgs_jpeg::Info *>(info), err, err_len);
}

extern "C" int dgs_jpeg_coefficients(const uint8_t *bytes, size_t len, const dgs_jpeg_info *info, int16_t *out,
                                     size_t capacity, char *err, size_t err_len) {
    return dgs_jpeg::coefficients(bytes, len, reinterpret_cast<const dgs_jpeg::Info *>(info), out, capacity, err, err_len);
}

extern "C" int dgs_ingest_jpeg(int B, int W, int H, int hs, int vs, const int16_t *coef, const uint16_t *qtables,
                               uint8_t *rgb8_out, uint8_t *scratch, void *stream_) {
    const bool layout = (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2);
    if (B < 0 || W < 1 || H < 1 || W > dgs_jpeg::MAX_DIM || H > dgs_jpeg::MAX_DIM || !layout ||
        (B > 0 && (!coef || !qtables || !rgb8_out || !scratch)) || (reinterpret_cast<uintptr_t>(coef) & 15) ||
        (reinterpret_cast<uintptr_t>(qtables) & 15) || (reinterpret_cast<uintptr_t>(scratch) & 7)) {
        dgs::set_error("dgs_ingest_jpeg: bad argument (sampling 1x1, 2x1 or 2x2; coef and qtables 16-byte aligned, "
                       "scratch 8-byte aligned)");
        return DGS_ERR_ARGS;
    }
    if (B == 0) return DGS_OK;
    const int mw = (W + 8 * hs - 1) / (8 * hs), mh = (H + 8 * vs - 1) / (8 * vs);
    const int bwY = mw * hs, bhY = mh * vs, bwC = mw, bhC = mh;
    const long long nbY = (long long)bwY * bhY, nbC = (long long)bwC * bhC, per_image = nbY + 2 * nbC;
    const long long total_blocks = per_image * B, total_px = (long long)B * W * H;
    if (per_image > 2147483647LL || total_blocks > 2147483647LL * dgs::WG_BLOCKS || total_px > 2147483647LL * 256) {
        dgs::set_error("dgs_ingest_jpeg: batch too large for one launch");
        return DGS_ERR_UNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(dgs::k_jpeg_idct, dim3((unsigned)((total_blocks + dgs::WG_BLOCKS - 1) / dgs::WG_BLOCKS)),
                       dim3(256), 0, stream, total_blocks, (int)per_image, (int)nbY, (int)nbC, bwY, bwC, coef, qtables,
                       scratch);
    DGS_LAUNCH_CHECK("k_jpeg_idct", false, stream);
    hipLaunchKernelGGL(dgs::k_jpeg_color, dim3((unsigned)((total_px + 255) / 256)), dim3(256), 0, stream, total_px, W, H, hs,
                       vs, (size_t)per_image * 64, (size_t)bwY * 8, (size_t)bwC * 8, (size_t)nbY * 64,
                       (size_t)(nbY + nbC) * 64, (const uint8_t *)scratch, rgb8_out);
    DGS_LAUNCH_CHECK("k_jpeg_color", false, stream);
    return DGS_OK;
}
