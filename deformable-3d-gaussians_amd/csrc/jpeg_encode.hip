// Batched baseline JPEG encoding on the device, the inverse of jpeg.hip: F uint8 frames (F,H,W,3) RGB -> per frame
// the entropy-coded data of one interleaved YCbCr scan at 4:4:4, 4:2:2 or 4:2:0 with a restart interval of one MCU
// row, packed back to back. The host adds the markers around it (deformgs/jpeg_gpu.py). The arithmetic is
// libjpeg-turbo's default compressor in integers (tests/jpeg_encode_ref.py is the numpy restatement). Four launches on
// one stream, no host wait, no floating point, no atomics to global memory: the bytes are bitwise reproducible.
//
//   k_jpeg_transform  eight lanes per 8x8 block (jpeg_tables.h: k_jpeg_idct's layout). Lane r converts row r to its
//                     component (jccolor.c in 16-bit fixed point; chroma of a subsampled frame is the h2v1 / h2v2 box
//                     of jcsample.c with the 0,1 / 1,2 alternating bias, pixel coordinates clamped to the image, rows
//                     past the component's height taking its last row), level-shifts and runs the row pass of
//                     jfdctint.c; after a transpose through LDS lane c runs the column pass and quantises against
//                     qtable << 3, half away from zero. int16 coefficients go to scratch in the layout of
//                     dgs_jpeg_coefficients. A block that exists only to fill an MCU (jccoefct.c's dummy block) is
//                     computed from the block whose DC it repeats, and its AC zeroed.
//   k_jpeg_entropy    one workgroup per restart segment = MCU row, one thread per block, JE_NT blocks at a time:
//                     the blocks' coefficients are staged in LDS in zigzag order, each thread counts its block's
//                     bits, a prefix scan gives the bit offsets, the bits are ORed into an LDS image (codec_bits.h's
//                     scan and bit writer, most significant bit first), and the whole bytes of the image are counted for 0xFF, scanned and,
//                     in the second launch, scattered with their stuffed 0x00. The bits of a byte that is not yet
//                     whole carry into the next round; the last byte is padded with ones. First launch (WRITE =
//                     false): the segment's stuffed byte count. Second launch: the bytes, at their final place.
//   k_jpeg_scan       exclusive prefix sum of the segments' byte counts (+ 2 for the RSTm after all but a frame's
//                     last; codec_bits.h segment_offsets), the frames' offsets and true lengths, and the flag of a frame that does not fit.
// Running the entropy coder twice costs its time again but needs no slot per segment sized for the worst case (208
// bytes a block before stuffing: 10 bytes a pixel at 4:4:4), which is what the capacity argument is there to avoid.
#include "codec_bits.h"
#include "dgs_common.h"
#include "jpeg_tables.h"

namespace dgs {
namespace {

using dgs_jpeg::LDS_ROW;
using dgs_jpeg::WG_BLOCKS;

constexpr int JE_NT = 128;                      // threads = blocks per round of k_jpeg_entropy
constexpr int JE_CSTRIDE = 66;                   // int16 per staged block: 33 words, odd, so lanes hit distinct banks
constexpr int JE_BLOCK_BITS = 20 + 63 * 26;      // DC: 9 + 11 bits; AC: 16 + 10 bits each
constexpr int JE_IMG_WORDS = (JE_NT * JE_BLOCK_BITS + 7 + 31) / 32 + 1;
constexpr long long JE_MAX_SEGMENTS = 1ll << 22;
constexpr int JE_MAX_DIM = 65535;                // the SOF0 field

// ITU-T T.81 Annex K.3: codes per length 1..16, then the symbols in code order. DC luma, DC chroma, AC luma, AC chroma.
__constant__ uint8_t HUFF_BITS[4][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
__constant__ uint8_t HUFF_AC_LUMA[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
__constant__ uint8_t HUFF_AC_CHROMA[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

__constant__ uint8_t JE_ZIGZAG[64] = {DGS_JPEG_ZIGZAG_ORDER};

struct QTables {
    uint16_t q[2][64];
};

// The frame's geometry, the same for every kernel.
struct Geo {
    int F, H, W, hs, vs;
    int mw, mh;          // MCUs
    int bw[3], bh[3];    // block grid per component, padded to whole MCUs
    int wib[3], hib[3];  // the component's own size in blocks: what is computed from pixels
    int base[3];         // first block of the component in a frame's coefficient buffer
    int total;           // blocks per frame
};

// ---- transform ----

// jccolor.c: FIX(x) = x * 65536 + 0.5
__device__ inline void ycc(const uint8_t *p, int &y, int &cb, int &cr) {
    const int r = p[0], g = p[1], b = p[2];
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one 8-point pass. FIRST: the row pass (results scaled up by 4); else the column pass.
template <bool FIRST>
__device__ inline void fdct8(int *d) {
    using namespace dgs_jpeg;  // FIX_*
    constexpr int SH = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << 2;
        d[4] = (t10 - t11) << 2;
    } else {
        d[0] = descale(t10 + t11, 2);
        d[4] = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * FIX_0_541196100;
    d[2] = descale(z1 + t13 * FIX_0_765366865, SH);
    d[6] = descale(z1 - t12 * FIX_1_847759065, SH);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    const int a4 = t4 * FIX_0_298631336, a5 = t5 * FIX_2_053119869, a6 = t6 * FIX_3_072711026, a7 = t7 * FIX_1_501321110;
    z1 *= -FIX_0_899976223;
    z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5;
    z4 = z4 * -FIX_0_390180644 + z5;
    d[7] = descale(a4 + z1 + z3, SH);
    d[5] = descale(a5 + z2 + z4, SH);
    d[3] = descale(a6 + z2 + z3, SH);
    d[1] = descale(a7 + z1 + z4, SH);
}

__global__ __launch_bounds__(256) void k_jpeg_transform(Geo g, QTables qt, const uint8_t *in, int16_t *coef) {
    __shared__ int ws[WG_BLOCKS][8][LDS_ROW];
    __shared__ __attribute__((aligned(16))) int16_t qs[WG_BLOCKS][64];
    const int t = threadIdx.x, slot = t >> 3, r = t & 7;
    const long long n_blocks = (long long)g.F * g.total;
    long long id = (long long)blockIdx.x * WG_BLOCKS + slot;
    const bool live = id < n_blocks;
    if (!live) id = n_blocks - 1;
    const int f = (int)(id / g.total);
    const int k = (int)(id - (long long)f * g.total);
    const int c = k >= g.base[2] ? 2 : (k >= g.base[1] ? 1 : 0);
    const int by = (k - g.base[c]) / g.bw[c], bx = (k - g.base[c]) - by * g.bw[c];
    // a dummy block repeats the DC of the block before it in the MCU's order: to the right of the component, the
    // last real block of its row; below it, the last block of the MCU's row above, itself real or a repeat
    const bool dummy = by >= g.hib[c] || bx >= g.wib[c];
    int sx = bx, sy = by;
    if (by >= g.hib[c]) {
        sy = g.hib[c] - 1;
        sx = (bx / g.hs) * g.hs + g.hs - 1;
    }
    sx = min(sx, g.wib[c] - 1);
    const uint8_t *img = in + (size_t)f * g.H * g.W * 3;
    int d[8];
    if (c == 0 || g.hs == 1) {
        const uint8_t *row = img + (size_t)min(sy * 8 + r, g.H - 1) * g.W * 3;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int y, cb, cr;
            ycc(row + (size_t)min(sx * 8 + x, g.W - 1) * 3, y, cb, cr);
            d[x] = (c == 0 ? y : (c == 1 ? cb : cr)) - 128;
        }
    } else {
        const int ch = (g.H + g.vs - 1) / g.vs;  // rows of the component
        const int cy = min(sy * 8 + r, ch - 1);
        const uint8_t *row0 = img + (size_t)min(cy * g.vs, g.H - 1) * g.W * 3;
        const uint8_t *row1 = img + (size_t)min(cy * g.vs + 1, g.H - 1) * g.W * 3;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int cx = sx * 8 + x;
            const size_t x0 = (size_t)min(2 * cx, g.W - 1) * 3, x1 = (size_t)min(2 * cx + 1, g.W - 1) * 3;
            int y, cb, cr, s;
            ycc(row0 + x0, y, cb, cr);
            s = c == 1 ? cb : cr;
            ycc(row0 + x1, y, cb, cr);
            s += c == 1 ? cb : cr;
            if (g.vs == 2) {
                ycc(row1 + x0, y, cb, cr);
                s += c == 1 ? cb : cr;
                ycc(row1 + x1, y, cb, cr);
                s += c == 1 ? cb : cr;
                s = (s + 1 + (x & 1)) >> 2;
            } else {
                s = (s + (x & 1)) >> 1;
            }
            d[x] = s - 128;
        }
    }
    fdct8<true>(d);
#pragma unroll
    for (int x = 0; x < 8; ++x) ws[slot][r][x] = d[x];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 8; ++y) d[y] = ws[slot][y][r];
    fdct8<false>(d);
    const uint16_t *q = qt.q[c ? 1 : 0];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const unsigned qv = (unsigned)q[y * 8 + r] << 3;
        const int v = d[y];
        const unsigned m = ((unsigned)abs(v) + (qv >> 1)) / qv;
        int o = v < 0 ? -(int)m : (int)m;
        if (dummy && (y | r)) o = 0;
        qs[slot][y * 8 + r] = (int16_t)o;
    }
    __syncthreads();
    if (live) *(uint4 *)(coef + id * 64 + r * 8) = *(const uint4 *)&qs[slot][r * 8];
}

// ---- entropy ----

using BitWriter = codec::BitWriter<true>;  // put: <= 16 + 10 = 26 bits

__device__ inline int bit_length(int a) { return 32 - __clz(a); }  // a >= 0; 0 -> 0

// One block through jchuff.c's encode_one_block; put(code word, length) sees every code and every value.
template <class Put>
__device__ inline void code_block(const int16_t *zz, int pred, const unsigned *dc, const unsigned *ac, Put put) {
    const int diff = (int)zz[0] - pred;
    int s = bit_length(abs(diff));
    put(dc[s] & 0xFFFFu, (int)(dc[s] >> 16));
    if (s) put((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
            run -= 16;
        }
        s = bit_length(abs(v));
        const unsigned cw = ac[(run << 4) | s];
        // the code and the value in one piece: 16 + 10 bits at the most
        put(((cw & 0xFFFFu) << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), (int)(cw >> 16) + s);
        run = 0;
    }
    if (run) put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

__device__ inline unsigned img_byte(const unsigned *img, unsigned i) { return (img[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

template <bool WRITE>
__global__ __launch_bounds__(JE_NT) void k_jpeg_entropy(Geo g, const int16_t *coef, unsigned *seg_bytes,
                                                        const unsigned long long *seg_off, uint8_t *out,
                                                        unsigned long long capacity) {
    __shared__ unsigned img[JE_IMG_WORDS];
    __shared__ __attribute__((aligned(4))) int16_t zz[JE_NT * JE_CSTRIDE];
    __shared__ unsigned lut[2 * 16 + 2 * 256];  // (length << 16) | code: DC luma, DC chroma, AC luma, AC chroma
    __shared__ unsigned sc[JE_NT];
    const int t = threadIdx.x;
    const long long seg = blockIdx.x;
    const int f = (int)(seg / g.mh), my = (int)(seg - (long long)f * g.mh);
    unsigned long long dst = 0;
    if (WRITE) {
        // a frame that does not fit whole is not written at all
        if (seg_off[(long long)(f + 1) * g.mh] > capacity) return;
        dst = seg_off[seg];
    }
    for (int i = t; i < 2 * 16 + 2 * 256; i += JE_NT) lut[i] = 0;
    __syncthreads();
    if (t < 4) {
        unsigned *tab = lut + (t < 2 ? 16 * t : 32 + 256 * (t - 2));
        const uint8_t *sym = t == 2 ? HUFF_AC_LUMA : HUFF_AC_CHROMA;
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < HUFF_BITS[t][len - 1]; ++i, ++k, ++code) tab[t < 2 ? k : sym[k]] = ((unsigned)len << 16) | code;
            code <<= 1;
        }
    }
    const int per_mcu = g.hs * g.vs + 2;
    const int n_blk = g.mw * per_mcu;
    const int16_t *fc = coef + (size_t)f * g.total * 64;
    unsigned carry_bits = 0, carry_val = 0;  // the bits of the byte that is not whole yet (uniform)
    unsigned long long written = 0;          // stuffed bytes of this segment so far (uniform)
    for (int b0 = 0; b0 < n_blk; b0 += JE_NT) {
        const int nb = min(JE_NT, n_blk - b0);
        const bool last_round = b0 + JE_NT >= n_blk;
        __syncthreads();  // the image and the staged blocks of the round before are read out
        // where thread t's block lies in the frame's coefficient buffer, and the block whose DC it predicts from
        int blk = -1, prev = -1, c = 0;
        if (t < nb) {
            const int i = b0 + t, mx = i / per_mcu, k = i - mx * per_mcu, nl = g.hs * g.vs;
            if (k < nl) {
                const int v = k / g.hs, h = k - v * g.hs;
                blk = (my * g.vs + v) * g.bw[0] + mx * g.hs + h;
                if (k > 0) {
                    const int pv = (k - 1) / g.hs, ph = (k - 1) - pv * g.hs;
                    prev = (my * g.vs + pv) * g.bw[0] + mx * g.hs + ph;
                } else if (mx > 0) {
                    prev = (my * g.vs + g.vs - 1) * g.bw[0] + mx * g.hs - 1;
                }
            } else {
                c = k - nl + 1;
                blk = g.base[c] + my * g.bw[c] + mx;
                if (mx > 0) prev = blk - 1;
            }
        }
        sc[t] = (unsigned)blk;
        for (int i = t; i < JE_IMG_WORDS; i += JE_NT) img[i] = 0;
        __syncthreads();
        for (int e = t; e < nb * 64; e += JE_NT) {  // 64 consecutive lanes read one block
            const int b = e >> 6, k = e & 63;
            zz[b * JE_CSTRIDE + k] = fc[(size_t)sc[b] * 64 + JE_ZIGZAG[k]];
        }
        __syncthreads();
        const unsigned *dc = lut + (c ? 16 : 0), *ac = lut + 32 + (c ? 256 : 0);
        const int pred = prev >= 0 ? (int)fc[(size_t)prev * 64] : 0;
        unsigned bits = 0;
        if (t < nb) code_block(zz + t * JE_CSTRIDE, pred, dc, ac, [&](unsigned, int n) { bits += (unsigned)n; });
        const unsigned incl = codec::block_scan<JE_NT>(bits, sc, t);
        unsigned total = carry_bits + sc[JE_NT - 1];
        if (t == 0 && carry_bits) atomicOr(&img[0], carry_val << (32 - carry_bits));
        if (t < nb) {
            BitWriter bw(img, carry_bits + incl - bits);
            code_block(zz + t * JE_CSTRIDE, pred, dc, ac, [&](unsigned v, int n) { bw.put(v, n); });
            bw.flush();
        }
        if (last_round && t == 0 && (total & 7)) {  // pad the last byte with ones
            const unsigned n = 8 - (total & 7);
            BitWriter bw(img, total);
            bw.put((1u << n) - 1, (int)n);
            bw.flush();
        }
        if (last_round) total = (total + 7) & ~7u;
        __syncthreads();
        // the whole bytes: thread t takes bytes [lo, hi), counts its 0xFF, and after the scan writes them stuffed
        const unsigned nbytes = total >> 3;
        const unsigned per = (nbytes + JE_NT - 1) / JE_NT;
        const unsigned lo = min(nbytes, (unsigned)t * per), hi = min(nbytes, lo + per);
        unsigned ff = 0;
        for (unsigned i = lo; i < hi; ++i) ff += img_byte(img, i) == 255u;
        const unsigned ff_incl = codec::block_scan<JE_NT>(ff, sc, t);
        if (WRITE) {
            uint8_t *o = out + dst + written + lo + (ff_incl - ff);
            for (unsigned i = lo; i < hi; ++i) {
                const unsigned v = img_byte(img, i);
                *o++ = (uint8_t)v;
                if (v == 255u) *o++ = 0;
            }
        }
        written += nbytes + sc[JE_NT - 1];
        carry_bits = total & 7;
        carry_val = carry_bits ? img_byte(img, nbytes) >> (8 - carry_bits) : 0u;
    }
    if (t == 0) {
        if (WRITE) {
            if (my < g.mh - 1) {
                out[dst + written] = 0xFF;
                out[dst + written + 1] = (uint8_t)(0xD0 + (my & 7));
            }
        } else {
            seg_bytes[seg] = (unsigned)written;
        }
    }
}

// seg_off[i] (G + 1 entries): where segment i starts in out, an RSTm (2 bytes) counted behind every segment but a
// frame's last. One workgroup.
__global__ __launch_bounds__(1024) void k_jpeg_scan(long long G, int mh, int F, const unsigned *seg_bytes,
                                                    unsigned long long *seg_off, unsigned long long capacity,
                                                    int64_t *out_offsets, int64_t *out_lengths, int *flags) {
    __shared__ unsigned long long part[1024];
    const int t = threadIdx.x;
    const unsigned long long total = codec::segment_offsets(
        G, [&](long long i) { return seg_bytes[i] + ((i % mh) != mh - 1 ? 2u : 0u); }, seg_off, part);
    if (t == 1023) seg_off[G] = total;
    __syncthreads();  // one workgroup: its global writes are visible to it behind the barrier
    for (int f = t; f < F; f += 1024) {
        const unsigned long long a = seg_off[(long long)f * mh], b = seg_off[(long long)(f + 1) * mh];
        out_offsets[f] = (int64_t)a;
        out_lengths[f] = (int64_t)(b - a);
        flags[f] = b > capacity;
    }
}

bool jpeg_geo(int F, int H, int W, int hs, int vs, Geo &g) {
    if (F < 1 || H < 1 || W < 1 || H > JE_MAX_DIM || W > JE_MAX_DIM) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    g.F = F, g.H = H, g.W = W, g.hs = hs, g.vs = vs;
    g.mw = (W + 8 * hs - 1) / (8 * hs);
    g.mh = (H + 8 * vs - 1) / (8 * vs);
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    long long total = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = g.mw * (c ? 1 : hs);
        g.bh[c] = g.mh * (c ? 1 : vs);
        g.wib[c] = ((c ? cw : W) + 7) / 8;
        g.hib[c] = ((c ? ch : H) + 7) / 8;
        g.base[c] = (int)total;
        total += (long long)g.bw[c] * g.bh[c];
    }
    g.total = (int)total;  // <= 3 * 8192 * 8192
    return true;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace
}  // namespace dgs

extern "C" size_t dgs_jpeg_encode_scratch_bytes(int F, int H, int W, int hs, int vs) {
    dgs::Geo g;
    if (!dgs::jpeg_geo(F, H, W, hs, vs, g)) return 0;
    const size_t G = (size_t)F * g.mh;
    return dgs::align16((size_t)F * g.total * 64 * sizeof(int16_t)) + dgs::align16(G * sizeof(unsigned)) +
           dgs::align16((G + 1) * sizeof(unsigned long long));
}

extern "C" int dgs_jpeg_encode(int F, int H, int W, int hs, int vs, const uint8_t *in, const uint16_t *qtables,
                               uint8_t *out, size_t out_capacity, int64_t *out_offsets, int64_t *out_lengths,
                               int *out_flags, uint8_t *scratch, void *stream_) {
    dgs::Geo g;
    bool ok = dgs::jpeg_geo(F, H, W, hs, vs, g) && in && qtables && out && out_offsets && out_lengths && out_flags &&
              scratch && !((uintptr_t)scratch & 15);
    dgs::QTables qt;
    for (int i = 0; ok && i < 128; ++i) {
        qt.q[i >> 6][i & 63] = qtables[i];
        ok = qtables[i] != 0;
    }
    if (!ok) {
        dgs::set_error("dgs_jpeg_encode: bad argument (F >= 1, H and W in 1..65535, sampling 1x1, 2x1 or 2x2, no zero "
                       "in a quantisation table, scratch 16-byte aligned)");
        return DGS_ERR_ARGS;
    }
    const long long G = (long long)F * g.mh;
    const long long n_blocks = (long long)F * g.total;
    const long long n_wg = (n_blocks + dgs_jpeg::WG_BLOCKS - 1) / dgs_jpeg::WG_BLOCKS;
    if (G > dgs::JE_MAX_SEGMENTS || n_wg > 0x7fffffffll) {
        dgs::set_error("dgs_jpeg_encode: batch too large for one launch (encode it in chunks)");
        return DGS_ERR_UNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    int16_t *coef = (int16_t *)scratch;
    unsigned *seg_bytes = (unsigned *)(scratch + dgs::align16((size_t)n_blocks * 64 * sizeof(int16_t)));
    unsigned long long *seg_off = (unsigned long long *)((uint8_t *)seg_bytes + dgs::align16((size_t)G * sizeof(unsigned)));
    const unsigned long long cap = out_capacity;
    hipLaunchKernelGGL(dgs::k_jpeg_transform, dim3((unsigned)n_wg), dim3(256), 0, stream, g, qt, in, coef);
    DGS_LAUNCH_CHECK("k_jpeg_transform", false, stream);
    hipLaunchKernelGGL(dgs::k_jpeg_entropy<false>, dim3((unsigned)G), dim3(dgs::JE_NT), 0, stream, g, (const int16_t *)coef,
                       seg_bytes, (const unsigned long long *)seg_off, out, cap);
    DGS_LAUNCH_CHECK("k_jpeg_entropy<count>", false, stream);
    hipLaunchKernelGGL(dgs::k_jpeg_scan, dim3(1), dim3(1024), 0, stream, G, g.mh, F, (const unsigned *)seg_bytes, seg_off, cap,
                       out_offsets, out_lengths, out_flags);
    DGS_LAUNCH_CHECK("k_jpeg_scan", false, stream);
    hipLaunchKernelGGL(dgs::k_jpeg_entropy<true>, dim3((unsigned)G), dim3(dgs::JE_NT), 0, stream, g, (const int16_t *)coef,
                       seg_bytes, (const unsigned long long *)seg_off, out, cap);
    DGS_LAUNCH_CHECK("k_jpeg_entropy<write>", false, stream);
    return DGS_OK;
}
