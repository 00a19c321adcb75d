// Batched PNG encoding on the device: F uint8 frames (F,H,W,3) RGB or (F,H,W) grey -> F zlib streams (the body of
// one IDAT chunk each), packed back to back. The host adds the signature, IHDR, the chunk framing and IEND
// (deformgs/png_gpu.py). Four launches on one stream, no host wait, no floating point and no order-dependent
// atomics: the bytes are bitwise reproducible.
//
//   k_png_filter   one wave per (frame, row): the five PNG filter candidates, the cost of each = sum of |residual
//                  as int8| (libpng's heuristic), the cheapest wins, ties toward the lower type; writes the filter
//                  byte + W*C residuals. Every output byte reads original pixels only (deformgs/png.py filter_rows
//                  is the numpy restatement).
//   k_png_deflate  one workgroup per segment of PNG_SEG = 32 KiB of a frame's filtered stream. Segments are
//                  independent (no match reaches outside its own), so they deflate in parallel and concatenate:
//                  one dynamic-Huffman block (BTYPE 10), then an empty stored block (00 00 00 FF FF) that
//                  byte-aligns the stream; the last segment of a frame carries BFINAL and no aligner. Matches are
//                  runs only: distance 1, lengths 3..258. A segment that would not shrink is one stored block
//                  (n + 5 bytes), which bounds a segment's output. Also the segment's Adler-32 partial sums.
//                  32 KiB: a stored block holds at most 65535 bytes; the segment, its padded copy and the output
//                  image (<= n + 5 bytes, or it is stored) take 66 KiB of LDS, so two workgroups share a CU's
//                  160 KiB; the constant part of a block header (~170 bytes: code lengths at 4 bits each under a
//                  fixed, complete code-length code) stays near 0.5 % of a segment. 16 KiB would double that.
//   k_png_scan     exclusive prefix sum of the segments' byte counts (codec_bits.h segment_offsets).
//   k_png_pack     gathers the segments behind the zlib header 78 01, combines the Adler partials per frame
//                  (adler32_combine's rule) and writes each frame's offset and length.
//
// Code lengths: l = ceil(log2(total / freq)) clamped to 15 (a Shannon code: Kraft sum <= 1; the clamp cannot push
// it past 1 since only freq = 1 of total = 32769 is clamped, and then sum <= 32768 + 286/32769 in units of 2^-15),
// then codes are shortened, the one with the largest freq * 2^l that still fits first, until the sum is exactly 1:
// inflate rejects an incomplete literal/length code as well as an over-subscribed one. The shortest unit left is
// always that of a longest code, so the fill always ends exactly. The distance code is the single code 0 with one
// bit, the one incomplete code inflate accepts, present whether or not the segment has a match.
//
// The block scan, the segment-offset sum and the bit writer (here least significant bit first) are codec_bits.h's,
// shared with jpeg_encode.hip.
#include "codec_bits.h"
#include "dgs_common.h"

namespace dgs {
namespace {

using codec::put_at;

constexpr int PNG_SEG = 32768;                 // bytes of filtered stream per deflate segment
constexpr int PNG_NT = 512;                    // threads of k_png_deflate
constexpr int PNG_CH = PNG_SEG / PNG_NT;       // 64 consecutive bytes per thread
constexpr int PNG_SLOT = PNG_SEG + 16;         // a segment's output slot in scratch (stored: n + 5 bytes)
constexpr int PNG_OUTW = (PNG_SEG + 8) / 4 + 2;  // words of the LDS output image
constexpr int PNG_NSYM = 320;                  // literal/length alphabet (286) padded to 5 per lane of a wave
constexpr int PNG_EOB = 256;
constexpr unsigned ADLER_P = 65521u;
constexpr int PNG_MAX_DIM = 65536;
constexpr long long PNG_MAX_SEGMENTS = 1ll << 22;

// LDS carve of k_png_deflate (bytes, every offset a multiple of 16)
constexpr int L_BUF = 0;                                   // the segment, 4 bytes of padding per 64
constexpr int L_OUT = L_BUF + PNG_SEG + PNG_SEG / 16;      // output image
constexpr int L_FREQ = L_OUT + ((PNG_OUTW * 4 + 15) & ~15);
constexpr int L_CODE = L_FREQ + PNG_NSYM * 4;              // (length << 16) | bit-reversed code
constexpr int L_SA = L_CODE + PNG_NSYM * 4;
constexpr int L_SB = L_SA + PNG_NT * 4;
constexpr int L_RED = L_SB + PNG_NT * 4;                   // 8 x u64
constexpr int L_MISC = L_RED + 64;                         // 16 counts, 16 next codes, hlit, ok
constexpr int L_TOTAL = L_MISC + 160;
static_assert(L_TOTAL <= 80 * 1024, "two workgroups per CU");

__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ inline unsigned cost8(int v) {
    v &= 255;
    return (unsigned)(v < 128 ? v : 256 - v);
}

__device__ inline unsigned wave_sum(unsigned v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ inline int predict(int type, int a, int b, int c) {
    switch (type) {
        case 1: return a;
        case 2: return b;
        case 3: return (a + b) >> 1;
        case 4: return paeth(a, b, c);
        default: return 0;
    }
}

__global__ __launch_bounds__(256) void k_png_filter(long long rows_total, int H, int rb, int C, const uint8_t *in,
                                                    uint8_t *filt) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_total) return;  // a whole wave
    const bool top = (row % H) == 0;
    const uint8_t *cur = in + row * rb;
    const uint8_t *up = cur - rb;  // read only below the top row
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int x = lane; x < rb; x += 64) {
        const int v = cur[x];
        const int a = x >= C ? cur[x - C] : 0;
        const int b = top ? 0 : up[x];
        const int c = (top || x < C) ? 0 : up[x - C];
        c0 += cost8(v);
        c1 += cost8(v - a);
        c2 += cost8(v - b);
        c3 += cost8(v - ((a + b) >> 1));
        c4 += cost8(v - paeth(a, b, c));
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    c2 = wave_sum(c2);
    c3 = wave_sum(c3);
    c4 = wave_sum(c4);
    int type = 0;
    unsigned best = c0;
    if (c1 < best) { best = c1; type = 1; }
    if (c2 < best) { best = c2; type = 2; }
    if (c3 < best) { best = c3; type = 3; }
    if (c4 < best) { best = c4; type = 4; }
    uint8_t *o = filt + row * (rb + 1);
    if (lane == 0) o[0] = (uint8_t)type;
    for (int x = lane; x < rb; x += 64) {
        const int v = cur[x];
        const int a = x >= C ? cur[x - C] : 0;
        const int b = top ? 0 : up[x];
        const int c = (top || x < C) ? 0 : up[x - C];
        o[1 + x] = (uint8_t)((v - predict(type, a, b, c)) & 255);
    }
}

// ---- deflate ----

__device__ inline int bidx(int i) { return i + ((i >> 6) << 2); }  // thread t's chunk starts 17 words after t-1's

// match length 3..258 -> literal/length symbol, extra bit count and value (RFC 1951 3.2.5)
__device__ inline void len_symbol(int len, int &sym, int &eb, int &ev) {
    const int l = len - 3;
    if (len == 258) { sym = 285; eb = 0; ev = 0; return; }
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
    const int e = 29 - __clz(l);
    sym = 261 + 4 * e + ((l >> e) & 3);
    eb = e;
    ev = l & ((1 << e) - 1);
}

// The tokens of thread t's chunk, in stream order. A run of equal bytes [s, e) is: the literal at s, then its
// other R = e - s - 1 bytes as matches of 258 and one of R % 258 if that is at least 3, else as literals. A token
// belongs to the chunk its first byte is in. prev_start: where the run that enters the chunk began; next_start:
// the first run start behind the chunk (n if none).
template <class Lit, class Match>
__device__ inline void walk(const uint8_t *buf, int n, int t, int prev_start, int next_start, Lit lit, Match match) {
    const int lo = t * PNG_CH;
    if (lo >= n) return;
    const int ce = min(lo + PNG_CH, n);
    int p = lo;
    int s = (lo == 0 || buf[bidx(lo)] != buf[bidx(lo - 1)]) ? lo : prev_start;
    while (p < ce) {
        const int v = buf[bidx(p)];
        int j = p + 1;
        while (j < ce && buf[bidx(j)] == v) ++j;
        const int e = j < ce ? j : next_start;
        const int hi = j;
        const int R = e - s - 1;
        const int q258 = (R / 258) * 258, r = R - q258;
        if (p == s) lit(v);
        int k = p > s + 1 ? ((p - s - 1 + 257) / 258) * 258 : 0;
        for (; k < q258 && s + 1 + k < hi; k += 258) match(258);
        const int tp = s + 1 + q258;
        if (r >= 3) {
            if (tp >= p && tp < hi) match(r);
        } else {
            for (int x = 0; x < r; ++x)
                if (tp + x >= p && tp + x < hi) lit(v);
        }
        p = hi;
        s = hi;
    }
}

__device__ inline unsigned long long block_sum(unsigned long long v, unsigned long long *red, int t) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();  // red free again
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
    for (int i = 0; i < PNG_NT / 64; ++i) s += red[i];
    return s;
}

// Code lengths of the literal/length alphabet from freq[] (every used symbol, the end-of-block symbol among them,
// has freq >= 1; at least two are used) into code[] as (length << 16) | bit-reversed canonical code; -> hlit, ok.
// Wave 0 only; lane l owns symbols l, l + 64, ...
__device__ inline void build_code(const unsigned *freq, unsigned *code, int *misc, int lane) {
    unsigned fr[5];
    int ln[5];
    unsigned total = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        fr[j] = freq[lane + 64 * j];
        total += fr[j];
    }
    total = wave_sum(total);
    unsigned K = 0;  // Kraft sum in units of 2^-15
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        int l = 0;
        if (fr[j]) {
            l = 1;
            while (l < 15 && (fr[j] << l) < total) ++l;
            K += 1u << (15 - l);
        }
        ln[j] = l;
    }
    K = wave_sum(K);
    for (int it = 0; it < 15 * 286 && K < 32768u; ++it) {
        const unsigned D = 32768u - K;
        unsigned long long best = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (ln[j] > 1 && (1u << (15 - ln[j])) <= D) {
                const unsigned long long key = ((unsigned long long)(fr[j] << ln[j]) << 20) |
                                               ((unsigned long long)(511 - (lane + 64 * j)) << 4) | (unsigned)ln[j];
                best = key > best ? key : best;
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d);
            best = o > best ? o : best;
        }
        if (best == 0) break;
        const int l = (int)(best & 15), sym = 511 - (int)((best >> 4) & 0xFFFF);
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (lane + 64 * j == sym) ln[j] -= 1;
        K += 1u << (15 - l);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) code[lane + 64 * j] = (unsigned)ln[j];
    __builtin_amdgcn_wave_barrier();  // one wave: its LDS accesses complete in program order
    if (lane == 0) {
        int *cnt = misc, *next = misc + 16;
        for (int i = 0; i < 16; ++i) cnt[i] = 0;
        int hlit = 257;
        for (int s = 0; s < 286; ++s) {
            const int l = (int)code[s];
            cnt[l] += 1;
            if (l && s >= 257) hlit = s + 1;
        }
        cnt[0] = 0;
        int c = 0;
        for (int b = 1; b <= 15; ++b) {
            c = (c + cnt[b - 1]) << 1;
            next[b] = c;
        }
        for (int s = 0; s < 286; ++s) {
            const int l = (int)code[s];
            if (l) {
                const unsigned cw = (unsigned)next[l]++;
                code[s] = (__brev(cw) >> (32 - l)) | ((unsigned)l << 16);
            }
        }
        misc[32] = hlit;
        misc[33] = K == 32768u;
    }
}

__global__ __launch_bounds__(PNG_NT) void k_png_deflate(int nseg, long long fbytes, const uint8_t *filt, uint8_t *slots,
                                                        uint4 *meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint8_t *buf = smem + L_BUF;
    unsigned *outw = (unsigned *)(smem + L_OUT);
    unsigned *freq = (unsigned *)(smem + L_FREQ);
    unsigned *code = (unsigned *)(smem + L_CODE);
    int *sa = (int *)(smem + L_SA);
    int *sb = (int *)(smem + L_SB);
    unsigned long long *red = (unsigned long long *)(smem + L_RED);
    int *misc = (int *)(smem + L_MISC);

    const int t = threadIdx.x;
    const long long g = blockIdx.x;
    const long long f = g / nseg;
    const int j = (int)(g - f * nseg);
    const long long off = (long long)j * PNG_SEG;
    const int n = (int)min((long long)PNG_SEG, fbytes - off);
    const bool last = j == nseg - 1;
    const uint8_t *src = filt + f * fbytes + off;
    uint8_t *dst = slots + g * PNG_SLOT;

    for (int i = t; i < n; i += PNG_NT) buf[bidx(i)] = src[i];
    for (int i = t; i < PNG_NSYM; i += PNG_NT) freq[i] = i == PNG_EOB ? 1u : 0u;
    for (int i = t; i < PNG_OUTW; i += PNG_NT) outw[i] = 0;
    __syncthreads();

    // run starts per chunk (last and first), Adler partial sums
    const int lo = t * PNG_CH, ce = min(lo + PNG_CH, n);
    int ls = -1, fs = n;
    unsigned a = 0, b = 0;
    {
        int prev = lo > 0 && lo < n ? buf[bidx(lo - 1)] : -1;
        for (int i = lo; i < ce; ++i) {
            const int v = buf[bidx(i)];
            if (v != prev) {
                ls = i;
                fs = min(fs, i);
            }
            a += (unsigned)v;
            b += (unsigned)(n - i) * (unsigned)v;
            prev = v;
        }
    }
    sa[t] = ls;
    sb[t] = fs;
    __syncthreads();
    // running maximum of sa, running minimum of sb from the right: two arrays and two directions under one pair of
    // barriers per step, which is why this is not codec::block_scan (codec_bits.h)
    for (int d = 1; d < PNG_NT; d <<= 1) {
        const int x = sa[t], y = t >= d ? sa[t - d] : -1;
        const int u = sb[t], w = t + d < PNG_NT ? sb[t + d] : n;
        __syncthreads();
        sa[t] = max(x, y);
        sb[t] = min(u, w);
        __syncthreads();
    }
    const int prev_start = t > 0 ? sa[t - 1] : 0;
    const int next_start = t < PNG_NT - 1 ? sb[t + 1] : n;
    const unsigned long long asum = block_sum(a, red, t);
    const unsigned long long bsum = block_sum(b, red, t);

    walk(buf, n, t, prev_start, next_start, [&](int v) { atomicAdd(&freq[v], 1u); },
         [&](int len) {
             int sym, eb, ev;
             len_symbol(len, sym, eb, ev);
             atomicAdd(&freq[sym], 1u);
         });
    __syncthreads();
    if (t < 64) build_code(freq, code, misc, t);
    __syncthreads();
    const int hlit = misc[32];
    const bool ok = misc[33] != 0;

    unsigned bits = 0;
    walk(buf, n, t, prev_start, next_start, [&](int v) { bits += code[v] >> 16; },
         [&](int len) {
             int sym, eb, ev;
             len_symbol(len, sym, eb, ev);
             bits += (code[sym] >> 16) + (unsigned)eb + 1u;
         });
    const unsigned my_bit = (unsigned)codec::block_scan<PNG_NT>((int)bits, sa, t) - bits;
    const unsigned tokbits = (unsigned)sa[PNG_NT - 1];
    const unsigned hdr_bits = 74u + 4u * (unsigned)(hlit + 1);
    const unsigned eob_len = code[PNG_EOB] >> 16;
    const unsigned end_bits = hdr_bits + tokbits + eob_len;
    const unsigned dyn_bytes = last ? (end_bits + 7) / 8 : (end_bits + 3 + 7) / 8 + 4;
    const bool use_dyn = ok && dyn_bytes <= (unsigned)n + 5u;

    unsigned out_len;
    if (use_dyn) {
        if (t == 0) {
            put_at(outw, 0, last ? 1u : 0u, 1);
            put_at(outw, 1, 2u, 2);                       // BTYPE 10
            put_at(outw, 3, (unsigned)(hlit - 257), 5);   // HLIT
            put_at(outw, 8, 0u, 5);                       // HDIST: one distance code
            put_at(outw, 13, 15u, 4);                     // HCLEN: all 19 code-length code lengths
            // in the order 16 17 18 0 8 7 ...: symbols 0..15 get 4 bits (a complete code), 16..18 are unused
            for (int k = 3; k < 19; ++k) put_at(outw, 17u + 3u * (unsigned)k, 4u, 3);
        }
        if (t <= hlit) {  // the code lengths, 4 bits each, code of value v = v, sent most significant bit first
            const unsigned l = t < hlit ? code[t] >> 16 : 1u;
            put_at(outw, 74u + 4u * (unsigned)t, __brev(l) >> 28, 4);
        }
        codec::BitWriter<false> bw(outw, hdr_bits + my_bit);  // put: <= 15 + 5 + 1 = 21 bits
        walk(buf, n, t, prev_start, next_start, [&](int v) { bw.put(code[v] & 0xFFFFu, (int)(code[v] >> 16)); },
             [&](int len) {
                 int sym, eb, ev;
                 len_symbol(len, sym, eb, ev);
                 const unsigned c = code[sym];
                 // the code, the extra bits, the one-bit distance code 0
                 bw.put((c & 0xFFFFu) | ((unsigned)ev << (c >> 16)), (int)(c >> 16) + eb + 1);
             });
        bw.flush();
        if (t == PNG_NT - 1) {
            put_at(outw, hdr_bits + tokbits, code[PNG_EOB] & 0xFFFFu, (int)eob_len);
            if (!last) put_at(outw, ((end_bits + 3 + 7) & ~7u), 0xFFFF0000u, 32);  // 000 + padding, LEN 0, NLEN FFFF
        }
        __syncthreads();
        unsigned *d32 = (unsigned *)dst;
        for (unsigned i = t; i < (dyn_bytes + 3) / 4; i += PNG_NT) d32[i] = outw[i];
        out_len = dyn_bytes;
    } else {
        if (t == 0) {
            dst[0] = last ? 1 : 0;
            dst[1] = (uint8_t)(n & 255);
            dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)(~n & 255);
            dst[4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int i = t; i < n; i += PNG_NT) dst[5 + i] = buf[bidx(i)];
        out_len = (unsigned)n + 5u;
    }
    if (t == 0) meta[g] = make_uint4(out_len, (unsigned)(asum % ADLER_P), (unsigned)(bsum % ADLER_P), (unsigned)n);
}

__global__ __launch_bounds__(1024) void k_png_scan(long long G, const uint4 *meta, unsigned long long *seg_off) {
    __shared__ unsigned long long part[1024];
    codec::segment_offsets(G, [&](long long i) { return meta[i].x; }, seg_off, part);
}

__global__ __launch_bounds__(256) void k_png_pack(int nseg, const uint8_t *slots, const uint4 *meta,
                                                  const unsigned long long *seg_off, uint8_t *out, int64_t *out_offsets,
                                                  int64_t *out_lengths) {
    const int t = threadIdx.x;
    const long long g = blockIdx.x;
    const long long f = g / nseg;
    const int j = (int)(g - f * nseg);
    const unsigned len = meta[g].x;
    const long long frame0 = 6 * f + (long long)seg_off[f * nseg];  // 2 bytes of zlib header + 4 of Adler-32 per frame
    const long long d0 = 6 * f + 2 + (long long)seg_off[g];
    const uint8_t *src = slots + g * PNG_SLOT;
    for (unsigned i = t; i < len; i += 256) out[d0 + i] = src[i];
    if (t != 0) return;
    if (j == 0) {
        out[frame0] = 0x78;
        out[frame0 + 1] = 0x01;
        out_offsets[f] = frame0;
    }
    if (j == nseg - 1) {
        unsigned long long A = 1, B = 0;
        for (int k = 0; k < nseg; ++k) {
            const uint4 m = meta[f * nseg + k];
            B = (B + (unsigned long long)(m.w % ADLER_P) * A + m.z) % ADLER_P;
            A = (A + m.y) % ADLER_P;
        }
        const long long e = d0 + len;
        out[e] = (uint8_t)(B >> 8);
        out[e + 1] = (uint8_t)(B & 255);
        out[e + 2] = (uint8_t)(A >> 8);
        out[e + 3] = (uint8_t)(A & 255);
        out_lengths[f] = e + 4 - frame0;
    }
}

struct PngPlan {
    long long fbytes, nseg, G;
    size_t filt_bytes, slot_bytes, meta_bytes, off_bytes;
};

bool png_plan(int F, int H, int W, int C, PngPlan &p) {
    if (F < 1 || H < 1 || W < 1 || (C != 1 && C != 3)) return false;
    if (H > PNG_MAX_DIM || W > PNG_MAX_DIM) return false;
    p.fbytes = (long long)H * (1 + (long long)W * C);
    p.nseg = (p.fbytes + PNG_SEG - 1) / PNG_SEG;
    p.G = p.nseg * F;
    p.filt_bytes = ((size_t)p.fbytes * F + 15) & ~(size_t)15;
    p.slot_bytes = (size_t)p.G * PNG_SLOT;
    p.meta_bytes = (size_t)p.G * sizeof(uint4);
    p.off_bytes = (size_t)p.G * sizeof(unsigned long long);
    return true;
}

}  // namespace
}  // namespace dgs

extern "C" size_t dgs_png_encode_scratch_bytes(int F, int H, int W, int C) {
    dgs::PngPlan p;
    if (!dgs::png_plan(F, H, W, C, p)) return 0;
    return p.filt_bytes + p.slot_bytes + p.meta_bytes + p.off_bytes;
}

extern "C" size_t dgs_png_out_capacity(int F, int H, int W, int C) {
    dgs::PngPlan p;
    if (!dgs::png_plan(F, H, W, C, p)) return 0;
    return (size_t)F * 6 + (size_t)p.fbytes * F + (size_t)p.G * 5;  // every segment stored
}

extern "C" int dgs_png_encode(int F, int H, int W, int C, const uint8_t *in, uint8_t *out, int64_t *out_offsets,
                              int64_t *out_lengths, uint8_t *scratch, void *stream_) {
    dgs::PngPlan p;
    if (!dgs::png_plan(F, H, W, C, p) || !in || !out || !out_offsets || !out_lengths || !scratch ||
        ((uintptr_t)scratch & 15)) {
        dgs::set_error("dgs_png_encode: bad argument (F, H, W >= 1, H and W <= 65536, C 1 or 3, scratch 16-byte aligned)");
        return DGS_ERR_ARGS;
    }
    const long long rows = (long long)F * H;
    if (p.G > dgs::PNG_MAX_SEGMENTS || (rows + 3) / 4 > 0x7fffffffll) {
        dgs::set_error("dgs_png_encode: batch too large for one launch (encode it in chunks)");
        return DGS_ERR_UNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t *filt = scratch;
    uint8_t *slots = filt + p.filt_bytes;
    uint4 *meta = (uint4 *)(slots + p.slot_bytes);
    unsigned long long *seg_off = (unsigned long long *)((uint8_t *)meta + p.meta_bytes);
    if (int rc = dgs::ensure_dynamic_lds((const void *)dgs::k_png_deflate, dgs::L_TOTAL)) return rc;
    hipLaunchKernelGGL(dgs::k_png_filter, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, rows, H, W * C, C, in, filt);
    DGS_LAUNCH_CHECK("k_png_filter", false, stream);
    hipLaunchKernelGGL(dgs::k_png_deflate, dim3((unsigned)p.G), dim3(dgs::PNG_NT), dgs::L_TOTAL, stream, (int)p.nseg, p.fbytes,
                       (const uint8_t *)filt, slots, meta);
    DGS_LAUNCH_CHECK("k_png_deflate", false, stream);
    hipLaunchKernelGGL(dgs::k_png_scan, dim3(1), dim3(1024), 0, stream, p.G, (const uint4 *)meta, seg_off);
    DGS_LAUNCH_CHECK("k_png_scan", false, stream);
    hipLaunchKernelGGL(dgs::k_png_pack, dim3((unsigned)p.G), dim3(256), 0, stream, (int)p.nseg, (const uint8_t *)slots,
                       (const uint4 *)meta, (const unsigned long long *)seg_off, out, out_offsets, out_lengths);
    DGS_LAUNCH_CHECK("k_png_pack", false, stream);
    return DGS_OK;
}
