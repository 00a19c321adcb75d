// What the device image encoders (png_encode.hip, jpeg_encode.hip) share, written once: the block-wide inclusive
// scan, the one-workgroup prefix sum that turns per-segment byte counts into segment offsets, and the writer that ORs
// a thread's bits into a zeroed LDS bit image. Device-only.
#pragma once
#include <hip/hip_runtime.h>

namespace dgs {
namespace codec {

// Inclusive prefix sum of v over the NT threads of the workgroup (Hillis-Steele: log2 NT steps, each reading both
// operands, a barrier, the store, a barrier); lds has NT entries. On return lds[i] is thread i's result for every i,
// so lds[NT - 1] is the total, until the next call.
// k_png_deflate's run-start scan (a running maximum from the left and a running minimum from the right over two arrays
// under the same two barriers per step) stays written out there: as two calls it would take twice the barriers, and
// as one call over a pair the template would need an operator, an identity and a direction per component.
template <int NT, class T>
__device__ inline T block_scan(T v, T *lds, int t) {
    __syncthreads();  // lds free again
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const T x = lds[t], y = t >= d ? lds[t - d] : T(0);
        __syncthreads();
        lds[t] = x + y;
        __syncthreads();
    }
    return lds[t];
}

// seg_off[i] = the sum of len_of(j) over j < i, for i in [0, G); -> the sum over all G, in every thread. One workgroup
// of 1024 threads, thread t taking ceil(G / 1024) consecutive segments; part has 1024 entries.
template <class LenOf>
__device__ inline unsigned long long segment_offsets(long long G, LenOf len_of, unsigned long long *seg_off,
                                                     unsigned long long *part) {
    const int t = threadIdx.x;
    const long long per = (G + 1023) / 1024;
    const long long i0 = min(G, t * per), i1 = min(G, i0 + per);
    unsigned long long s = 0;
    for (long long i = i0; i < i1; ++i) s += len_of(i);
    unsigned long long run = block_scan<1024>(s, part, t) - s;
    for (long long i = i0; i < i1; ++i) {
        seg_off[i] = run;
        run += len_of(i);
    }
    return part[1023];
}

// ORs the low nbits (<= 32) of v into the zeroed bit image at bit pos, least significant bit first
__device__ inline void put_at(unsigned *img, unsigned pos, unsigned v, int nbits) {
    const unsigned long long x = (unsigned long long)v << (pos & 31);
    (void)nbits;
    if ((unsigned)x) atomicOr(&img[pos >> 5], (unsigned)x);
    if ((unsigned)(x >> 32)) atomicOr(&img[(pos >> 5) + 1], (unsigned)(x >> 32));
}

// Writes a thread's bits, from bit pos on, into the zeroed image: bit i of the stream is bit 31 - (i & 31) of word
// i >> 5 (MSB_FIRST: JPEG) or bit i & 31 (deflate). A thread's bits are contiguous, so only its first and its last
// word are shared with a neighbour; the LDS atomics cover those, and flush() skips a last word that is zero.
// put(v, n): v < 2^n, and n <= 32 since acc holds up to 31 pending bits; n <= 26 in jpeg_encode.hip (a 16-bit code
// + a 10-bit value), <= 21 in png_encode.hip (a 15-bit code + 5 extra bits + the distance bit).
template <bool MSB_FIRST>
struct BitWriter {
    unsigned *img;
    unsigned long long acc;
    int nacc;
    unsigned w;
    __device__ BitWriter(unsigned *o, unsigned pos) : img(o), acc(0), nacc((int)(pos & 31)), w(pos >> 5) {}
    __device__ void put(unsigned v, int n) {
        if constexpr (MSB_FIRST) {
            acc = (acc << n) | v;
            nacc += n;
            if (nacc >= 32) {
                nacc -= 32;
                atomicOr(&img[w++], (unsigned)(acc >> nacc));
                acc &= (1ull << nacc) - 1;
            }
        } else {
            acc |= (unsigned long long)v << nacc;
            nacc += n;
            if (nacc >= 32) {
                atomicOr(&img[w++], (unsigned)acc);
                acc >>= 32;
                nacc -= 32;
            }
        }
    }
    __device__ void flush() {
        if constexpr (MSB_FIRST) {
            if (nacc > 0 && acc) atomicOr(&img[w], (unsigned)(acc << (32 - nacc)));
        } else {
            if (nacc > 0 && (unsigned)acc) atomicOr(&img[w], (unsigned)acc);
        }
    }
};

}  // namespace codec
}  // namespace dgs
