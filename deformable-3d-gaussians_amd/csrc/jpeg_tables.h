// What the JPEG files of csrc/ share, written once: the zigzag order (jpeg_decode.h on the host, jpeg_encode.hip's
// __constant__ copy on the device), the fixed-point constants of libjpeg's "islow" DCT pair (idct8 of jpeg.hip, fdct8
// of jpeg_encode.hip) and the block layout of the two 8x8 transform kernels. Plain C++17, no HIP includes:
// tools/jpeg_host_check.cpp compiles it with jpeg_decode.h on the host alone.
// The Python restatements (deformgs/jpeg.py, tests/jpeg_encode_ref.py) and the Annex K tables keep their own copies on
// purpose: they are what the tests hold this code against.
#pragma once

#include <cstdint>

// Position k of a block's zigzag sequence -> its index in natural (row-major) order. A list, so that a
// __constant__ array can be initialised from the same 64 numbers.
#define DGS_JPEG_ZIGZAG_ORDER                                                                      \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, \
    13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,  \
    52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63

namespace dgs_jpeg {

static const uint8_t ZIGZAG[64] = {DGS_JPEG_ZIGZAG_ORDER};

// jfdctint.c / jidctint.c: FIX(x) = round(x * 2^13) (CONST_BITS 13)
constexpr int FIX_0_298631336 = 2446;
constexpr int FIX_0_390180644 = 3196;
constexpr int FIX_0_541196100 = 4433;
constexpr int FIX_0_765366865 = 6270;
constexpr int FIX_0_899976223 = 7373;
constexpr int FIX_1_175875602 = 9633;
constexpr int FIX_1_501321110 = 12299;
constexpr int FIX_1_847759065 = 15137;
constexpr int FIX_1_961570560 = 16069;
constexpr int FIX_2_053119869 = 16819;
constexpr int FIX_2_562915447 = 20995;
constexpr int FIX_3_072711026 = 25172;

// k_jpeg_idct and k_jpeg_transform: eight lanes per 8x8 block, so a 256-thread workgroup holds WG_BLOCKS blocks; lane r
// has row r and, after a transpose through LDS, column r. The rows of a block lie LDS_ROW dwords apart (a block 72),
// so the row and the column accesses both spread over the banks.
constexpr int WG_BLOCKS = 32;
constexpr int LDS_ROW = 9;

}  // namespace dgs_jpeg
