// Fused deformation MLP on split f16, the active set (device code of mlp_split.hip's translation unit):
// the Gaussians whose dOut row has any nonzero element, found and compacted on the device every step.
//
// A culled Gaussian, or one behind the transmittance cut-off of every pixel it covers, gets an all-zero
// dOut row from the rasterizer's backward; its dZ is zero at every layer and it adds +0 to every weight
// and bias gradient (xyz enters the network detached: no input gradient either). About half of the
// bench scene's Gaussians are such rows, spread evenly over the 64-point blocks, so the
// dX chain and the dW GEMM cannot skip them in place. Instead the training step's first forward saves
// nothing (k_fwd8_nosave), and after the input glue's backward the M active rows' xyz and dOut are
// gathered in ascending index order (stable: the gradients stay a deterministic function of dOut); the
// saving forward, the dX chain and the dW GEMM then run on M dense points, reading M from device memory
// (FwdArgs::n_dev, BwdArgs::n_dev, k_dws's n_dev): the host never waits for it.
//
//   k_active_count   one workgroup per ACT_ROWS rows: the number of active rows among them
//   k_active_gather  the same workgroups: the sum of the counts before theirs, the block scan of their
//                    flags (codec_bits.h block_scan), the rows' xyz and dOut to their compacted places;
//                    the last workgroup stores M. Launched as one workgroup with `gather` off it only
//                    stores M (the steps that keep the full backward still measure the active fraction).
#pragma once
#include <hip/hip_runtime.h>

#include "codec_bits.h"
#include "dgs_common.h"

namespace dgs {
namespace mlps {

constexpr int ACT_ROWS = 1024;  // rows per workgroup = threads

struct ActiveArgs {
    int N, nout;
    const float *xyz, *dout;   // (N, 3), (N, nout)
    float *xyz_c, *dout_c;     // the active rows, compacted
    int *counts;               // [div_up(N, ACT_ROWS)]
    int *m_dev;                // M
    uint32_t *m_host;          // a mapped host word that receives M as well, or nullptr
};

// any element of the row is nonzero (+-0 are not; a denormal or a NaN is)
__device__ __forceinline__ bool row_active(const ActiveArgs &a, int r) {
    if (r >= a.N) return false;
    uint32_t bits = 0;
    for (int c = 0; c < a.nout; c++) bits |= __float_as_uint(a.dout[(size_t)r * a.nout + c]);
    return (bits & 0x7fffffffu) != 0;
}

__global__ __launch_bounds__(ACT_ROWS) void k_active_count(ActiveArgs a) {
    const int n = __syncthreads_count(row_active(a, blockIdx.x * ACT_ROWS + threadIdx.x) ? 1 : 0);
    if (threadIdx.x == 0) a.counts[blockIdx.x] = n;
}

__global__ __launch_bounds__(ACT_ROWS) void k_active_gather(ActiveArgs a, int gather) {
    __shared__ int part[ACT_ROWS];
    const int t = threadIdx.x;
    const int nb = div_up(a.N, ACT_ROWS);
    const int b = gather ? (int)blockIdx.x : nb;  // counting only: the total of every workgroup's count
    int s = 0;
    for (int i = t; i < b; i += ACT_ROWS) s += a.counts[i];
    codec::block_scan<ACT_ROWS>(s, part, t);
    const int base = part[ACT_ROWS - 1];
    if (!gather) {
        if (t == 0) {
            *a.m_dev = base;
            if (a.m_host) *a.m_host = (uint32_t)base;
        }
        return;
    }
    const int r = b * ACT_ROWS + t;
    const int f = row_active(a, r) ? 1 : 0;
    const int pos = base + codec::block_scan<ACT_ROWS>(f, part, t) - f;
    if (b == nb - 1 && t == ACT_ROWS - 1) {
        *a.m_dev = pos + f;
        if (a.m_host) *a.m_host = (uint32_t)(pos + f);
    }
    if (!f) return;
    for (int c = 0; c < 3; c++) a.xyz_c[(size_t)pos * 3 + c] = a.xyz[(size_t)r * 3 + c];
    for (int c = 0; c < a.nout; c++) a.dout_c[(size_t)pos * a.nout + c] = a.dout[(size_t)r * a.nout + c];
}

}  // namespace mlps
}  // namespace dgs
