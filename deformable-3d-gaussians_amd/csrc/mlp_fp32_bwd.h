// Fused deformation MLP on fp32 MFMA, backward dX chain (device code of mlp.hip's translation
// unit): k_mlp_bwd writes dZ_i of every layer to scratch; deterministic.
#pragma once
#include "mlp_fp32_core.h"

namespace dgs {
namespace mlp {

// float offsets into the packed buffer (make_plan): backward (transposed) A images
struct BwdOffsets {
    int tHd, tL[8], tT2;
};

struct BwdArgs {
    int N;
    size_t Ns;
    const float *packed;
    const float *saved;
    const uint32_t *mask;
    const float *dout;
    float *dz;
    BwdOffsets o;
    int flags;
};

// relu' of the layer input for this wave's 32x32 tile: the forward's 16 bits per lane (same lane
// layout), one u16 load per lane ahead of the GEMM instead of 16 activation loads
struct MaskPre {
    uint32_t *mk;
    const uint32_t *words;  // &mask[block][mrow0 + n0]: 64 u16, one per lane
    int lane;
    __device__ void operator()() const { *mk = reinterpret_cast<const unsigned short *>(words)[lane]; }
};

__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_mlp_bwd(BwdArgs a) {
    __shared__ float4 lds[G_TOTAL * BM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (scalar branches)
    const int p0 = blockIdx.x * BM;
    const Flags F = make_flags(a.flags);
    const float4 *pk = reinterpret_cast<const float4 *>(a.packed);
    float *lf = reinterpret_cast<float *>(lds);
    const uint32_t *mwords = a.mask + (size_t)blockIdx.x * F.nmask + wave * 32;  // + mask row
    // dOut -> LDS TE region (the head-gradient image G) and dz rows Z_G
    for (int e = tid; e < 32 * BM; e += NTHR) {
        int m = e % BM, c = e / BM;
        int p = p0 + m;
        float v = (p < a.N && c < F.nout) ? a.dout[(size_t)p * F.nout + c] : 0.f;
        lf[((G_TE + c / 4) * BM + m) * 4 + (c & 3)] = v;
        a.dz[(size_t)(Z_G + c) * a.Ns + p] = v;
    }
    lds_barrier();
    // dZ_i of the trunk stays in registers and is stored during the next GEMM (Stash1)
    f32x16 kt;  // dZ of the layer whose GEMM runs next
    // heads^T: dH7 = W_h^T dOut (K = 32 from TE region) -> mask H7 -> dZ7
    {
        uint32_t mk;
        f32x16 c = zero16();
        gemm<4>(pk + a.o.tHd / 4 + wave * 4 * 64, 0, lds, G_TE, lane, c, MaskPre{&mk, mwords + m_h(7), lane});
        mask_apply(c, mk);
        lds_barrier();  // TE (dOut image) reads done before TE is reused for dTE
        acc_to_lds(c, lds, G_H, wave * 32, lane);
        kt = c;
    }
    // zero the dTE accumulator (TE region holds dL/dt_emb from layers 5 and 0)
    for (int e = tid; e < 8 * BM; e += NTHR) lds[G_TE * BM + e] = make_float4(0.f, 0.f, 0.f, 0.f);
    lds_barrier();
    for (int L = 7; L >= 1; L--) {
        // dX_L = W_L^T dZ_L ; H-part rows of the padded input live at tiles (F_H/32 + w) for L=5
        const int tile0 = (L == 5) ? F_H / 32 : 0;
        if (L == 5 && F.blender) {
            // t_emb slice (padded rows 64..95 = tile 2): K split over the 8 waves -> PART
            f32x16 ct = zero16();
            gemm<4>(pk + a.o.tL[5] / 4 + (F_TE / 32) * 32 * 64, wave * 4, lds, G_H, lane, ct);
            acc_to_lds(ct, lds, G_PART + 8 * wave, 0, lane);
        }
        uint32_t mk;  // relu' of H_{L-1}, in flight during the GEMM
        f32x16 c = zero16();
        gemm<32>(pk + a.o.tL[L] / 4 + (tile0 + wave) * 32 * 64, 0, lds, G_H, lane, c, MaskPre{&mk, mwords + m_h(L - 1), lane},
                 Stash1{kt, tile_addr(a.dz, a.Ns, Z_L0 + L * 256, wave * 32, p0, lane)});
        mask_apply(c, mk);
        lds_barrier();
        if (L == 5 && F.blender) sum_parts(lds, G_TE, nullptr, tid, true);
        acc_to_lds(c, lds, G_H, wave * 32, lane);
        lds_barrier();
        kt = c;
    }
    const Stash1 dz0{kt, tile_addr(a.dz, a.Ns, Z_L0, wave * 32, p0, lane)};
    if (!F.blender) {
        dz0.store_all();
        return;  // raw t PE has no parameters upstream of it
    }
    // layer 0: t_emb slice of W_0^T dZ_0 (K split over the waves); dZ_0 is stored under it
    {
        f32x16 ct = zero16();
        gemm<4>(pk + a.o.tL[0] / 4 + (F_TE / 32) * 32 * 64, wave * 4, lds, G_H, lane, ct, NoPre(), dz0);
        acc_to_lds(ct, lds, G_PART + 8 * wave, 0, lane);
        lds_barrier();
        sum_parts(lds, G_TE, nullptr, tid, true);
        lds_barrier();
    }
    // dTE (30 real rows) -> global (dW of timenet.2)
    lds_to_global(lds, G_TE, 8, a.dz, Z_TE, a.Ns, p0, tid);
    // timenet.2^T: dTH = W_T2^T dTE (K = 32) -> mask TH -> dZ_T1
    {
        uint32_t mk;
        f32x16 c = zero16();
        gemm<4>(pk + a.o.tT2 / 4 + wave * 4 * 64, 0, lds, G_TE, lane, c, MaskPre{&mk, mwords + M_TH, lane});
        mask_apply(c, mk);
        Stash1{c, tile_addr(a.dz, a.Ns, Z_T1, wave * 32, p0, lane)}.store_all();
    }
}

}  // namespace mlp
}  // namespace dgs
