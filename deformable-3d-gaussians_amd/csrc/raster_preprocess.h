// Rasterizer, per-Gaussian stage (device code of raster.hip's translation unit; the pipeline map is at the
// top of raster.hip):
//   k_preprocess     1 thread / Gaussian: cull, Sigma3D, EWA Sigma2D, conic, radius, tile rect, SH->RGB,
//                    depth key (float bits; culled -> all-ones); zeroes the backward's accumulators
//   k_preprocess_bwd 1 thread / Gaussian: conic->Sigma2D->(Sigma3D, mean), projection, SH, Sigma3D->(s,q)
//   k_mark_visible   dgs_mark_visible: the frustum test alone
#pragma once
#include "raster_kernels.h"

namespace dgs {

// STAGE (M = 16, 16-byte aligned SH): the block's SH rows are read into LDS with coalesced
// 16-byte loads before any thread culls its Gaussian (see k_preprocess_bwd)
constexpr int SH_ROW = 48, SH_PAD = 49;  // odd LDS row stride: a thread-per-row access is conflict-free

// The block's nrow SH rows into LDS rows of SH_PAD floats: from one (P, 16, 3) tensor, or split
// (rest != nullptr) from features_dc (P, 1, 3) and features_rest (P, 15, 3) as the Gaussian model
// stores them (no concatenated copy). All loads are 16-byte units of contiguous row blocks, every
// load of a thread issued before its first LDS store (a rolled loop waited out one HBM round trip
// per 256 units: 12 in a row for the 256 rows of a block).
template <int MAXU>
__device__ __forceinline__ void sh_get(float *s_sh, const float *base, int rowlen, int off, int b0, int nrow) {
    const int n = nrow * rowlen;
    const float *src = base + (size_t)b0 * rowlen;
    const int nu = div_up(n, 4);
    auto put = [&](int u, const float *w) {
        int r = 4 * u / rowlen, c = 4 * u - r * rowlen;  // one division per unit, then carry
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (4 * u + j < n) s_sh[r * SH_PAD + off + c] = w[j];
            if (++c == rowlen) {
                c = 0;
                r++;
            }
        }
    };
    if (n % 4 == 0) {  // whole units (every block but possibly the tensor's last): loads first
        float4 v[MAXU];
#pragma unroll
        for (int k = 0; k < MAXU; k++) {
            const int u = threadIdx.x + 256 * k;
            if (u < nu) v[k] = reinterpret_cast<const float4 *>(src)[u];
        }
#pragma unroll
        for (int k = 0; k < MAXU; k++) {
            const int u = threadIdx.x + 256 * k;
            if (u < nu) {
                const float w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                put(u, w);
            }
        }
        return;
    }
    for (int u = threadIdx.x; u < nu; u += 256) {
        float w[4];
        if (4 * u + 3 < n) {
            const float4 v = reinterpret_cast<const float4 *>(src)[u];
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {  // the tensor's last partial unit: no read past its end
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = 4 * u + j < n ? src[4 * u + j] : 0.f;
        }
        put(u, w);
    }
}

__device__ __forceinline__ void sh_stage_in(float *s_sh, const float *shs, const float *rest, int b0, int nrow) {
    if (!rest) {
        sh_get<SH_ROW / 4>(s_sh, shs, SH_ROW, 0, b0, nrow);  // 256 rows x 12 units: 12 per thread
        return;
    }
    sh_get<1>(s_sh, shs, 3, 0, b0, nrow);                                  // 192 units
    sh_get<(256 * (SH_ROW - 3) / 4 + 255) / 256>(s_sh, rest, SH_ROW - 3, 3, b0, nrow);  // 2880 units
}

// LDS rows -> the (P, 16, 3) gradient, or split into the dc (P, 1, 3) / rest (P, 15, 3) gradients
__device__ __forceinline__ void sh_stage_out(const float *s_sh, float *dsh, float *drest, int b0, int nrow) {
    if (!drest) {
        float4 *dst = reinterpret_cast<float4 *>(dsh + (size_t)b0 * SH_ROW);
        for (int u = threadIdx.x; u < nrow * (SH_ROW / 4); u += 256) {
            const float *d = s_sh + (u / (SH_ROW / 4)) * SH_PAD + (u % (SH_ROW / 4)) * 4;
            dst[u] = make_float4(d[0], d[1], d[2], d[3]);
        }
        return;
    }
    auto put = [&](float *base, int rowlen, int off) {
        const int n = nrow * rowlen;
        float4 *dst = reinterpret_cast<float4 *>(base + (size_t)b0 * rowlen);
        for (int u = threadIdx.x; u < div_up(n, 4); u += 256) {
            float w[4];
            int r = 4 * u / rowlen, c = 4 * u - r * rowlen;  // one division per unit, then carry
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w[j] = 4 * u + j < n ? s_sh[r * SH_PAD + off + c] : 0.f;
                if (++c == rowlen) {
                    c = 0;
                    r++;
                }
            }
            if (4 * u + 3 < n) {
                dst[u] = make_float4(w[0], w[1], w[2], w[3]);
            } else {
                for (int j = 0; 4 * u + j < n; j++) base[(size_t)b0 * rowlen + 4 * u + j] = w[j];
            }
        }
    };
    put(dsh, 3, 0);
    put(drest, SH_ROW - 3, 3);
}

// FWD (forward-only rendering, dgs_render_frames): no backward accumulators are zeroed and neither clamped
// nor visible is written (acc, clamped, visible are null); every value binning and the blend read (radii
// included: the binning kernels take the tile rectangle from it) is computed by the same instructions
template <bool STAGE, bool FWD = false>
__global__ __launch_bounds__(256) void k_preprocess(
    int P, int D, int M, const float *__restrict__ means3D, const float *__restrict__ scales, float mod,
    const float *__restrict__ rots, const float *__restrict__ cov_pre, const float *__restrict__ opac,
    const float *__restrict__ shs, const float *__restrict__ shs_rest, const float *__restrict__ colors_pre,
    const float *view, const float *proj, const float *campos, int W, int H, float tanx, float tany, float fx, float fy,
    int gx, int gy, int *__restrict__ radii, float2 *__restrict__ xy, float4 *__restrict__ conic_o,
    float4 *__restrict__ rgbd, uint32_t *__restrict__ tiles, uint8_t *__restrict__ clamped,
    uint32_t *__restrict__ dkey, uint32_t *__restrict__ gid, float4 *__restrict__ acc,
    uint8_t *__restrict__ visible) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < P;
    // every per-Gaussian input is in flight with the SH rows (one HBM round trip per block instead of
    // a chain of them: camera -> mean -> cull -> scale / rotation; the grid is ~1.5 blocks per CU)
    float3 p = make_float3(0.f, 0.f, 0.f), s = p;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    float op = 0.f;
    if (live) {
        p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
        if (!cov_pre) {
            s = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
            q = *reinterpret_cast<const float4 *>(rots + 4 * i);
        }
        op = opac[i];
    }
    Cam cam;
    load_cam(cam, view, proj, campos);
    [[maybe_unused]] const float *s_row = nullptr;
    if constexpr (STAGE) {
        __shared__ float s_sh[256 * SH_PAD];
        const int b0 = blockIdx.x * blockDim.x, nrow = min(256, P - b0);
        sh_stage_in(s_sh, shs, shs_rest, b0, nrow);
        __syncthreads();
        s_row = s_sh + threadIdx.x * SH_PAD;
    }
    if (!live) return;
    // zero this Gaussian's backward accumulator row (the blend backward adds into it): no memset
    // launch in the backward
    if constexpr (!FWD) acc[3 * i] = acc[3 * i + 1] = acc[3 * i + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
    radii[i] = 0;
    if constexpr (!FWD)
        if (visible) visible[i] = 0;  // render()'s visibility_filter (radii > 0), when asked for
    tiles[i] = 0;
    dkey[i] = 0xffffffffu;  // culled: sorts last, emits no pairs
    gid[i] = (uint32_t)i;
    float3 pv = xform43(cam.v, p);
    if (pv.z <= 0.2f) return;
    float c3[6];
    if (cov_pre) {
#pragma unroll
        for (int k = 0; k < 6; k++) c3[k] = cov_pre[6 * i + k];
    } else {
        cov3d(s, mod, q, c3);
    }
    Ewa e;
    ewa_T(pv, fx, fy, tanx, tany, cam.v, e);
    float3 c2 = cov2d(e, c3);
    float det = c2.x * c2.z - c2.y * c2.y;
    if (det == 0.f) return;
    float di = 1.f / det;
    float3 con = make_float3(c2.z * di, -c2.y * di, c2.x * di);
    float mid = 0.5f * (c2.x + c2.z);
    float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    float l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
    int rad = (int)ceilf(3.f * sqrtf(fmaxf(l1, l2)));
    float4 ph = xform44(cam.p, p);
    float pw = 1.f / (ph.w + 0.0000001f);
    float px = ((ph.x * pw + 1.f) * W - 1.f) * 0.5f;
    float py = ((ph.y * pw + 1.f) * H - 1.f) * 0.5f;
    int x0, y0, x1, y1;
    tile_rect(px, py, rad, gx, gy, x0, y0, x1, y1);
    int area = (x1 - x0) * (y1 - y0);
    if (area == 0) return;
    float3 rgb;
    uint8_t cl = 0;
    if (colors_pre) {
        rgb = make_float3(colors_pre[3 * i], colors_pre[3 * i + 1], colors_pre[3 * i + 2]);
    } else {
        float dx = p.x - cam.c[0], dy = p.y - cam.c[1], dz = p.z - cam.c[2];
        float n = sqrtf(dx * dx + dy * dy + dz * dz);
        float x = dx / n, y = dy / n, z = dz / n;
        const float *sh = STAGE ? s_row : shs + (size_t)i * M * 3;
        float r[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v = SH_C0 * sh[c];
            if (D > 0) {
                v = v - SH_C1 * y * sh[3 + c] + SH_C1 * z * sh[6 + c] - SH_C1 * x * sh[9 + c];
                if (D > 1) {
                    float xx = x * x, yy = y * y, zz = z * z, xy_ = x * y, yz = y * z, xz = x * z;
                    v = v + SH_C2_0 * xy_ * sh[12 + c] + SH_C2_1 * yz * sh[15 + c] +
                        SH_C2_2 * (2.f * zz - xx - yy) * sh[18 + c] + SH_C2_3 * xz * sh[21 + c] +
                        SH_C2_4 * (xx - yy) * sh[24 + c];
                    if (D > 2) {
                        v = v + SH_C3_0 * y * (3.f * xx - yy) * sh[27 + c] + SH_C3_1 * xy_ * z * sh[30 + c] +
                            SH_C3_2 * y * (4.f * zz - xx - yy) * sh[33 + c] +
                            SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy) * sh[36 + c] +
                            SH_C3_4 * x * (4.f * zz - xx - yy) * sh[39 + c] +
                            SH_C3_5 * z * (xx - yy) * sh[42 + c] + SH_C3_6 * x * (xx - 3.f * yy) * sh[45 + c];
                    }
                }
            }
            v += 0.5f;
            cl |= (v < 0.f) << c;
            r[c] = v < 0.f ? 0.f : v;
        }
        rgb = make_float3(r[0], r[1], r[2]);
    }
    radii[i] = rad;
    if constexpr (!FWD)
        if (visible) visible[i] = rad > 0;
    xy[i] = make_float2(px, py);
    conic_o[i] = make_float4(con.x, con.y, con.z, op);
    rgbd[i] = make_float4(rgb.x, rgb.y, rgb.z, pv.z);
    tiles[i] = (uint32_t)area;
    if constexpr (!FWD) clamped[i] = cl;
    dkey[i] = __float_as_uint(pv.z);  // depth > 0.2: float bits order as the values
}

__device__ inline void dR_dq(float4 q, const float dR[9], float4 &dq) {
    float r = q.x, x = q.y, y = q.z, z = q.w;
    dq.x = 2.f * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]);
    dq.y = 2.f * (y * dR[1] + z * dR[2] + y * dR[3] - r * dR[5] + z * dR[6] + r * dR[7]) - 4.f * x * (dR[4] + dR[8]);
    dq.z = 2.f * (x * dR[1] + r * dR[2] + x * dR[3] + z * dR[5] - r * dR[6] + z * dR[7]) - 4.f * y * (dR[0] + dR[8]);
    dq.w = 2.f * (-r * dR[1] + x * dR[2] + r * dR[3] + y * dR[5] + x * dR[6] + y * dR[7]) - 4.f * z * (dR[0] + dR[4]);
}

// one Gaussian's backward inputs, loaded before the block's SH staging so that they and the SH rows
// share one HBM round trip (the loads otherwise chained: accumulators -> radius -> scale / rotation)
struct PbIn {
    float4 a0, a1, a2;  // blend-backward accumulators (mx, my, cx, cy), (cz, op, r, g), (b, depth, dx, dy)
    float3 p, s;
    float4 q;
    int rad;
    uint8_t cl;
};

__device__ __forceinline__ void pb_load(PbIn &in, int i, const float *acc, const int *radii, const float *means3D,
                                        const float *scales, const float *rots, const float *cov_pre,
                                        const uint8_t *clamped) {
    const float *a = acc + (size_t)i * ACC_STRIDE;
    in.a0 = *reinterpret_cast<const float4 *>(a);
    in.a1 = *reinterpret_cast<const float4 *>(a + 4);
    in.a2 = *reinterpret_cast<const float4 *>(a + 8);
    in.rad = radii[i];
    in.p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    in.s = make_float3(0.f, 0.f, 0.f);
    in.q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!cov_pre) {
        in.s = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
        in.q = *reinterpret_cast<const float4 *>(rots + 4 * i);
    }
    in.cl = clamped ? clamped[i] : (uint8_t)0;
}

// STAGE (degree-3 SH rows, M = 16, 16-byte aligned tensors): the block's SH rows (contiguous in
// HBM) are read into LDS with coalesced 16-byte loads, and its SH gradient rows are written back the
// same way (one thread per Gaussian would otherwise store 48 scattered words per row: 3x the HBM
// write traffic in partial lines).
template <bool STAGE>
__device__ __forceinline__ void preprocess_bwd_one(
    int i, int D, int M, const float *__restrict__ means3D, const float *__restrict__ scales, float mod,
    const float *__restrict__ rots, const float *__restrict__ cov_pre, const float *__restrict__ shs,
    const float *view, const float *proj, const float *campos, int W, int H, float tanx, float tany,
    float fx, float fy, const int *__restrict__ radii, const uint8_t *__restrict__ clamped,
    const float *__restrict__ acc, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D,
    float *__restrict__ dL_ddens, float *__restrict__ dL_dcolors, float *__restrict__ dL_dopac,
    float *__restrict__ dL_dcov3D, float *__restrict__ dL_dshs, float *__restrict__ dL_dscales,
    float *__restrict__ dL_drots, float *s_row, float dsmul, const PbIn &in, const Cam &cam);

template <bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_bwd(
    int P, int D, int M, const float *__restrict__ means3D, const float *__restrict__ scales, float mod,
    const float *__restrict__ rots, const float *__restrict__ cov_pre, const float *__restrict__ shs,
    const float *view, const float *proj, const float *campos, int W, int H, float tanx, float tany,
    float fx, float fy, const int *__restrict__ radii, const uint8_t *__restrict__ clamped,
    const float *__restrict__ acc, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D,
    float *__restrict__ dL_ddens, float *__restrict__ dL_dcolors, float *__restrict__ dL_dopac,
    float *__restrict__ dL_dcov3D, float *__restrict__ dL_dshs, float *__restrict__ dL_dscales,
    float *__restrict__ dL_drots, const float *__restrict__ shs_rest, float *__restrict__ dL_dshs_rest, float dsmul) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    [[maybe_unused]] const int b0 = blockIdx.x * blockDim.x, nrow = min(256, P - b0);
    [[maybe_unused]] float *s_row = nullptr;
    PbIn in;
    if (i < P) pb_load(in, i, acc, radii, means3D, scales, rots, cov_pre, clamped);
    Cam cam;
    load_cam(cam, view, proj, campos);
    if constexpr (STAGE) {
        __shared__ float s_sh[256 * SH_PAD];
        s_row = s_sh + threadIdx.x * SH_PAD;
        sh_stage_in(s_sh, shs, shs_rest, b0, nrow);
        __syncthreads();
        if (i < P) preprocess_bwd_one<STAGE>(i, D, M, means3D, scales, mod, rots, cov_pre, shs, view, proj, campos, W, H,
                                             tanx, tany, fx, fy, radii, clamped, acc, dL_dmeans3D, dL_dmeans2D, dL_ddens,
                                             dL_dcolors, dL_dopac, dL_dcov3D, dL_dshs, dL_dscales, dL_drots, s_row, dsmul,
                                             in, cam);
        __syncthreads();
        sh_stage_out(s_sh, dL_dshs, dL_dshs_rest, b0, nrow);
    } else {
        if (i < P) preprocess_bwd_one<STAGE>(i, D, M, means3D, scales, mod, rots, cov_pre, shs, view, proj, campos, W, H,
                                             tanx, tany, fx, fy, radii, clamped, acc, dL_dmeans3D, dL_dmeans2D, dL_ddens,
                                             dL_dcolors, dL_dopac, dL_dcov3D, dL_dshs, dL_dscales, dL_drots, nullptr, dsmul,
                                             in, cam);
    }
}

// one Gaussian of k_preprocess_bwd; STAGE: its SH row is s_row in LDS, overwritten by its gradient
template <bool STAGE>
__device__ __forceinline__ void preprocess_bwd_one(
    int i, int D, int M, const float *__restrict__ means3D, const float *__restrict__ scales, float mod,
    const float *__restrict__ rots, const float *__restrict__ cov_pre, const float *__restrict__ shs,
    const float *view, const float *proj, const float *campos, int W, int H, float tanx, float tany,
    float fx, float fy, const int *__restrict__ radii, const uint8_t *__restrict__ clamped,
    const float *__restrict__ acc, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D,
    float *__restrict__ dL_ddens, float *__restrict__ dL_dcolors, float *__restrict__ dL_dopac,
    float *__restrict__ dL_dcov3D, float *__restrict__ dL_dshs, float *__restrict__ dL_dscales,
    float *__restrict__ dL_drots, float *s_row, float dsmul, const PbIn &in, const Cam &cam) {
    const float4 a0 = in.a0, a1 = in.a1, a2 = in.a2;
    // a0 = (mx, my, cx, cy), a1 = (cz, op, r, g), a2 = (b, depth, dx, dy)
    dL_dmeans2D[3 * i] = a0.x;
    dL_dmeans2D[3 * i + 1] = a0.y;
    dL_dmeans2D[3 * i + 2] = 0.f;
    dL_ddens[3 * i] = a2.z;
    dL_ddens[3 * i + 1] = a2.w;
    dL_ddens[3 * i + 2] = 0.f;
    dL_dopac[i] = a1.y;
    if (dL_dcolors) {
        dL_dcolors[3 * i] = a1.z;
        dL_dcolors[3 * i + 1] = a1.w;
        dL_dcolors[3 * i + 2] = a2.x;
    }
    const bool vis = in.rad > 0;
    const float3 p = in.p;
    float dm0 = 0.f, dm1 = 0.f, dm2 = 0.f;
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float c3[6];
    const float3 s3 = in.s;
    const float4 q = in.q;
    if (vis) {
        if (cov_pre) {
#pragma unroll
            for (int k = 0; k < 6; k++) c3[k] = cov_pre[6 * i + k];
        } else {
            cov3d(s3, mod, q, c3);
        }
        float3 tv = xform43(cam.v, p);
        Ewa e;
        ewa_T(tv, fx, fy, tanx, tany, cam.v, e);
        const float *Tm = e.T;
        float3 c2 = cov2d(e, c3);
        float A = c2.x, B = c2.y, Cc = c2.z;
        float den = A * Cc - B * B;
        float d2i = 1.f / (den * den + 0.0000001f);
        float gcx = a0.z, gcy = a0.w, gcz = a1.x;
        float dLa = 0.f, dLb = 0.f, dLc = 0.f;
        if (d2i != 0.f) {
            dLa = d2i * (-Cc * Cc * gcx + 2.f * B * Cc * gcy + (den - A * Cc) * gcz);
            dLc = d2i * (-A * A * gcz + 2.f * A * B * gcy + (den - A * Cc) * gcx);
            dLb = d2i * 2.f * (B * Cc * gcx - (den + 2.f * B * B) * gcy + A * B * gcz);
        }
        dcov[0] = Tm[0] * Tm[0] * dLa + Tm[0] * Tm[3] * dLb + Tm[3] * Tm[3] * dLc;
        dcov[3] = Tm[1] * Tm[1] * dLa + Tm[1] * Tm[4] * dLb + Tm[4] * Tm[4] * dLc;
        dcov[5] = Tm[2] * Tm[2] * dLa + Tm[2] * Tm[5] * dLb + Tm[5] * Tm[5] * dLc;
        dcov[1] = 2.f * Tm[0] * Tm[1] * dLa + (Tm[0] * Tm[4] + Tm[1] * Tm[3]) * dLb + 2.f * Tm[3] * Tm[4] * dLc;
        dcov[2] = 2.f * Tm[0] * Tm[2] * dLa + (Tm[0] * Tm[5] + Tm[2] * Tm[3]) * dLb + 2.f * Tm[3] * Tm[5] * dLc;
        dcov[4] = 2.f * Tm[2] * Tm[1] * dLa + (Tm[1] * Tm[5] + Tm[2] * Tm[4]) * dLb + 2.f * Tm[4] * Tm[5] * dLc;
        float V[9] = {c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]};
        float dT[6];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float v0 = V[k * 3] * Tm[0] + V[k * 3 + 1] * Tm[1] + V[k * 3 + 2] * Tm[2];
            float v1 = V[k * 3] * Tm[3] + V[k * 3 + 1] * Tm[4] + V[k * 3 + 2] * Tm[5];
            dT[k] = 2.f * v0 * dLa + v1 * dLb;
            dT[3 + k] = 2.f * v1 * dLc + v0 * dLb;
        }
        const float *vm = cam.v;
        // W rows: W0 = (vm0, vm4, vm8), W1 = (vm1, vm5, vm9), W2 = (vm2, vm6, vm10)
        float dJ00 = vm[0] * dT[0] + vm[4] * dT[1] + vm[8] * dT[2];
        float dJ02 = vm[2] * dT[0] + vm[6] * dT[1] + vm[10] * dT[2];
        float dJ11 = vm[1] * dT[3] + vm[5] * dT[4] + vm[9] * dT[5];
        float dJ12 = vm[2] * dT[3] + vm[6] * dT[4] + vm[10] * dT[5];
        float tz = e.tz;
        float tz2 = 1.f / (tz * tz), tz3 = tz2 / tz;
        float dtx = e.mx * -fx * tz2 * dJ02;
        float dty = e.my * -fy * tz2 * dJ12;
        float dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.f * fx * e.tx) * tz3 * dJ02 + (2.f * fy * e.ty) * tz3 * dJ12;
        dtz += a2.y;  // depth output: depth = t.z
        dm0 += vm[0] * dtx + vm[1] * dty + vm[2] * dtz;
        dm1 += vm[4] * dtx + vm[5] * dty + vm[6] * dtz;
        dm2 += vm[8] * dtx + vm[9] * dty + vm[10] * dtz;
        // projection: mean2D (NDC) -> mean3D
        const float *pj = cam.p;
        float4 ph = xform44(pj, p);
        float mw = 1.f / (ph.w + 0.0000001f);
        float mul1 = ph.x * mw * mw, mul2 = ph.y * mw * mw;
        float gx_ = a0.x, gy_ = a0.y;
        dm0 += (pj[0] * mw - pj[3] * mul1) * gx_ + (pj[1] * mw - pj[3] * mul2) * gy_;
        dm1 += (pj[4] * mw - pj[7] * mul1) * gx_ + (pj[5] * mw - pj[7] * mul2) * gy_;
        dm2 += (pj[8] * mw - pj[11] * mul1) * gx_ + (pj[9] * mw - pj[11] * mul2) * gy_;
    }
    // SH backward (also writes zeros for culled Gaussians)
    if (shs) {
        float *dsh = STAGE ? s_row : dL_dshs + (size_t)i * M * 3;
        if (!vis) {
            for (int k = 0; k < M * 3; k++) dsh[k] = 0.f;
        } else {
            float shr[STAGE ? SH_ROW : 1];  // STAGE: the row in registers (the LDS row is overwritten)
            const float *sh = shs + (size_t)i * M * 3;
            if constexpr (STAGE) {
#pragma unroll
                for (int k = 0; k < SH_ROW; k++) shr[k] = s_row[k];
                sh = shr;
            }
            float vx = p.x - cam.c[0], vy = p.y - cam.c[1], vz = p.z - cam.c[2];
            float n = sqrtf(vx * vx + vy * vy + vz * vz);
            float x = vx / n, y = vy / n, z = vz / n;
            const uint8_t cl = in.cl;
            float g3[3] = {(cl & 1) ? 0.f : a1.z, (cl & 2) ? 0.f : a1.w, (cl & 4) ? 0.f : a2.x};
            float ddx = 0.f, ddy = 0.f, ddz = 0.f;
            float xx = x * x, yy = y * y, zz = z * z, xy_ = x * y, yz = y * z, xz = x * z;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float g = g3[c];
#define SHV(k) sh[(k) * 3 + c]
                dsh[c] = SH_C0 * g;
                float gxx = 0.f, gyy = 0.f, gzz = 0.f;
                if (D > 0) {
                    dsh[3 + c] = -SH_C1 * y * g;
                    dsh[6 + c] = SH_C1 * z * g;
                    dsh[9 + c] = -SH_C1 * x * g;
                    gxx = -SH_C1 * SHV(3);
                    gyy = -SH_C1 * SHV(1);
                    gzz = SH_C1 * SHV(2);
                    if (D > 1) {
                        dsh[12 + c] = SH_C2_0 * xy_ * g;
                        dsh[15 + c] = SH_C2_1 * yz * g;
                        dsh[18 + c] = SH_C2_2 * (2.f * zz - xx - yy) * g;
                        dsh[21 + c] = SH_C2_3 * xz * g;
                        dsh[24 + c] = SH_C2_4 * (xx - yy) * g;
                        gxx += SH_C2_0 * y * SHV(4) + SH_C2_2 * 2.f * -x * SHV(6) + SH_C2_3 * z * SHV(7) + SH_C2_4 * 2.f * x * SHV(8);
                        gyy += SH_C2_0 * x * SHV(4) + SH_C2_1 * z * SHV(5) + SH_C2_2 * 2.f * -y * SHV(6) + SH_C2_4 * 2.f * -y * SHV(8);
                        gzz += SH_C2_1 * y * SHV(5) + SH_C2_2 * 2.f * 2.f * z * SHV(6) + SH_C2_3 * x * SHV(7);
                        if (D > 2) {
                            dsh[27 + c] = SH_C3_0 * y * (3.f * xx - yy) * g;
                            dsh[30 + c] = SH_C3_1 * xy_ * z * g;
                            dsh[33 + c] = SH_C3_2 * y * (4.f * zz - xx - yy) * g;
                            dsh[36 + c] = SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy) * g;
                            dsh[39 + c] = SH_C3_4 * x * (4.f * zz - xx - yy) * g;
                            dsh[42 + c] = SH_C3_5 * z * (xx - yy) * g;
                            dsh[45 + c] = SH_C3_6 * x * (xx - 3.f * yy) * g;
                            gxx += SH_C3_0 * SHV(9) * 3.f * 2.f * xy_ + SH_C3_1 * SHV(10) * yz + SH_C3_2 * SHV(11) * -2.f * xy_ +
                                   SH_C3_3 * SHV(12) * -3.f * 2.f * xz + SH_C3_4 * SHV(13) * (-3.f * xx + 4.f * zz - yy) +
                                   SH_C3_5 * SHV(14) * 2.f * xz + SH_C3_6 * SHV(15) * 3.f * (xx - yy);
                            gyy += SH_C3_0 * SHV(9) * 3.f * (xx - yy) + SH_C3_1 * SHV(10) * xz +
                                   SH_C3_2 * SHV(11) * (-3.f * yy + 4.f * zz - xx) + SH_C3_3 * SHV(12) * -3.f * 2.f * yz +
                                   SH_C3_4 * SHV(13) * -2.f * xy_ + SH_C3_5 * SHV(14) * -2.f * yz + SH_C3_6 * SHV(15) * -3.f * 2.f * xy_;
                            gzz += SH_C3_1 * SHV(10) * xy_ + SH_C3_2 * SHV(11) * 4.f * 2.f * yz +
                                   SH_C3_3 * SHV(12) * 3.f * (2.f * zz - xx - yy) + SH_C3_4 * SHV(13) * 4.f * 2.f * xz +
                                   SH_C3_5 * SHV(14) * (xx - yy);
                        }
                    }
                }
#undef SHV
                ddx += gxx * g;
                ddy += gyy * g;
                ddz += gzz * g;
            }
            int kmax = (D + 1) * (D + 1);
            for (int k = kmax; k < M; k++) {
                dsh[3 * k] = 0.f;
                dsh[3 * k + 1] = 0.f;
                dsh[3 * k + 2] = 0.f;
            }
            float s2 = vx * vx + vy * vy + vz * vz;
            float inv32 = 1.f / sqrtf(s2 * s2 * s2);
            dm0 += ((s2 - vx * vx) * ddx - vy * vx * ddy - vz * vx * ddz) * inv32;
            dm1 += (-vx * vy * ddx + (s2 - vy * vy) * ddy - vz * vy * ddz) * inv32;
            dm2 += (-vx * vz * ddx - vy * vz * ddy + (s2 - vz * vz) * ddz) * inv32;
        }
    }
    dL_dmeans3D[3 * i] = dm0;
    dL_dmeans3D[3 * i + 1] = dm1;
    dL_dmeans3D[3 * i + 2] = dm2;
    if (cov_pre) {
        if (dL_dcov3D)
            for (int k = 0; k < 6; k++) dL_dcov3D[6 * i + k] = dcov[k];
    } else {
        float ds0 = 0.f, ds1 = 0.f, ds2 = 0.f;
        float4 dq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vis) {
            float R[9];
            quat_to_R(q, R);
            float sp[3] = {mod * s3.x, mod * s3.y, mod * s3.z};
            float G[9] = {dcov[0], 0.5f * dcov[1], 0.5f * dcov[2], 0.5f * dcov[1], dcov[3], 0.5f * dcov[4],
                          0.5f * dcov[2], 0.5f * dcov[4], dcov[5]};
            float L[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) L[r * 3 + k] = R[r * 3 + k] * sp[k];
            float dRm[9];
            float ds[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float acc_s = 0.f;
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    float dl = 2.f * (G[r * 3] * L[k] + G[r * 3 + 1] * L[3 + k] + G[r * 3 + 2] * L[6 + k]);
                    acc_s += dl * R[r * 3 + k];
                    dRm[r * 3 + k] = dl * sp[k];
                }
                ds[k] = acc_s * dsmul;  // upstream: dL/d(mod s) (dsmul = 1); exact: dL/ds (dsmul = mod)
            }
            ds0 = ds[0]; ds1 = ds[1]; ds2 = ds[2];
            dR_dq(q, dRm, dq);
        }
        dL_dscales[3 * i] = ds0;
        dL_dscales[3 * i + 1] = ds1;
        dL_dscales[3 * i + 2] = ds2;
        *reinterpret_cast<float4 *>(dL_drots + 4 * i) = dq;
    }
}

__global__ __launch_bounds__(256) void k_mark_visible(int P, const float *__restrict__ means3D, const float *view,
                                                      uint8_t *__restrict__ visible) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    float3 pv = make_float3(0.f, 0.f, view[2] * p.x + view[6] * p.y + view[10] * p.z + view[14]);
    visible[i] = pv.z > 0.2f;
}

}  // namespace dgs
