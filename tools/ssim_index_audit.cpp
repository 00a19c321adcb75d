// Host audit of the SSIM tile kernels' index arithmetic: the loss (csrc/ssim.hip: k_ssim_fwd / k_ssim_final /
// k_ssim_bwd; VERDICT r4 "close the r4v abort from the evidence in hand") and the batched image metrics
// (csrc/metrics.hip: k_tile<false>, k_tile<true>, k_pool). Every thread of every workgroup is replayed on the
// CPU with the kernels' own index expressions and every global and LDS address each thread forms is checked
// against the extent of its buffer. The tile constants, the tile load and the partial slot are written once,
// in csrc/ssim_tile.h: that header is the one place audit_load_tile, audit_tile_sums and the constants below
// must match term for term; the row and column passes (audit_row_pass / audit_col_pass) and what each kernel
// adds around them (origin, guards, its own reads and writes, the buffer extents of
// dgs_l1_ssim_scratch_floats and of metrics.hip's make_layout) are replayed from ssim.hip and metrics.hip.
// Usage: ssim_index_audit <group> ...; a group is
//   C H W            the three loss kernels on a (C, H, W) image
//   same P H W       k_tile<false> (zero-padded pass: PSNR + SSIM) on P = F * C planes of H x W
//   ms P H W         the MS-SSIM pyramid: k_tile<true> on each of the five levels and the four k_pool between
// exit 0 = every address in bounds. Built and run by tests/test_ssim_index_audit.py for the shapes of
// tests/test_gpu_loss.py and tests/test_gpu_image_metrics.py.
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>

namespace {
constexpr int T = 32, R = 5, S = T + 2 * R, SP = S + 1, HP = T + 1, HX = 8, VY = 4;
constexpr int LEVELS = 5;

long long g_checks = 0;
int g_fail = 0;

void chk(const char *what, long long idx, long long n, int c, int bx, int by, int tid) {
    ++g_checks;
    if (idx < 0 || idx >= n) {
        if (g_fail++ < 20)
            std::fprintf(stderr, "OUT OF BOUNDS %s: index %lld not in [0, %lld) (c %d block %d,%d thread %d)\n", what,
                         idx, n, c, bx, by, tid);
    }
}

int div_up(int a, int b) { return (a + b - 1) / b; }
int imin(int a, int b) { return a < b ? a : b; }

// load_tile<NM>: element e of the 42x42 input tile with origin (ox, oy), global read src[q][p] only when
// `in`; src[q] = buffer + base[q], checked against the region the map lives in (region_n)
void audit_load_tile(int NM, const long long *base, long long region_n, int H, int W, int ox, int oy, int c, int bx,
                     int by) {
    const int NIT = (S * S + 255) / 256;
    for (int tid = 0; tid < 256; tid++)
        for (int it = 0; it < NIT; it++) {
            const int e = tid + 256 * it;
            const int ly = e / S, lx = e - ly * S;
            const int gy = oy + ly, gx = ox + lx;
            const bool in = e < S * S && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const long long p = in ? (long long)gy * W + gx : 0;
            if (in)
                for (int q = 0; q < NM; q++) chk("load_tile global", base[q] + p, region_n, c, bx, by, tid);
            if (e < S * S)
                for (int q = 0; q < NM; q++) chk("load_tile LDS", ((long long)q * S + ly) * SP + lx, (long long)NM * S * SP, c, bx, by, tid);
        }
}

// row pass (k_ssim_fwd, k_tile: 2 input maps -> 5 row-filtered; k_ssim_bwd: 3 -> 3)
void audit_row_pass(int NIN, int NOUT, int c, int bx, int by) {
    for (int tid = 0; tid < 256; tid++) {
        if (!(tid < S * (T / HX))) continue;
        const int ly = tid / (T / HX), lx0 = (tid % (T / HX)) * HX;
        for (int m = 0; m < NIN; m++)
            for (int k = 0; k < HX + 10; k++)
                chk("row pass LDS read", ((long long)m * S + ly) * SP + lx0 + k, (long long)NIN * S * SP, c, bx, by, tid);
        for (int m = 0; m < NOUT; m++)
            for (int j = 0; j < HX; j++)
                chk("row pass LDS write", ((long long)m * S + ly) * HP + lx0 + j, (long long)NOUT * S * HP, c, bx, by, tid);
        // the row index must stay inside a row of the padded array (no wrap into the next row)
        if (lx0 + HX + 10 - 1 >= SP) chk("row pass read within row", lx0 + HX + 9, SP, c, bx, by, tid);
        if (lx0 + HX - 1 >= HP) chk("row pass write within row", lx0 + HX - 1, HP, c, bx, by, tid);
    }
}

void audit_col_pass(int NM, int c, int bx, int by) {
    for (int tid = 0; tid < 256; tid++) {
        const int lx = tid % T, ly0 = (tid / T) * VY;
        for (int m = 0; m < NM; m++)
            for (int k = 0; k < VY + 10; k++) {
                chk("column pass LDS read", ((long long)m * S + ly0 + k) * HP + lx, (long long)NM * S * HP, c, bx, by, tid);
                chk("column pass row", ly0 + k, S, c, bx, by, tid);
            }
    }
}

// tile_sums: the wave leaders' red[.][tid >> 6] and thread 0's slot 2 * block + 1 of `partial` (partial_n floats)
void audit_tile_sums(long long partial_n, int z, int gx, int gy, int bx, int by) {
    for (int tid = 0; tid < 256; tid++)
        if ((tid & 63) == 0) chk("tile_sums red", tid >> 6, 4, z, bx, by, tid);
    const long long blk = ((long long)z * gy + by) * gx + bx;
    chk("tile_sums partial write", 2 * blk + 1, partial_n, z, bx, by, 0);
}

int audit_loss(int C, int H, int W) {
    const long long plane = (long long)H * W;
    const int gx = div_up(W, T), gy = div_up(H, T);
    const long long nb = (long long)C * gx * gy;
    const long long scratch_n = 3LL * C * H * W + 2 * nb;  // dgs_l1_ssim_scratch_floats
    const long long img_n = (long long)C * plane;
    for (int c = 0; c < C; c++)
        for (int by = 0; by < gy; by++)
            for (int bx = 0; bx < gx; bx++) {
                const int x0 = bx * T, y0 = by * T;
                // ---- k_ssim_fwd ----
                // src planes I + c*plane, G + c*plane: global index = c*plane + p
                const long long fb[2] = {c * plane, c * plane};  // I + c*plane, G + c*plane
                audit_load_tile(2, fb, img_n, H, W, x0 - R, y0 - R, c, bx, by);
                audit_row_pass(2, 5, c, bx, by);
                audit_col_pass(5, c, bx, by);
                for (int tid = 0; tid < 256; tid++) {
                    const int lx = tid % T, ly0 = (tid / T) * VY;
                    const int x = x0 + lx;
                    for (int j = 0; j < VY; j++) {
                        const int y = y0 + ly0 + j;
                        if (x < W && y < H) {
                            const long long p = (long long)y * W + x;
                            for (int m = 0; m < 3; m++) chk("fwd maps write", (3LL * c + m) * plane + p, scratch_n, c, bx, by, tid);
                            chk("fwd maps region", (3LL * c + 2) * plane + p, 3LL * C * H * W, c, bx, by, tid);
                            chk("fwd l1 LDS read", ((long long)0 * S + ly0 + j + R) * SP + lx + R, 2LL * S * SP, c, bx, by, tid);
                            chk("fwd l1 LDS read G", ((long long)1 * S + ly0 + j + R) * SP + lx + R, 2LL * S * SP, c, bx, by, tid);
                        }
                    }
                }
                audit_tile_sums(2 * nb, c, gx, gy, bx, by);  // partial = scratch + 3*C*H*W, 2*nb floats
                // ---- k_ssim_bwd ----
                const long long bb[3] = {3LL * c * plane, (3LL * c + 1) * plane, (3LL * c + 2) * plane};  // maps
                audit_load_tile(3, bb, 3LL * C * H * W, H, W, x0 - R, y0 - R, c, bx, by);
                audit_row_pass(3, 3, c, bx, by);
                audit_col_pass(3, c, bx, by);
                for (int tid = 0; tid < 256; tid++) {
                    const int lx = tid % T, ly0 = (tid / T) * VY;
                    const int x = x0 + lx;
                    for (int j = 0; j < VY; j++) {
                        const int y = y0 + ly0 + j;
                        if (x >= W || y >= H) continue;
                        const long long p = c * plane + (long long)y * W + x;
                        chk("bwd I/G read, grad write", p, img_n, c, bx, by, tid);
                    }
                }
            }
    // ---- k_ssim_final: one workgroup of 1024, reads partial[2 i + 1] for i < nblocks ----
    for (int t = 0; t < 1024; t++) {
        for (long long i = t; i < nb; i += 1024) chk("final partial read", 3LL * C * H * W + 2 * i + 1, scratch_n, -1, 0, 0, t);
        if ((t & 63) == 0) chk("final red", t >> 6, 16, -1, 0, 0, t);
    }
    return g_fail;
}

// ---- metrics.hip ----
// k_tile<VALID> on `planes` planes of h x w; its partial sums have make_layout's extent for the pass,
// 2 * planes * tiles(oh, ow)
void audit_tile(bool VALID, int planes, int h, int w) {
    const long long plane = (long long)h * w, img_n = planes * plane;
    const int ow = VALID ? w - 2 * R : w, oh = VALID ? h - 2 * R : h;
    const int gx = div_up(ow, T), gy = div_up(oh, T);           // the launch's grid
    const long long partial_n = 2LL * planes * (div_up(oh, T) * div_up(ow, T));  // make_layout: 2 * planes * tiles()
    for (int z = 0; z < planes; z++)
        for (int by = 0; by < gy; by++)
            for (int bx = 0; bx < gx; bx++) {
                const int x0 = bx * T, y0 = by * T;
                const int ox = VALID ? x0 : x0 - R, oy = VALID ? y0 : y0 - R;
                if (VALID) {
                    const long long pc = (long long)imin(oy + S / 2, h - 1) * w + imin(ox + S / 2, w - 1);
                    chk("tile centre pixel", z * plane + pc, img_n, z, bx, by, -1);
                }
                const long long base[2] = {z * plane, z * plane};  // X + z*plane, Y + z*plane
                audit_load_tile(2, base, img_n, h, w, ox, oy, z, bx, by);
                audit_row_pass(2, 5, z, bx, by);
                audit_col_pass(5, z, bx, by);
                for (int tid = 0; tid < 256; tid++) {
                    const int lx = tid % T, ly0 = (tid / T) * VY;
                    const int x = x0 + lx;
                    for (int j = 0; j < VY; j++) {
                        const int y = y0 + ly0 + j;
                        if (x < ow && y < oh && !VALID)
                            for (int q = 0; q < 2; q++)
                                chk("tile squared-error LDS read", ((long long)q * S + ly0 + j + R) * SP + lx + R, 2LL * S * SP, z, bx, by, tid);
                    }
                }
                audit_tile_sums(partial_n, z, gx, gy, bx, by);
            }
}

// k_pool: (h, w) -> (ph, pw), 64 x 4 outputs per workgroup; four source reads (when inside), one destination
void audit_pool(int planes, int h, int w, int ph, int pw) {
    const long long src_n = (long long)planes * h * w, dst_n = (long long)planes * ph * pw;
    for (int z = 0; z < planes; z++)
        for (int by = 0; by < div_up(ph, 4); by++)
            for (int bx = 0; bx < div_up(pw, 64); bx++)
                for (int tid = 0; tid < 256; tid++) {
                    const int ox = bx * 64 + (tid & 63), oy = by * 4 + (tid >> 6);
                    if (ox >= pw || oy >= ph) continue;
                    const long long src = z * ((long long)h * w), dst = z * ((long long)ph * pw) + (long long)oy * pw + ox;
                    const int ix = 2 * ox - (w & 1), iy = 2 * oy - (h & 1);
                    for (int k = 0; k < 4; k++) {
                        const int gx = ix + (k & 1), gy = iy + (k >> 1);
                        const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
                        if (in) chk("pool source read", src + (long long)gy * w + gx, src_n, z, bx, by, tid);
                    }
                    chk("pool destination write", dst, dst_n, z, bx, by, tid);
                }
}

int pooled(int s) { return (s + 2 * (s & 1) - 2) / 2 + 1; }  // metrics.hip

void report(const char *what, long long before, int f0) {
    std::printf("%s: %lld addresses checked, %d out of bounds\n", what, g_checks - before, g_fail - f0);
}
}  // namespace

int main(int argc, char **argv) {
    char what[128];
    int a = 1;
    while (a < argc) {
        const bool same = !std::strcmp(argv[a], "same"), ms = !std::strcmp(argv[a], "ms");
        if (same || ms) a++;
        if (a + 2 >= argc) break;
        const int C = std::atoi(argv[a]), H = std::atoi(argv[a + 1]), W = std::atoi(argv[a + 2]);
        a += 3;
        long long before = g_checks;
        int f0 = g_fail;
        if (same) {
            audit_tile(false, C, H, W);
            std::snprintf(what, sizeof what, "k_tile<false> %dx%d (%d planes)", H, W, C);
            report(what, before, f0);
        } else if (ms) {
            int h = H, w = W;
            for (int l = 0; l < LEVELS; l++) {
                before = g_checks, f0 = g_fail;
                audit_tile(true, C, h, w);
                std::snprintf(what, sizeof what, "k_tile<true> level %d %dx%d (%d planes)", l, h, w, C);
                report(what, before, f0);
                if (l + 1 == LEVELS) break;
                const int ph = pooled(h), pw = pooled(w);
                before = g_checks, f0 = g_fail;
                audit_pool(C, h, w, ph, pw);
                std::snprintf(what, sizeof what, "k_pool %dx%d -> %dx%d (%d planes)", h, w, ph, pw, C);
                report(what, before, f0);
                h = ph, w = pw;
            }
        } else {
            audit_loss(C, H, W);
            std::snprintf(what, sizeof what, "shape (%d,%d,%d)", C, H, W);
            report(what, before, f0);
        }
    }
    if (a != argc || argc < 4) {
        std::fprintf(stderr, "usage: %s <C H W | same P H W | ms P H W> ...\n", argv[0]);
        return 2;
    }
    return g_fail ? 1 : 0;
}
