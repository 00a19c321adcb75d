// Robustness check of the host JPEG front end (deformable-3d-gaussians_amd/csrc/jpeg_decode.h) on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -I deformable-3d-gaussians_amd/csrc tools/jpeg_host_check.cpp -o jpeg_host_check   (one line)
//   ./jpeg_host_check file.jpg [file.jpg ...]
//
// For each file: the file itself, every truncation of it, and the file with each byte in turn XOR-ed with
// 0xFF go through header + coefficients. Every input is copied into a heap block of exactly its size, so a
// read outside the input is a heap-buffer-overflow for AddressSanitizer. Every call must return 0 or -1, a
// failure must leave a message, and a success must have filled a buffer of exactly the size the header
// announces. Prints one line per file; exit status 1 when a rule was broken. tests/test_jpeg_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_decode.h"

static long long g_ok = 0, g_refused = 0, g_broken = 0;

static void one(const uint8_t *src, size_t n) {
    uint8_t *data = (uint8_t *)std::malloc(n ? n : 1);  // exactly n bytes: no slack behind the input
    if (n) std::memcpy(data, src, n);
    dgs_jpeg::Info info;
    char err[200];
    err[0] = 0;
    int rc = dgs_jpeg::header(data, n, &info, err, sizeof(err));
    if (rc == 0) {
        size_t blocks = 0;
        for (int c = 0; c < 3; c++) blocks += (size_t)info.blocks_w[c] * (size_t)info.blocks_h[c];
        if (info.width < 1 || info.height < 1 || blocks == 0 || blocks > (size_t)1 << 24) {
            // a mutated header may announce up to 65535^2 pixels: the check does not allocate gigabytes
            if (blocks <= (size_t)1 << 24) g_broken++;
            else g_refused++;
            std::free(data);
            return;
        }
        int16_t *coef = (int16_t *)std::malloc(blocks * 64 * sizeof(int16_t));
        rc = dgs_jpeg::coefficients(data, n, &info, coef, blocks * 64, err, sizeof(err));
        std::free(coef);
    }
    if (rc == 0) g_ok++;
    else if (rc == -1 && err[0]) g_refused++;
    else g_broken++;
    std::free(data);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s file.jpg [file.jpg ...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> buf;
        uint8_t chunk[4096];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
        std::fclose(f);
        const long long ok0 = g_ok, ref0 = g_refused, br0 = g_broken;
        one(buf.data(), buf.size());
        const bool whole_ok = g_ok == ok0 + 1;
        for (size_t cut = 0; cut < buf.size(); cut++) one(buf.data(), cut);
        for (size_t i = 0; i < buf.size(); i++) {
            buf[i] ^= 0xFF;
            one(buf.data(), buf.size());
            buf[i] ^= 0xFF;
        }
        std::printf("%s: %zu bytes, whole file %s, variants decoded %lld, refused %lld, broken %lld\n", argv[a], buf.size(),
                    whole_ok ? "decoded" : "refused", g_ok - ok0, g_refused - ref0, g_broken - br0);
    }
    return g_broken ? 1 : 0;
}
