// Host JPEG front end: marker parsing and Huffman decoding of baseline / extended sequential JPEG files
// down to quantised coefficients (deformgs/jpeg.py is the same thing in Python). Everything per pixel is
// the device's work (jpeg.hip). Plain C++17, header-only, no HIP includes, no globals: thread-safe. The zigzag
// order is jpeg_tables.h's.
//
// This parser reads user files: every byte is fetched through a bounds check (Reader::byte / Bits::fill),
// every table index comes from a masked or range-checked value, and every failure is a message, never a
// read past the input.
//
// Read: SOF0 / SOF1, 8 bits, three components (YCbCr) in one interleaved scan, chroma 1x1 with luma 1x1,
// 2x1 or 2x2, DRI / RSTn, any number of DQT / DHT segments, APPn / COM skipped, 0xFF00 stuffing and fill
// bytes. Refused, with the reason: progressive, lossless, arithmetic, 12-bit, grayscale, CMYK / YCCK, Adobe
// transform 0, other sampling layouts, multi-scan files, truncated or corrupt entropy data.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "jpeg_tables.h"  // ZIGZAG

namespace dgs_jpeg {

// include/dgs.h dgs_jpeg_info, field for field
struct Info {
    int32_t width, height;
    int32_t hs, vs;        // luma sampling factors
    int32_t blocks_w[3];   // 8x8 blocks per component, padded to whole MCUs
    int32_t blocks_h[3];
    uint16_t qt[3][64];    // per component, natural order
};

constexpr int MAX_DIM = 65535;

struct Huffman {
    bool defined = false;
    uint8_t look_len[256];   // code length when the code fits the next 8 bits, else 0
    uint8_t look_sym[256];
    int32_t maxcode[18];     // largest code of each length (-1: none)
    int32_t valptr[17];      // index of the first symbol of each length
    int32_t mincode[17];
    uint8_t symbols[256];
};

struct Parsed {
    Info info;
    Huffman dc[3], ac[3];    // per component
    int restart = 0;
    int mcus_w = 0, mcus_h = 0;
    size_t scan_offset = 0;  // first byte of the entropy data
};

inline int fail(std::string &err, const std::string &msg) {
    err = "JPEG: " + msg;
    return -1;
}

inline int build_huffman(const uint8_t *counts, const uint8_t *symbols, int total, Huffman &h, std::string &err) {
    std::memset(h.look_len, 0, sizeof(h.look_len));
    std::memset(h.look_sym, 0, sizeof(h.look_sym));
    std::memset(h.symbols, 0, sizeof(h.symbols));
    std::memcpy(h.symbols, symbols, (size_t)total);
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        h.valptr[len] = k;
        h.mincode[len] = code;
        const int n = counts[len - 1];
        if (code + n > (1 << len)) return fail(err, "bad Huffman table (code lengths overflow)");
        if (len <= 8)
            for (int i = 0; i < n; i++) {
                const int first = (code + i) << (8 - len);
                for (int j = 0; j < (1 << (8 - len)); j++) {
                    h.look_len[first + j] = (uint8_t)len;
                    h.look_sym[first + j] = symbols[k + i];
                }
            }
        k += n;
        code += n;
        h.maxcode[len] = n ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.defined = true;
    return 0;
}

// Everything up to and including the SOS header.
inline int parse(const uint8_t *data, size_t n, Parsed &out, std::string &err) {
    if (!data || n < 2 || data[0] != 0xFF || data[1] != 0xD8) return fail(err, "not a JPEG file (no SOI)");
    size_t pos = 2;
    uint16_t qtabs[4][64];
    bool have_q[4] = {false, false, false, false};
    Huffman *huff = new Huffman[8];  // [tc * 4 + th]
    struct Guard {
        Huffman *p;
        ~Guard() { delete[] p; }
    } guard{huff};
    bool have_frame = false, jfif = false;
    int adobe = -1;
    int width = 0, height = 0;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0};
    out.restart = 0;
    for (;;) {
        if (pos >= n) return fail(err, "truncated before the scan (no SOS)");
        if (data[pos] != 0xFF) return fail(err, "expected a marker at byte " + std::to_string(pos));
        while (pos < n && data[pos] == 0xFF) pos++;  // fill bytes
        if (pos >= n) return fail(err, "truncated inside a marker");
        const int m = data[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone markers
        if (m == 0xD9) return fail(err, "EOI before any scan");
        if (m == 0x00) return fail(err, "stuffed byte outside entropy data at byte " + std::to_string(pos - 2));
        if (n - pos < 2) return fail(err, "truncated segment length");
        const size_t length = ((size_t)data[pos] << 8) | data[pos + 1];
        if (length < 2 || length > n - pos) return fail(err, "truncated segment");
        const uint8_t *seg = data + pos + 2;
        const size_t sl = length - 2;
        pos += length;
        switch (m) {
        case 0xC2: return fail(err, "progressive JPEG (SOF2) is unsupported (baseline / extended sequential Huffman only)");
        case 0xC3: case 0xC7: case 0xCB: case 0xCF:
            return fail(err, "lossless JPEG is unsupported (baseline / extended sequential Huffman only)");
        case 0xC5: case 0xC6:
            return fail(err, "differential (hierarchical) JPEG is unsupported (baseline / extended sequential Huffman only)");
        case 0xC9: case 0xCA: case 0xCD: case 0xCE: case 0xCC:
            return fail(err, "arithmetic coding is unsupported (baseline / extended sequential Huffman only)");
        case 0xC0: case 0xC1: {
            if (have_frame) return fail(err, "two frame headers");
            if (sl < 6) return fail(err, "short frame header");
            const int prec = seg[0], nf = seg[5];
            height = (seg[1] << 8) | seg[2];
            width = (seg[3] << 8) | seg[4];
            if (prec != 8) return fail(err, std::to_string(prec) + "-bit precision is unsupported (8-bit only)");
            if (nf == 1) return fail(err, "grayscale JPEG is unsupported (three components, YCbCr)");
            if (nf == 4) return fail(err, "CMYK / YCCK JPEG is unsupported (three components, YCbCr)");
            if (nf != 3) return fail(err, std::to_string(nf) + " components are unsupported (three components, YCbCr)");
            if (sl != 6 + 3 * (size_t)nf) return fail(err, "frame header length does not match its component count");
            if (width < 1 || height < 1)
                return fail(err, "image size " + std::to_string(width) + "x" + std::to_string(height) +
                                     " (a zero height, defined by a DNL marker, is unsupported)");
            for (int i = 0; i < 3; i++) {
                comp_id[i] = seg[6 + 3 * i];
                comp_h[i] = seg[7 + 3 * i] >> 4;
                comp_v[i] = seg[7 + 3 * i] & 15;
                comp_q[i] = seg[8 + 3 * i];
            }
            have_frame = true;
            break;
        }
        case 0xDB: {
            size_t p = 0;
            while (p < sl) {
                const int pq = seg[p] >> 4, tq = seg[p] & 15;
                p++;
                if (pq > 1 || tq > 3) return fail(err, "bad quantisation table header");
                const size_t size = 64 * (size_t)(pq + 1);
                if (size > sl - p) return fail(err, "truncated quantisation table");
                for (int i = 0; i < 64; i++)
                    qtabs[tq][ZIGZAG[i]] = pq ? (uint16_t)((seg[p + 2 * i] << 8) | seg[p + 2 * i + 1]) : seg[p + i];
                have_q[tq] = true;
                p += size;
            }
            break;
        }
        case 0xC4: {
            size_t p = 0;
            while (p < sl) {
                const int tc = seg[p] >> 4, th = seg[p] & 15;
                if (tc > 1 || th > 3) return fail(err, "bad Huffman table header");
                if (sl - p < 17) return fail(err, "truncated Huffman table");
                int total = 0;
                for (int i = 0; i < 16; i++) total += seg[p + 1 + i];
                if (total > 256 || (size_t)total > sl - p - 17) return fail(err, "truncated Huffman table");
                if (build_huffman(seg + p + 1, seg + p + 17, total, huff[tc * 4 + th], err)) return -1;
                p += 17 + (size_t)total;
            }
            break;
        }
        case 0xDD:
            if (sl != 2) return fail(err, "bad DRI segment");
            out.restart = (seg[0] << 8) | seg[1];
            break;
        case 0xE0:
            if (sl >= 5 && std::memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
            break;
        case 0xEE:
            if (sl >= 12 && std::memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
            break;
        case 0xDA: {
            if (!have_frame) return fail(err, "SOS before the frame header");
            if (sl < 1 || seg[0] != 3 || sl != 1 + 2 * 3 + 3)
                return fail(err, "non-interleaved (multi-scan) JPEG is unsupported: the three components must share one scan");
            if (!jfif) {
                if (adobe == 0) return fail(err, "Adobe transform 0 (RGB stored directly) is unsupported (YCbCr only)");
                if (adobe < 0 && comp_id[0] == 0x52 && comp_id[1] == 0x47 && comp_id[2] == 0x42)
                    return fail(err, "RGB component ids (no YCbCr transform) are unsupported (YCbCr only)");
            }
            for (int i = 0; i < 3; i++) {
                if (seg[1 + 2 * i] != comp_id[i]) return fail(err, "scan components are not in frame order");
                const int td = seg[2 + 2 * i] >> 4, ta = seg[2 + 2 * i] & 15;
                if (td > 3 || ta > 3 || !huff[td].defined || !huff[4 + ta].defined)
                    return fail(err, "scan refers to a Huffman table that was not defined");
                out.dc[i] = huff[td];
                out.ac[i] = huff[4 + ta];
            }
            const int hs = comp_h[0], vs = comp_v[0];
            if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1 ||
                !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) {
                std::string lay;
                for (int i = 0; i < 3; i++)
                    lay += (i ? ", " : "") + std::to_string(comp_h[i]) + "x" + std::to_string(comp_v[i]);
                return fail(err, "sampling layout " + lay + " is unsupported (4:4:4, 4:2:2 or 4:2:0 with 1x1 chroma)");
            }
            Info &in = out.info;
            in.width = width;
            in.height = height;
            in.hs = hs;
            in.vs = vs;
            out.mcus_w = (width + 8 * hs - 1) / (8 * hs);
            out.mcus_h = (height + 8 * vs - 1) / (8 * vs);
            in.blocks_w[0] = out.mcus_w * hs;
            in.blocks_h[0] = out.mcus_h * vs;
            in.blocks_w[1] = in.blocks_w[2] = out.mcus_w;
            in.blocks_h[1] = in.blocks_h[2] = out.mcus_h;
            for (int i = 0; i < 3; i++) {
                if (comp_q[i] > 3 || !have_q[comp_q[i]])
                    return fail(err, "frame refers to a quantisation table that was not defined");
                std::memcpy(in.qt[i], qtabs[comp_q[i]], sizeof(in.qt[i]));
            }
            out.scan_offset = pos;
            return 0;
        }
        default: break;  // APPn, COM and everything else with a length: skipped
        }
    }
}

// The bits of the entropy data: 0xFF00 unstuffed, stops in front of any marker (which it does not consume).
struct Bits {
    const uint8_t *data;
    size_t n, pos;
    uint64_t buf = 0;
    int cnt = 0;
    bool at_marker = false;  // the next unread bytes are a marker, or the input has ended

    Bits(const uint8_t *d, size_t n_, size_t p) : data(d), n(n_), pos(p) {}

    void fill() {
        while (cnt <= 56 && !at_marker) {
            if (pos >= n) {
                at_marker = true;
                break;
            }
            const uint8_t b = data[pos];
            if (b == 0xFF) {
                if (pos + 1 < n && data[pos + 1] == 0x00) {
                    pos += 2;
                } else {
                    at_marker = true;  // a marker, fill bytes before one, or a lone 0xFF at the end
                    break;
                }
            } else {
                pos++;
            }
            buf = (buf << 8) | b;
            cnt += 8;
        }
    }

    // the next 8 bits, zero-padded when fewer are left
    int peek8() {
        if (cnt < 8) fill();
        if (cnt >= 8) return (int)((buf >> (cnt - 8)) & 0xFF);
        return (int)((buf << (8 - cnt)) & 0xFF);
    }

    bool take(int nbits, int &v) {
        if (nbits == 0) {
            v = 0;
            return true;
        }
        if (cnt < nbits) fill();
        if (cnt < nbits) return false;
        v = (int)((buf >> (cnt - nbits)) & ((1u << nbits) - 1u));
        cnt -= nbits;
        return true;
    }

    // 0 ok, 1 out of data, 2 bad code
    int symbol(const Huffman &h, int &sym) {
        const int look = peek8();
        const int len = h.look_len[look];
        if (len) {
            if (cnt < len) return 1;
            cnt -= len;
            sym = h.look_sym[look];
            return 0;
        }
        int code;
        if (!take(8, code)) return 1;
        for (int l = 9; l <= 16; l++) {
            int bit;
            if (!take(1, bit)) return 1;
            code = (code << 1) | bit;
            if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) {
                const int idx = h.valptr[l] + code - h.mincode[l];
                if (idx < 0 || idx > 255) return 2;
                sym = h.symbols[idx];
                return 0;
            }
        }
        return 2;
    }

    // After the last block of a segment: drop the padding bits; whole bytes left over are an error.
    bool segment_done() {
        fill();
        if (cnt >= 8 || !at_marker) return false;
        buf = 0;
        cnt = 0;
        return true;
    }

    // The marker in front of which the reader stopped (fill bytes skipped): -1 when the input has ended.
    int marker() {
        while (pos < n && data[pos] == 0xFF) pos++;
        if (pos >= n || pos == 0 || data[pos - 1] != 0xFF) return -1;
        at_marker = false;
        return data[pos++];
    }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// out: capacity int16 values, at least 64 x the blocks of the three components. Zeroed and filled.
inline int decode(const uint8_t *data, size_t n, const Parsed &p, int16_t *out, size_t capacity, std::string &err) {
    const Info &in = p.info;
    size_t base[3], total = 0;
    for (int c = 0; c < 3; c++) {
        base[c] = total;
        total += (size_t)in.blocks_w[c] * (size_t)in.blocks_h[c];
    }
    if (!out || capacity < total * 64) return fail(err, "coefficient buffer too small");
    std::memset(out, 0, total * 64 * sizeof(int16_t));
    const char *early = "entropy data ends early (truncated file, or dimensions that do not match the data)";
    Bits br(data, n, p.scan_offset);
    const long long n_mcu = (long long)p.mcus_w * p.mcus_h;
    const long long per_seg = p.restart ? p.restart : n_mcu;
    const int samp_h[3] = {in.hs, 1, 1}, samp_v[3] = {in.vs, 1, 1};
    long long mcu = 0;
    int rst = 0;
    while (mcu < n_mcu) {
        int pred[3] = {0, 0, 0};
        const long long stop = mcu + per_seg < n_mcu ? mcu + per_seg : n_mcu;
        for (; mcu < stop; mcu++) {
            const int my = (int)(mcu / p.mcus_w), mx = (int)(mcu % p.mcus_w);
            for (int c = 0; c < 3; c++)
                for (int v = 0; v < samp_v[c]; v++)
                    for (int h = 0; h < samp_h[c]; h++) {
                        const size_t b = base[c] + (size_t)(my * samp_v[c] + v) * (size_t)in.blocks_w[c] +
                                         (size_t)(mx * samp_h[c] + h);
                        int16_t *blk = out + b * 64;
                        int s, bits, rc;
                        if ((rc = br.symbol(p.dc[c], s)))
                            return fail(err, rc == 1 ? early : "bad Huffman code in the entropy data");
                        if (s > 15) return fail(err, "bad DC size in the entropy data");
                        if (s) {
                            if (!br.take(s, bits)) return fail(err, early);
                            pred[c] = (int16_t)(pred[c] + extend(bits, s));
                        }
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            int rs;
                            if ((rc = br.symbol(p.ac[c], rs)))
                                return fail(err, rc == 1 ? early : "bad Huffman code in the entropy data");
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail(err, "coefficient index past 63 in the entropy data");
                            if (!br.take(s, bits)) return fail(err, early);
                            blk[ZIGZAG[k]] = (int16_t)extend(bits, s);
                            k++;
                        }
                    }
        }
        if (!br.segment_done())
            return fail(err, "entropy data left over after the last block (dimensions that do not match the data)");
        const int m = br.marker();
        if (mcu < n_mcu) {
            if (m < 0) return fail(err, early);
            if (m < 0xD0 || m > 0xD7)
                return fail(err, "restart markers do not match the restart interval (dimensions that do not match the data)");
            if (m - 0xD0 != (rst & 7)) return fail(err, "restart markers out of sequence");
            rst++;
        } else {
            if (m < 0) return fail(err, "missing EOI (truncated file)");
            if (m == 0xDA)
                return fail(err, "non-interleaved (multi-scan) JPEG is unsupported: a second scan follows the first");
            if (m >= 0xD0 && m <= 0xD7)
                return fail(err, "restart markers do not match the restart interval (dimensions that do not match the data)");
            if (m != 0xD9) {
                char hex[8];
                std::snprintf(hex, sizeof(hex), "%02X", m);
                return fail(err, std::string("marker 0x") + hex + " inside or after the entropy data instead of EOI");
            }
        }
    }
    return 0;
}

inline void copy_error(const std::string &err, char *buf, size_t len) {
    if (!buf || !len) return;
    const size_t k = err.size() < len - 1 ? err.size() : len - 1;
    std::memcpy(buf, err.data(), k);
    buf[k] = 0;
}

// The two C entries (jpeg.hip exports them from libdgs_hip.so; tools/jpeg_host_check.cpp calls them directly).
inline int header(const uint8_t *bytes, size_t len, Info *info, char *errbuf, size_t errlen) {
    std::string err;
    Parsed *p = new Parsed();
    int rc = info ? parse(bytes, len, *p, err) : fail(err, "null info");
    if (rc == 0) *info = p->info;
    delete p;
    if (rc) copy_error(err, errbuf, errlen);
    return rc;
}

inline int coefficients(const uint8_t *bytes, size_t len, const Info *info, int16_t *out, size_t capacity, char *errbuf,
                        size_t errlen) {
    std::string err;
    Parsed *p = new Parsed();
    int rc = info ? parse(bytes, len, *p, err) : fail(err, "null info");
    if (rc == 0 && std::memcmp(&p->info, info, sizeof(Info)) != 0)
        rc = fail(err, "the header passed in is not this file's (dgs_jpeg_header first)");
    if (rc == 0) rc = decode(bytes, len, *p, out, capacity, err);
    delete p;
    if (rc) copy_error(err, errbuf, errlen);
    return rc;
}

}  // namespace dgs_jpeg
