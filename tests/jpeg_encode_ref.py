"""A numpy restatement of the baseline JPEG encoder of csrc/jpeg_encode.hip + deformgs/jpeg_gpu.py: the oracle of the
encoder tests, as deformgs/jpeg.py is the oracle of the decoder. Slow (the entropy coder is a Python loop per
coefficient): for small images. It shares no code and no table with the encoder under test.

  quant_tables(quality)             jcparam.c: jpeg_quality_scaling + the two Annex K tables, force_baseline
  coefficients(rgb, qt, hs, vs)     libjpeg-turbo's default compressor in integers: jccolor.c RGB -> YCbCr, jcsample.c
                                    h2v1 / h2v2 box downsampling, jfdctint.c forward DCT, quantisation against
                                    qtable << 3 rounding half away from zero, jccoefct.c's dummy blocks; the layout
                                    of deformgs.jpeg.decode_coefficients
  encode(rgb, quality, subsampling) the complete JFIF file: one interleaved scan, the Annex K Huffman tables, a
                                    restart interval of one MCU row
"""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63]

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# ITU-T T.81 Annex K.1, natural order
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# ITU-T T.81 Annex K.3: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def quant_tables(quality):
    """-> uint16 (2, 64), natural order: luma, chroma."""
    if not 1 <= quality <= 100:
        raise ValueError("quality 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    out = np.zeros((2, 64), np.uint16)
    for i, base in enumerate((STD_LUMA, STD_CHROMA)):
        out[i] = [min(max((b * scale + 50) // 100, 1), 255) for b in base]
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    """jccolor.c rgb_ycc_convert: uint8 (H, W, 3) -> three int64 (H, W) planes."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    off = (128 << 16) + half - 1
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + off) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + off) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    """Replicates the last column, then the last row, up to (rows, cols)."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def component_planes(rgb, hs, vs):
    """-> [Y, Cb, Cr] int64 planes at each component's own block-padded size (no dummy blocks)."""
    H, W = rgb.shape[:2]
    y, cb, cr = rgb_to_ycc(rgb)
    planes = [_pad(y, -(-H // 8) * 8, -(-W // 8) * 8)]
    cw, ch = -(-W // hs), -(-H // vs)
    ocols, orows = -(-cw // 8) * 8, -(-ch // 8) * 8
    for p in (cb, cr):
        if hs == 2:
            # the input rows are padded to the row group (vs rows) and 2 * ocols columns, then box-filtered
            q = _pad(p, ch * vs, 2 * ocols)
            if vs == 2:
                s = q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]
                bias = np.tile([1, 2], ocols // 2)
                q = (s + bias) >> 2
            else:
                s = q[:, 0::2] + q[:, 1::2]
                bias = np.tile([0, 1], ocols // 2)
                q = (s + bias) >> 1
            p = q
        planes.append(_pad(p, orows, ocols))
    return planes


_C = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
          f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """jfdctint.c, one pass of the 8-point forward DCT along the last axis of int64 (..., 8)."""
    C = _C
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 13 - 2 if first else 13 + 2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * C["f0_541"]
    out[2] = _descale(z1 + t13 * C["f0_765"], sh)
    out[6] = _descale(z1 - t12 * C["f1_847"], sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["f1_175"]
    t4, t5, t6, t7 = t4 * C["f0_298"], t5 * C["f2_053"], t6 * C["f3_072"], t7 * C["f1_501"]
    z1, z2 = -z1 * C["f0_899"], -z2 * C["f2_562"]
    z3, z4 = -z3 * C["f1_961"] + z5, -z4 * C["f0_390"] + z5
    out[7] = _descale(t4 + z1 + z3, sh)
    out[5] = _descale(t5 + z2 + z4, sh)
    out[3] = _descale(t6 + z2 + z3, sh)
    out[1] = _descale(t7 + z1 + z4, sh)
    return np.stack(out, axis=-1)


def fdct_quantise(plane, qt):
    """int64 (8 bh, 8 bw) samples, uint16 (64,) -> int64 (bh, bw, 64) quantised coefficients, natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    x = _fdct_pass(x, True)  # rows
    x = _fdct_pass(x.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # columns
    q = qt.astype(np.int64).reshape(8, 8) << 3
    mag = (np.abs(x) + (q >> 1)) // q
    return (np.sign(x) * mag).reshape(bh, bw, 64)


def coefficients(rgb, qt, hs, vs):
    """-> int16 (total_blocks, 64) in the layout of deformgs.jpeg.decode_coefficients: component-major,
    block-row-major, the grids padded to whole MCUs with jccoefct.c's dummy blocks (AC zero, DC of the block before
    in the MCU's own order)."""
    H, W = rgb.shape[:2]
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    out = []
    for c, plane in enumerate(component_planes(rgb, hs, vs)):
        ch_, cv = (hs, vs) if c == 0 else (1, 1)
        real = fdct_quantise(plane, qt[min(c, 1)])
        hib, wib = real.shape[:2]
        full = np.zeros((mh * cv, mw * ch_, 64), np.int64)
        full[:hib, :wib] = real
        for my in range(mh):
            for mx in range(mw):
                last = None  # DC of the previous block of this MCU
                for v in range(cv):
                    for h in range(ch_):
                        by, bx = my * cv + v, mx * ch_ + h
                        if by >= hib or bx >= wib:
                            full[by, bx, 0] = last
                        last = full[by, bx, 0]
        out.append(full.reshape(-1, 64))
    return np.concatenate(out).astype(np.int16)


def _codes(table):
    """-> {symbol: (code, length)} of a canonical Huffman table."""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _encode_block(bw, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    a = abs(diff)
    s = a.bit_length()
    bw.put(*dc[s])
    if s:
        bw.put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        s = abs(v).bit_length()
        bw.put(*ac[(run << 4) | s])
        bw.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        run = 0
    if run:
        bw.put(*ac[0x00])


def entropy_scan(coef, W, H, hs, vs):
    """The entropy-coded data of the one interleaved scan with a restart interval of one MCU row (RSTm between the
    rows, none after the last)."""
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    grids = [(mw * hs, mh * vs), (mw, mh), (mw, mh)]
    base = [0, grids[0][0] * grids[0][1]]
    base.append(base[1] + mw * mh)
    dc = [_codes(DC_LUMA), _codes(DC_CHROMA)]
    ac = [_codes(AC_LUMA), _codes(AC_CHROMA)]
    out = bytearray()
    for my in range(mh):
        bw = _BitWriter()
        pred = [0, 0, 0]
        for mx in range(mw):
            for c in range(3):
                ch_, cv = (hs, vs) if c == 0 else (1, 1)
                for v in range(cv):
                    for h in range(ch_):
                        blk = coef[base[c] + (my * cv + v) * grids[c][0] + mx * ch_ + h]
                        _encode_block(bw, blk, pred[c], dc[min(c, 1)], ac[min(c, 1)])
                        pred[c] = int(blk[0])
        bw.flush()
        out += bw.out
        if my < mh - 1:
            out += bytes((0xFF, 0xD0 + (my & 7)))
    return bytes(out)


def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def header(W, H, hs, vs, qt):
    """SOI, APP0 (JFIF 1.01, density 1:1), two DQT, SOF0, four DHT, DRI (one MCU row), SOS."""
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for i in range(2):
        parts.append(_segment(0xDB, bytes([i]) + bytes(int(qt[i][z]) for z in ZIGZAG)))
    parts.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes((1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1))))
    for tc, table in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        parts.append(_segment(0xC4, bytes([tc]) + bytes(table[0]) + bytes(table[1])))
    parts.append(_segment(0xDD, struct.pack(">H", -(-W // (8 * hs)))))
    parts.append(_segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(parts)


def encode(rgb, quality=90, subsampling="4:2:0"):
    """uint8 (H, W, 3) -> the JFIF file as bytes."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    hs, vs = SAMPLING[subsampling]
    H, W = rgb.shape[:2]
    qt = quant_tables(quality)
    coef = coefficients(rgb, qt, hs, vs)
    return header(W, H, hs, vs, qt) + entropy_scan(coef, W, H, hs, vs) + b"\xff\xd9"
