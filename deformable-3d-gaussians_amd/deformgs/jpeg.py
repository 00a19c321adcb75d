"""A baseline JPEG decoder on the standard library and numpy alone: the CPU path of deformgs/ingest.py for JPEG
files (device="cpu") and the oracle of the GPU tests, as png.py / ingest_group_numpy are for PNG. Slow (the
entropy decoder is a Python loop per coefficient): for small images. It does not need libdgs_hip.so.

Two halves, split where the device path splits them (csrc/jpeg_decode.h on the host, csrc/jpeg.hip on the GPU):

  parse_header / decode_coefficients   markers, Huffman decoding -> quantised coefficients, component-major,
                                       block-row-major, 64 int16 per block in natural (de-zigzagged) order,
                                       the block grid padded to whole MCUs
  idct_planes / upsample_color         libjpeg-turbo's default decompressor in integers: dequantise + the
                                       "islow" 8x8 inverse DCT (jidctint.c), fancy chroma upsampling
                                       (jdsample.c), YCbCr -> RGB in 16-bit fixed point (jdcolor.c)

The output is PIL's (libjpeg-turbo 3.x) byte for byte: tests/golden/jpeg_ingest.npz.

Read: SOF0 / SOF1 (baseline / extended sequential Huffman), 8 bits, three components (YCbCr) in one interleaved
scan, chroma 1x1 with luma 1x1, 2x1 or 2x2, restart intervals, any number of DQT / DHT segments, APPn / COM
skipped (EXIF orientation is ignored, as Image.open ignores it). Everything else raises ValueError naming the
reason; so does truncated or corrupt entropy data.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                   45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

_SOF_REFUSED = {0xC2: "progressive JPEG (SOF2)", 0xC3: "lossless JPEG (SOF3)",
                0xC5: "differential sequential JPEG (SOF5)", 0xC6: "differential progressive JPEG (SOF6)",
                0xC7: "differential lossless JPEG (SOF7)", 0xC9: "arithmetic coding (SOF9)",
                0xCA: "arithmetic coding (SOF10)", 0xCB: "arithmetic coding (SOF11)",
                0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)",
                0xCF: "arithmetic coding (SOF15)"}


class JpegHeader:
    """width, height; hs, vs: the luma sampling factors; blocks: [(blocks_w, blocks_h)] per component, padded to
    whole MCUs; qt: (3, 64) uint16 quantisation tables per component in natural order; plus what the entropy
    decoder needs (Huffman tables per component, restart interval, the offset of the entropy data)."""

    @property
    def total_blocks(self):
        return sum(w * h for w, h in self.blocks)


def _fail(msg):
    raise ValueError(f"JPEG: {msg}")


def _huffman(counts, symbols):
    """-> {(length, code): symbol} of a canonical table."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= (1 << length):
                _fail("bad Huffman table (code lengths overflow)")
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


def parse_header(data):
    """Everything up to and including the SOS header. -> JpegHeader."""
    data = bytes(data)
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        _fail("not a JPEG file (no SOI)")
    pos = 2
    qtabs, huff = {}, {}
    frame = None
    restart = 0
    jfif, adobe = False, None
    while True:
        if pos >= n:
            _fail("truncated before the scan (no SOS)")
        if data[pos] != 0xFF:
            _fail(f"expected a marker at byte {pos}")
        while pos < n and data[pos] == 0xFF:  # fill bytes
            pos += 1
        if pos >= n:
            _fail("truncated inside a marker")
        m = data[pos]
        pos += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue  # stand-alone markers
        if m == 0xD9:
            _fail("EOI before any scan")
        if m == 0x00:
            _fail(f"stuffed byte outside entropy data at byte {pos - 2}")
        if pos + 2 > n:
            _fail("truncated segment length")
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2 or pos + length > n:
            _fail("truncated segment")
        seg = data[pos + 2:pos + length]
        pos += length
        if m in _SOF_REFUSED:
            _fail(f"{_SOF_REFUSED[m]} is unsupported (baseline / extended sequential Huffman only)")
        if m in (0xC0, 0xC1):
            if frame is not None:
                _fail("two frame headers")
            if len(seg) < 6:
                _fail("short frame header")
            prec, h, w, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                _fail(f"{prec}-bit precision is unsupported (8-bit only)")
            if nf == 1:
                _fail("grayscale JPEG is unsupported (three components, YCbCr)")
            if nf == 4:
                _fail("CMYK / YCCK JPEG is unsupported (three components, YCbCr)")
            if nf != 3:
                _fail(f"{nf} components are unsupported (three components, YCbCr)")
            if len(seg) != 6 + 3 * nf:
                _fail("frame header length does not match its component count")
            if w < 1 or h < 1:
                _fail(f"image size {w}x{h} (a zero height, defined by a DNL marker, is unsupported)")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(3)]
            frame = (w, h, comps)
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                p += 1
                if pq > 1 or tq > 3:
                    _fail("bad quantisation table header")
                size = 64 * (pq + 1)
                if p + size > len(seg):
                    _fail("truncated quantisation table")
                raw = np.frombuffer(seg, np.uint8, size, p).astype(np.uint16)
                if pq:
                    raw = (raw[0::2] << 8) | raw[1::2]
                tab = np.zeros(64, np.uint16)
                tab[ZIGZAG] = raw
                qtabs[tq] = tab
                p += size
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 3:
                    _fail("bad Huffman table header")
                if p + 17 > len(seg):
                    _fail("truncated Huffman table")
                counts = list(seg[p + 1:p + 17])
                total = sum(counts)
                if total > 256 or p + 17 + total > len(seg):
                    _fail("truncated Huffman table")
                huff[(tc, th)] = _huffman(counts, list(seg[p + 17:p + 17 + total]))
                p += 17 + total
        elif m == 0xCC:
            _fail("arithmetic coding (DAC) is unsupported")
        elif m == 0xDD:
            if len(seg) != 2:
                _fail("bad DRI segment")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            if seg[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                _fail("SOS before the frame header")
            w, h, comps = frame
            if len(seg) < 1 or seg[0] != 3 or len(seg) != 1 + 2 * 3 + 3:
                _fail("non-interleaved (multi-scan) JPEG is unsupported: the three components must share one scan")
            if not jfif:
                if adobe == 0:
                    _fail("Adobe transform 0 (RGB stored directly) is unsupported (YCbCr only)")
                if adobe is None and [c[0] for c in comps] == [0x52, 0x47, 0x42]:
                    _fail("RGB component ids (no YCbCr transform) are unsupported (YCbCr only)")
            tables = []
            for i in range(3):
                cs, t = seg[1 + 2 * i], seg[2 + 2 * i]
                if cs != comps[i][0]:
                    _fail("scan components are not in frame order")
                td, ta = t >> 4, t & 15
                if (0, td) not in huff or (1, ta) not in huff:
                    _fail("scan refers to a Huffman table that was not defined")
                tables.append((huff[(0, td)], huff[(1, ta)]))
            (_, hs, vs, _), c1, c2 = comps
            if (c1[1], c1[2], c2[1], c2[2]) != (1, 1, 1, 1) or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
                lay = ", ".join(f"{c[1]}x{c[2]}" for c in comps)
                _fail(f"sampling layout {lay} is unsupported (4:4:4, 4:2:2 or 4:2:0 with 1x1 chroma)")
            hd = JpegHeader()
            hd.width, hd.height, hd.hs, hd.vs = w, h, hs, vs
            hd.mcus_w, hd.mcus_h = -(-w // (8 * hs)), -(-h // (8 * vs))
            hd.blocks = [(hd.mcus_w * hs, hd.mcus_h * vs), (hd.mcus_w, hd.mcus_h), (hd.mcus_w, hd.mcus_h)]
            qt = np.zeros((3, 64), np.uint16)
            for i in range(3):
                if comps[i][3] not in qtabs:
                    _fail("frame refers to a quantisation table that was not defined")
                qt[i] = qtabs[comps[i][3]]
            hd.qt = qt
            hd.huffman = tables
            hd.restart = restart
            hd.scan_offset = pos
            return hd
        # APPn, COM and everything else with a length: skipped


class _Bits:
    """The bits of one entropy-coded segment (between markers), 0xFF00 unstuffed."""

    def __init__(self, payload):
        self.data = payload
        self.pos = 0
        self.buf = 0
        self.cnt = 0

    def bit(self):
        if self.cnt == 0:
            if self.pos >= len(self.data):
                _fail("entropy data ends early (truncated file, or dimensions that do not match the data)")
            self.buf = self.data[self.pos]
            self.pos += 1
            self.cnt = 8
        self.cnt -= 1
        return (self.buf >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        _fail("bad Huffman code in the entropy data")

    def left_over(self):
        return len(self.data) - self.pos


def _segments(data, pos):
    """Entropy data from `pos`: -> [unstuffed bytes per restart segment], [the RSTn numbers between them], the
    marker that ends the scan (None when the data runs out)."""
    segs, rsts, cur = [], [], bytearray()
    n = len(data)
    while pos < n:
        nxt = data.find(b"\xff", pos)
        if nxt < 0:
            cur += data[pos:]
            pos = n
            break
        cur += data[pos:nxt]
        pos = nxt + 1
        while pos < n and data[pos] == 0xFF:  # fill bytes before a marker
            pos += 1
        if pos >= n:
            break
        m = data[pos]
        pos += 1
        if m == 0:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            segs.append(bytes(cur))
            rsts.append(m - 0xD0)
            cur = bytearray()
        else:
            segs.append(bytes(cur))
            return segs, rsts, m
    segs.append(bytes(cur))
    return segs, rsts, None


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _wrap16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def decode_coefficients(data, header=None):
    """-> int16 (total_blocks, 64): quantised coefficients, component-major, block-row-major, natural order."""
    data = bytes(data)
    hd = header or parse_header(data)
    segs, rsts, end = _segments(data, hd.scan_offset)
    if end is None:
        _fail("missing EOI (truncated file)")
    if end == 0xDA:
        _fail("non-interleaved (multi-scan) JPEG is unsupported: a second scan follows the first")
    if end != 0xD9:
        _fail(f"marker 0x{end:02X} inside or after the entropy data instead of EOI")
    n_mcu = hd.mcus_w * hd.mcus_h
    per_seg = hd.restart or n_mcu
    if len(segs) != -(-n_mcu // per_seg):
        _fail("restart markers do not match the restart interval (dimensions that do not match the data)")
    if any(r != (i & 7) for i, r in enumerate(rsts)):
        _fail("restart markers out of sequence")
    out = np.zeros((hd.total_blocks, 64), np.int16)
    base = [0, hd.blocks[0][0] * hd.blocks[0][1]]
    base.append(base[1] + hd.blocks[1][0] * hd.blocks[1][1])
    samp = [(hd.hs, hd.vs), (1, 1), (1, 1)]
    zz = ZIGZAG.tolist()
    mcu = 0
    for seg in segs:
        br = _Bits(seg)
        pred = [0, 0, 0]
        for _ in range(min(per_seg, n_mcu - mcu)):
            my, mx = divmod(mcu, hd.mcus_w)
            for c in range(3):
                dc_tab, ac_tab = hd.huffman[c]
                ch, cv = samp[c]
                for v in range(cv):
                    for h in range(ch):
                        blk = out[base[c] + (my * cv + v) * hd.blocks[c][0] + mx * ch + h]
                        s = br.symbol(dc_tab)
                        if s > 15:
                            _fail("bad DC size in the entropy data")
                        if s:
                            pred[c] = _wrap16(pred[c] + _extend(br.bits(s), s))
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = br.symbol(ac_tab)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                _fail("coefficient index past 63 in the entropy data")
                            blk[zz[k]] = _wrap16(_extend(br.bits(s), s))
                            k += 1
            mcu += 1
        if br.left_over():
            _fail("entropy data left over after the last block (dimensions that do not match the data)")
    return out


_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
          f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


def _idct_pass(x, shift):
    """jidctint.c, one pass of the 8-point inverse DCT along axis 1 of int64 (n, 8, 8); descale by `shift`."""
    F = _F
    z2, z3 = x[:, 2], x[:, 6]
    z1 = (z2 + z3) * F["f0_541"]
    tmp2 = z1 - z3 * F["f1_847"]
    tmp3 = z1 + z2 * F["f0_765"]
    tmp0 = (x[:, 0] + x[:, 4]) << 13
    tmp1 = (x[:, 0] - x[:, 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[:, 7], x[:, 5], x[:, 3], x[:, 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F["f1_175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F["f0_298"], tmp1 * F["f2_053"], tmp2 * F["f3_072"], tmp3 * F["f1_501"]
    z1, z2 = -z1 * F["f0_899"], -z2 * F["f2_562"]
    z3, z4 = -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rows = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
            tmp10 - tmp3]
    return (np.stack(rows, axis=1) + (1 << (shift - 1))) >> shift


def idct_blocks(coef, qt):
    """int16 (n, 64) natural order, uint16 (64,) -> uint8 (n, 8, 8): dequantise + jpeg_idct_islow."""
    x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(-1, 8, 8)
    ws = _idct_pass(x, 13 - 2)  # columns: along the row index
    y = _idct_pass(ws.transpose(0, 2, 1), 13 + 2 + 3).transpose(0, 2, 1)  # rows
    s = ((y & 1023) ^ 512) - 512  # the wrap-around range-limit table: a signed 10-bit value
    return np.clip(s + 128, 0, 255).astype(np.uint8)


def idct_planes(coef, header):
    """-> [Y, Cb, Cr] uint8 planes at block-padded size."""
    planes, k = [], 0
    for c, (bw, bh) in enumerate(header.blocks):
        px = idct_blocks(coef[k:k + bw * bh], header.qt[c])
        planes.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
        k += bw * bh
    return planes


def _fancy_h2v1(p):
    """jdsample.c h2v1_fancy_upsample on int64 (rows, cw), cw > 2 -> (rows, 2 cw)."""
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0] = p[:, 0]
    out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + 2) >> 2
    out[:, -1] = p[:, -1]
    return out


def _fancy_h2v2(p):
    """jdsample.c h2v2_fancy_upsample on int64 (ch, cw), cw > 2 -> (2 ch, 2 cw); the row above the first and
    below the last is that row itself."""
    up = np.concatenate([p[:1], p[:-1]])
    down = np.concatenate([p[1:], p[-1:]])
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for v, far in ((0, up), (1, down)):
        s = 3 * p + far
        o = out[v::2]
        o[:, 0] = (4 * s[:, 0] + 8) >> 4
        o[:, 2::2] = (3 * s[:, 1:] + s[:, :-1] + 8) >> 4
        o[:, 1:-1:2] = (3 * s[:, :-1] + s[:, 1:] + 7) >> 4
        o[:, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def upsample_chroma(plane, W, H, hs, vs):
    """A block-padded chroma plane -> int64 (H, W) at full size."""
    cw, ch = -(-W // hs), -(-H // vs)
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 1:
        return p
    if cw > 2:
        p = _fancy_h2v1(p) if vs == 1 else _fancy_h2v2(p)
    else:
        p = np.repeat(p, 2, axis=1)
        if vs == 2:
            p = np.repeat(p, 2, axis=0)
    return p[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert on int64 arrays -> uint8 (..., 3)."""
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def upsample_color(planes, header):
    """[Y, Cb, Cr] block-padded planes -> uint8 (H, W, 3)."""
    W, H, hs, vs = header.width, header.height, header.hs, header.vs
    y = planes[0][:H, :W].astype(np.int64)
    return ycc_to_rgb(y, upsample_chroma(planes[1], W, H, hs, vs), upsample_chroma(planes[2], W, H, hs, vs))


def decode_jpeg(data):
    """-> uint8 (H, W, 3) RGB: what np.asarray(PIL.Image.open(...)) gives with libjpeg-turbo."""
    hd = parse_header(data)
    return upsample_color(idct_planes(decode_coefficients(data, hd), hd), hd)


def jpeg_size(path):
    """(width, height) from the frame header of a JPEG file: markers only, and only as much of the file as
    holds them (the first 4 KiB, doubled while the markers before the scan run on: a large EXIF segment)."""
    with open(path, "rb") as f:
        data = f.read(4096)
        while True:
            try:
                hd = parse_header(data)
                break
            except ValueError as e:
                more = f.read(len(data))
                if not more:
                    raise ValueError(f"{path}: {e}") from None
                data += more
    return hd.width, hd.height


def read_jpeg(path):
    with open(path, "rb") as f:
        return decode_jpeg(f.read())
