"""Plain numpy / Python statement of the baseline JPEG rule of ``stac_mjx_amd/csrc/stac_jpeg.hip`` (test infrastructure).

It is what libjpeg does for 8-bit RGB input with its default settings at 4:2:0: integer colour conversion, edge replication,
2 x 2 box downsampling with alternating bias, the "slow integer" forward DCT, IJG quality scaling, Annex K Huffman tables, one
interleaved scan, an optional restart interval.  ``encode(rgb, quality, restart_mcus)`` returns the whole file;
``tests/test_jpeg_host.py`` checks it byte for byte against Pillow.  It shares no code with the product.
"""

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K, natural (row-major) order
QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
              80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
              95, 98, 112, 100, 103, 99]
QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                99, 99] + [99] * 32

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def quant_table(base, quality):
    """IJG scaling; natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255)


def _codes(spec):
    bits, vals = spec
    tab, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            tab[vals[k]] = (code, length)
            k += 1
            code += 1
        code <<= 1
    return tab


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(width, height, quality, restart_mcus=0):
    """SOI .. SOS."""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t, base in enumerate((QUANT_LUMA, QUANT_CHROMA)):
        q = quant_table(base, quality)
        out += _segment(0xDB, [t] + [int(q[z]) for z in ZIGZAG])
    out += _segment(0xC0, [8] + list(height.to_bytes(2, "big")) + list(width.to_bytes(2, "big")) + [3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, [cls] + bits + vals)
    if restart_mcus:
        out += _segment(0xDD, list(restart_mcus.to_bytes(2, "big")))
    return out + _segment(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0])


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """1-D pass over the last axis."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o2, o6 = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5, o3, o1 = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct(block):
    """[..., 8, 8] samples minus 128 -> 8 x the DCT."""
    rows = _dct_pass(block.astype(np.int64), True)
    return np.swapaxes(_dct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def _quantise(coef, q):
    d = 8 * q
    t = np.abs(coef) + (d >> 1)
    t = np.where(t >= d, t // d, 0)
    return np.where(coef < 0, -t, t)


def _edge(x, h, w):
    return np.pad(x, ((0, h - x.shape[0]), (0, w - x.shape[1])), mode="edge")


def planes(rgb):
    """Padded Y [16 mh, 16 mw] and Cb, Cr [8 mh, 8 mw]."""
    H, W, _ = rgb.shape
    R, G, B = [rgb[..., k].astype(np.int64) for k in range(3)]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    mw, mh = (W + 15) // 16, (H + 15) // 16

    def down(x):
        x = _edge(x, H + (H & 1), 16 * mw)  # columns out to the MCU grid, rows only to an even height
        s = x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2]
        bias = np.tile([1, 2], s.shape[1] // 2)[None, :]
        return _edge((s + bias) >> 2, 8 * mh, 8 * mw)  # then the last downsampled row is repeated

    return _edge(Y, 16 * mh, 16 * mw), down(Cb), down(Cr)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _lane_words(z, pred, dc, ac):
    """The words of one coded block, one per coefficient that codes something (what one lane of the kernel forms):
    ("dc", category, 0, bits, n), ("ac", symbol, ZRL codes in front, bits, n), ("eob", 0, 0, bits, n)."""
    d = int(z[0]) - pred
    s = abs(d).bit_length()
    code, length = dc[s]
    yield "dc", s, 0, (code << s) | ((d if d >= 0 else d - 1) & ((1 << s) - 1)), length + s
    run = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            run += 1
            continue
        bits, n, chain = 0, 0, 0
        while run > 15:
            code, length = ac[0xF0]
            bits, n, chain = (bits << length) | code, n + length, chain + 1
            run -= 16
        s = abs(v).bit_length()
        code, length = ac[(run << 4) | s]
        bits = (((bits << length) | code) << s) | ((v if v >= 0 else v - 1) & ((1 << s) - 1))
        yield "ac", (run << 4) | s, chain, bits, n + length + s
        run = 0
    if run:
        yield ("eob", 0, 0) + ac[0x00]


def _walk(rgb, quality, restart_mcus):
    """The scan in stream order: ("rst", k) where a restart marker goes, ("mcu",) in front of every MCU and
    ("block", table, z, pred) for every coded block (z: 64 quantised coefficients in zigzag order, pred: its DC prediction)."""
    H, W, _ = rgb.shape
    Y, Cb, Cr = planes(np.asarray(rgb))
    mw, mh = (W + 15) // 16, (H + 15) // 16
    q = [quant_table(QUANT_LUMA, quality), quant_table(QUANT_CHROMA, quality)]
    zz = np.asarray(ZIGZAG)

    def coefficients(p, qt):
        by, bx = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(by, 8, bx, 8).swapaxes(1, 2) - 128
        return _quantise(fdct(blocks), qt.reshape(8, 8)).reshape(by, bx, 64)[..., zz]

    cy, ccb, ccr = coefficients(Y, q[0]), coefficients(Cb, q[1]), coefficients(Cr, q[1])
    real_y = ((W + 7) // 8, (H + 7) // 8)  # real blocks per row / column of the component; beyond them: dummy blocks
    real_c = (((W + 1) // 2 + 7) // 8, ((H + 1) // 2 + 7) // 8)
    pred, n, rst = [0, 0, 0], 0, 0
    for my in range(mh):
        for mx in range(mw):
            if restart_mcus and n and n % restart_mcus == 0:
                yield "rst", rst
                rst = (rst + 1) & 7
                pred = [0, 0, 0]
            n += 1
            yield ("mcu",)
            blocks = [(0, cy, 2 * mx + bx, 2 * my + by, real_y) for by in range(2) for bx in range(2)]
            blocks += [(1, ccb, mx, my, real_c), (2, ccr, mx, my, real_c)]
            for comp, coef, X, Yb, real in blocks:
                if X < real[0] and Yb < real[1]:
                    z = coef[Yb, X]
                else:  # not transformed: AC 0, DC = the DC coded just before
                    z = np.zeros(64, np.int64)
                    z[0] = pred[comp]
                yield "block", min(comp, 1), z, pred[comp]
                pred[comp] = int(z[0])


def scan(rgb, quality, restart_mcus=0):
    """The entropy-coded data between SOS and EOI."""
    dc = [_codes(DC_LUMA), _codes(DC_CHROMA)]
    ac = [_codes(AC_LUMA), _codes(AC_CHROMA)]
    w = _Bits()
    for item in _walk(np.asarray(rgb), quality, restart_mcus):
        if item[0] == "rst":
            w.flush()
            w.out.extend([0xFF, 0xD0 + item[1]])
        elif item[0] == "block":
            _, t, z, pred = item
            for _, _, _, bits, n in _lane_words(z, pred, dc[t], ac[t]):
                w.put(bits, n)
    w.flush()
    return bytes(w.out)


def encode(rgb, quality, restart_mcus=0):
    rgb = np.asarray(rgb)
    H, W, _ = rgb.shape
    return header(W, H, quality, restart_mcus) + scan(rgb, quality, restart_mcus) + b"\xff\xd9"


def pillow(rgb, quality, restart_mcus=0):
    """Pillow's bytes for the same settings (the yardstick)."""
    import io

    from PIL import Image

    buf = io.BytesIO()
    kw = {"restart_marker_blocks": restart_mcus} if restart_mcus else {}
    Image.fromarray(np.ascontiguousarray(rgb, dtype=np.uint8), "RGB").save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


def images():
    """name -> [H, W, 3] uint8: the cases of the parity tests."""
    rng = np.random.default_rng(1)
    out = {"noise97x61": rng.integers(0, 256, (61, 97, 3), dtype=np.uint8),
           "noise100x36": rng.integers(0, 256, (36, 100, 3), dtype=np.uint8)}
    g = np.zeros((40, 50, 3), np.uint8)
    g[..., 0] = np.arange(50)[None] * 5
    g[..., 1] = np.arange(40)[:, None] * 6
    g[..., 2] = 77
    out["grad50x40"] = g
    yy, xx = np.mgrid[0:90, 0:130]
    out["smooth130x90"] = np.stack([(xx * 2) % 256, (yy * 3) % 256, (xx + yy) % 256], -1).astype(np.uint8)
    out["const16x16"] = np.full((16, 16, 3), 200, np.uint8)
    out["tiny5x3"] = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    out["one1x1"] = np.array([[[9, 200, 31]]], np.uint8)
    out["sat33x17"] = (rng.integers(0, 2, (17, 33, 3)) * 255).astype(np.uint8)
    s = np.zeros((64, 160, 3), np.uint8)
    s[10:30, 20:90] = (255, 0, 0)
    s[40:60, 100:150] = (0, 255, 255)
    out["shapes160x64"] = s
    return out


# ---- what a stream exercises ---------------------------------------------------------------------------------------------
LONG_WORD = 34  # a word of 34 bits or more reaches a third 32-bit word at some bit position


def stats(rgb, quality, restart_mcus=0):
    """What the scan of `encode(rgb, quality, restart_mcus)` exercises.  {"luma": t, "chroma": t, "mcu_bits": the most bits in
    one MCU, "intervals": [the unstuffed bytes of every restart interval, padded]}, t = {"dc": set of DC categories, "ac": set of
    AC symbols, "zrl": set of ZRL chain lengths in front of a symbol (0 included), "eob" / "no_eob": a block ended with / without
    EOB, "longest": the longest word in bits, "long_at": set of (bit position mod 32 inside the interval's unstuffed stream) of
    the words of LONG_WORD bits or more}."""
    dc = [_codes(DC_LUMA), _codes(DC_CHROMA)]
    ac = [_codes(AC_LUMA), _codes(AC_CHROMA)]
    tabs = [dict(dc=set(), ac=set(), zrl=set(), eob=False, no_eob=False, longest=0, long_at=set()) for _ in range(2)]
    intervals, acc, pos, mcu_start, mcu_bits = [], 0, 0, 0, 0

    def close():
        pad = -pos % 8
        intervals.append((((acc << pad) | ((1 << pad) - 1)).to_bytes((pos + pad) // 8, "big")))

    for item in _walk(np.asarray(rgb), quality, restart_mcus):
        if item[0] == "rst":
            mcu_bits = max(mcu_bits, pos - mcu_start)
            close()
            acc, pos, mcu_start = 0, 0, 0
        elif item[0] == "mcu":
            mcu_bits = max(mcu_bits, pos - mcu_start)
            mcu_start = pos
        else:
            _, t, z, pred = item
            T, ended = tabs[t], False
            for kind, sym, chain, bits, n in _lane_words(z, pred, dc[t], ac[t]):
                if kind == "dc":
                    T["dc"].add(sym)
                elif kind == "ac":
                    T["ac"].add(sym)
                    T["zrl"].add(chain)
                else:
                    ended = True
                T["longest"] = max(T["longest"], n)
                if n >= LONG_WORD:
                    T["long_at"].add(pos % 32)
                acc, pos = (acc << n) | bits, pos + n
            T["eob" if ended else "no_eob"] = True
    mcu_bits = max(mcu_bits, pos - mcu_start)
    close()
    return {"luma": tabs[0], "chroma": tabs[1], "mcu_bits": mcu_bits, "intervals": intervals}


def restuffed(st):
    """The scan bytes from stats()'s intervals: stuffing and restart markers put back (ties stats() to scan())."""
    return b"".join((b"" if k == 0 else bytes([0xFF, 0xD0 + (k - 1) % 8])) + iv.replace(b"\xff", b"\xff\x00")
                    for k, iv in enumerate(st["intervals"]))


# ---- edge images ------------------------------------------------------------------------------------------------------------
_C = np.array([[(0.5 if k else np.sqrt(0.125)) * np.cos((2 * x + 1) * k * np.pi / 16) for x in range(8)] for k in range(8)])
BLUE, YELLOW, RED, CYAN = (0, 0, 255), (255, 255, 0), (255, 0, 0), (0, 255, 255)


def idct(coef):
    """[..., 8, 8] orthonormal DCT coefficients (natural order) -> samples, in floating point."""
    return _C.T @ np.asarray(coef, np.float64) @ _C


def _grey(y):
    return np.repeat(np.clip(np.rint(y), 0, 255).astype(np.uint8)[..., None], 3, -1)


def _tile(blocks):
    """[by, bx, 8, 8] -> [8 by, 8 bx]."""
    by, bx = blocks.shape[:2]
    return blocks.swapaxes(1, 2).reshape(8 * by, 8 * bx)


def _along(pattern, c0, c1):
    """Colours between c0 and c1 (pattern -127.5 .. 127.5, 0 = half way) at 2 x 2 pixels per sample: one chroma component
    swings over its whole range while the picture stays inside the RGB cube."""
    t = np.clip(0.5 + np.asarray(pattern) / 255.0, 0, 1)
    t = np.repeat(np.repeat(t, 2, 0), 2, 1)[..., None]
    return np.rint(np.asarray(c0, np.float64) * (1 - t) + np.asarray(c1, np.float64) * t).astype(np.uint8)


def _tail_block(amplitude):
    c = np.zeros((8, 8))
    c[7, 7] = amplitude
    return idct(c)


def luma_tail(by, bx):
    """Grey, every block the (7, 7) basis function at amplitude 520: at quality 92 one coefficient of size 6 behind 62 zeros."""
    return _grey(_tile(np.broadcast_to(_tail_block(520.0), (by, bx, 8, 8))) + 128)


def chroma_tail(my, mx):
    """Y = 128, Cb the (7, 7) basis function at amplitude 300 (one block per MCU), Cr = 128."""
    cb = np.rint(_tile(np.broadcast_to(_tail_block(300.0), (my, mx, 8, 8))))
    cb = np.repeat(np.repeat(cb, 2, 0), 2, 1)
    rgb = np.stack([np.full_like(cb, 128.0), 128 - 0.344136 * cb, 128 + 1.772 * cb], -1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def _behind_noise(tail, n_noise, seed):
    """One row of MCUs: n_noise MCUs of noise, then the tail image's MCUs (their words then start at other bit positions)."""
    out = np.concatenate([np.random.default_rng(seed).integers(0, 256, (tail.shape[0], 16 * n_noise, 3), dtype=np.uint8), tail], 1)
    return np.ascontiguousarray(out)


def _magnitude(rng, size):
    return int(rng.integers(1 << (size - 1), 1 << size)) * int(rng.choice([-1, 1]))


def sparse_blocks(rng, by, bx):
    """[by, bx, 8, 8] samples about 0: per block a DC in +-1000 and 1-4 AC coefficients at random zigzag positions, their
    magnitudes drawn per size category 1..10 (orthonormal scale: the quantised values at quality 100)."""
    coef = np.zeros((by, bx, 64))
    for b in coef.reshape(-1, 64):
        b[0] = rng.integers(-1000, 1001)
        for k in rng.choice(np.arange(1, 64), int(rng.integers(1, 5)), replace=False):
            b[ZIGZAG[k]] = _magnitude(rng, int(rng.integers(1, 11)))
    return idct(coef.reshape(by, bx, 8, 8))


def symbol_blocks(rng):
    """[20, 16, 8, 8] samples about 0 that aim at every AC symbol (run, size 1..10) twice: as the first coefficient of a block
    (at zigzag run + 1), and behind a small coefficient at a random place.  The magnitude sits low in its category, since a
    big coefficient clips; what comes out is what stats() says."""
    coef = np.zeros((320, 64))
    for run in range(16):
        for size in range(1, 11):
            m = max(1, int(round((1 << (size - 1)) * (1.12 if size > 8 else 1.3)))) * int(rng.choice([-1, 1]))
            coef[run * 10 + size - 1, ZIGZAG[run + 1]] = m
            b = coef[160 + run * 10 + size - 1]
            k = int(rng.integers(1, 63 - run))
            b[ZIGZAG[k]] = rng.choice([-2, 2])
            b[ZIGZAG[k + run + 1]] = m
    return idct(coef.reshape(20, 16, 8, 8))


def _chroma_image(blocks, rng):
    """Every block one MCU: the pattern along blue-yellow (Cb) or red-cyan (Cr), chosen per MCU."""
    rows = []
    for row in blocks:
        rows.append(np.concatenate([_along(b, *((YELLOW, BLUE) if rng.integers(2) else (CYAN, RED))) for b in row], 1))
    return np.ascontiguousarray(np.concatenate(rows, 0))


def _columns(colours, width, height=32):
    out = np.zeros((height, width, 3), np.uint8)
    for k in range(width // 16):
        out[:, 16 * k:16 * k + 16] = colours[k % len(colours)]
    return out


def stuffing_candidate(seed):
    """(image, quality) number `seed` of the search for streams with 0xFF bytes in particular places: noise or saturated
    noise of a random size below 65 x 65 at quality 95, 98 or 100."""
    rng = np.random.default_rng(seed)
    W, H = int(rng.integers(17, 65)), int(rng.integers(17, 65))
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if seed % 2 == 0 else (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return img, int(rng.choice([100, 98, 95]))


def stuffing(st):
    """Which byte-stuffing situations the unstuffed intervals of a stats() hold: "pair" (two consecutive 0xFF), "last" (0xFF
    as the last byte of an interval), "pos0".."pos3" (0xFF at that byte of a 32-bit word), "round" (0xFF as the last byte of
    a pack round of 1024 bytes)."""
    out = set()
    for iv in st["intervals"]:
        ff = np.flatnonzero(np.frombuffer(iv, np.uint8) == 255)
        if len(ff):
            out |= {f"pos{k}" for k in set(ff % 4)}
            out |= {"pair"} if (np.diff(ff) == 1).any() else set()
            out |= {"last"} if ff[-1] == len(iv) - 1 else set()
            out |= {"round"} if (ff % 1024 == 1023).any() else set()
    return out


def edge_images():
    """name -> ([H, W, 3] uint8, quality): inputs that reach what images() does not (tests/test_jpeg_host.py says what each
    kind must emit): words of 55 and 51 bits behind three ZRL codes at every bit position, nearly every AC symbol, DC
    categories 10 and 11, 0xFF bytes at the places where byte stuffing can go wrong."""
    out = {"luma_tail": (luma_tail(2, 4), 92), "chroma_tail": (chroma_tail(2, 2), 93)}
    for seed in range(3):  # the tail words at all 32 bit positions
        out[f"luma_tail_behind_noise{seed}"] = (_behind_noise(luma_tail(2, 16), 1 + seed, seed), 92)
        out[f"chroma_tail_behind_noise{seed}"] = (_behind_noise(chroma_tail(1, 22), 1 + seed, seed), 92)
    rng = np.random.default_rng(0)
    out["sparse_luma"] = (_grey(_tile(sparse_blocks(rng, 12, 12)) + 128), 100)
    out["sparse_chroma"] = (_chroma_image(sparse_blocks(rng, 8, 8), rng), 100)
    out["symbols_luma"] = (_grey(_tile(symbol_blocks(rng)) + 128), 100)
    out["symbols_chroma"] = (_chroma_image(symbol_blocks(rng), rng), 100)
    for q in (100, 90):  # DC differences of categories 11 and 10, in both tables
        out[f"dc_black_white_q{q}"] = (_columns([(0, 0, 0), (255, 255, 255)], 64), q)
        out[f"dc_colours_q{q}"] = (_columns([BLUE, YELLOW, RED, CYAN], 128), q)
    out["stuffing_pair_last"] = stuffing_candidate(31)  # 43 x 60: 0xFF 0xFF, 0xFF at the end of an interval (R = 1)
    out["stuffing_round"] = stuffing_candidate(27)  # 17 x 50: 0xFF as byte 1023 of an interval (R = 8 and more than all MCUs)
    return out


def restart_cases(W, H):
    """The restart intervals of the parity tests: 1, 3, 8, one MCU row, more than all MCUs (DRI present, no marker)."""
    mw, mh = (W + 15) // 16, (H + 15) // 16
    return (1, 3, 8, mw, mw * mh + 5)


# ---- seeded random cases (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py, tests/fuzz_jpeg.py) ----------------------------------
FAMILIES = ("noise", "saturated", "smooth", "shapes", "sparse")


def content(rng, kind, H, W):
    """[H, W, 3] uint8 of one family."""
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    if kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        a = rng.integers(1, 8, 6)
        return np.stack([(xx * a[0] + yy * a[1]) % 256, (xx * a[2] + yy * a[3]) % 256, (xx * a[4] + yy * a[5]) % 256], -1).astype(np.uint8)
    if kind == "shapes":  # render-like: a flat background, a few flat rectangles
        out = np.empty((H, W, 3), np.uint8)
        out[:] = rng.integers(0, 256, 3) * int(rng.integers(2))
        for _ in range(int(rng.integers(1, 6))):
            y, x = int(rng.integers(H)), int(rng.integers(W))
            out[y:y + int(rng.integers(1, H + 1)), x:x + int(rng.integers(1, W + 1))] = rng.integers(0, 256, 3)
        return out
    if kind == "sparse":
        by, bx = (H + 7) // 8, (W + 7) // 8
        blocks = sparse_blocks(rng, by, bx)
        if rng.integers(2):
            return np.ascontiguousarray(_grey(_tile(blocks) + 128)[:H, :W])
        return np.ascontiguousarray(_chroma_image(blocks[:(by + 1) // 2, :(bx + 1) // 2], rng)[:H, :W])
    raise ValueError(kind)


def fuzz_case(seed, max_side=96):
    """Case number `seed`: {"kind", "frames" [N, H, W, 3] (N 1..4), "quality" 1..100, "R" (1, small, one MCU row, more than
    all MCUs, 65535), "offset": the odd byte offset (1 or 3) at which the GPU tests place the frames}."""
    rng = np.random.default_rng(1000 + seed)
    kind = FAMILIES[seed % len(FAMILIES)]
    side = lambda: int(rng.integers(1, max_side + 1) if rng.integers(4) else rng.choice([1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33]))
    W, H, N = side(), side(), int(rng.integers(1, 5))
    mw, mh = (W + 15) // 16, (H + 15) // 16
    R = int(rng.choice([1, 2, int(rng.integers(1, 20)), mw, mw * mh, mw * mh + 5, 65535]))
    frames = np.stack([content(rng, kind, H, W) for _ in range(N)])
    return dict(kind=kind, frames=frames, quality=int(rng.integers(1, 101)), R=R, offset=int(rng.choice([1, 3])))
