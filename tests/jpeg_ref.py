"""numpy restatement of include/codetr_jpeg.h: `encode(rgb, quality, subsampling) -> bytes` reproduces the file of
hip_ops.encode_jpeg byte for byte, and `decode(data) -> rgb` is a minimal baseline decoder for the files `encode` writes
(Huffman decode, dequantise, float inverse DCT, chroma replication, colour) -- the tests need no imaging library.

Every table is typed here on its own (not read from the library): test_jpeg_cpu.py pins them to Pillow's and to the
library's header.  `encode(..., stats=dict)` counts what the entropy coder did, for the coverage conditions of the case list.
"""
import math

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63]

BASE_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
            87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
            72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROM = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
              99, 99, 99, 99] + [99] * 32

DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROM = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROM = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HUFF = (DC_LUM, AC_LUM, DC_CHROM, AC_CHROM)   # the order of the DHT segments; ids 0x00, 0x10, 0x01, 0x11

# round(8192 * c(k) / 2 * cos((2n + 1) k pi / 16))
DCT = np.array([[round(8192 * (math.sqrt(0.5) if k == 0 else 1.0) / 2 * math.cos((2 * n + 1) * k * math.pi / 16))
                 for n in range(8)] for k in range(8)], np.int64)


def codes(spec):
    """symbol -> (code, length)"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_table(quality, base):
    """the 64 divisors in natural order"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def mcu_size(subsampling):
    if subsampling not in ("420", "444"):
        raise ValueError(subsampling)
    return 16 if subsampling == "420" else 8


def header(H, W, quality, subsampling):
    """SOI up to and including SOS"""
    px = mcu_size(subsampling)

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0")
    for i, base in enumerate((BASE_LUM, BASE_CHROM)):
        q = quant_table(quality, base)
        out += seg(0xDB, bytes([i]) + bytes(q[z] for z in ZIGZAG))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big")
               + bytes([3, 1, 0x22 if subsampling == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFF):
        out += seg(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, (-(-W // px)).to_bytes(2, "big"))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def ycc_planes(rgb, subsampling):
    """the padded sample planes (Y, Cb, Cr) as int64; chroma subsampled at 4:2:0"""
    px = mcu_size(subsampling)
    H, W = rgb.shape[:2]
    Hp, Wp = -(-H // px) * px, -(-W // px) * px
    ys = np.minimum(np.arange(Hp), H - 1)
    xs = np.minimum(np.arange(Wp), W - 1)
    p = rgb[ys][:, xs].astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = np.minimum((-11058 * r - 21710 * g + 32768 * b + 8388608 + 32768) >> 16, 255)
    cr = np.minimum((32768 * r - 27439 * g - 5329 * b + 8388608 + 32768) >> 16, 255)
    if subsampling == "420":
        cb = (cb[0::2, 0::2] + cb[0::2, 1::2] + cb[1::2, 0::2] + cb[1::2, 1::2] + 2) >> 2
        cr = (cr[0::2, 0::2] + cr[0::2, 1::2] + cr[1::2, 0::2] + cr[1::2, 1::2] + 2) >> 2
    return y, cb, cr


def quantised_blocks(plane, table):
    """[h, w] samples -> [h / 8, w / 8, 64] quantised coefficients in zigzag order"""
    h, w = plane.shape
    s = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)        # [by, bx, y, x]
    t = (np.einsum("ux,abyx->abyu", DCT, s) + 512) >> 10
    f = (np.einsum("vy,abyu->abvu", DCT, t) + 32768) >> 16
    assert np.abs(f).max() <= 1024
    q = np.asarray(table, np.int64).reshape(8, 8)
    out = np.sign(f) * ((np.abs(f) + q // 2) // q)
    return out.reshape(h // 8, w // 8, 64)[:, :, ZIGZAG]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.raw, self.out = 0, 0, bytearray(), bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        if self.n >= 64:   # whole bytes leave the accumulator
            keep = self.n & 7
            self.raw += (self.acc >> keep).to_bytes(self.n >> 3, "big")
            self.acc &= (1 << keep) - 1
            self.n = keep

    def flush_row(self, stats):
        pad = -self.n % 8
        self.acc, self.n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        raw = bytes(self.raw) + self.acc.to_bytes(self.n // 8, "big")
        stats["stuffed"] += raw.count(b"\xff")
        self.out += raw.replace(b"\xff", b"\xff\x00")
        self.acc, self.n, self.raw = 0, 0, bytearray()


def _magnitude(v):
    n = abs(int(v)).bit_length()
    return n, (v - 1 if v < 0 else v) & ((1 << n) - 1)


def new_stats():
    return dict(zrl=0, no_eob=0, stuffed=0, dc_categories=set(), negative_dc=0, zero_dc=0, rows=0, blocks=0)


def encode(rgb, quality=90, subsampling="420", stats=None):
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or min(rgb.shape[:2]) < 1:
        raise ValueError("expected an RGB uint8 image [H, W, 3]")
    if not 1 <= quality <= 100:
        raise ValueError(quality)
    stats = new_stats() if stats is None else stats
    H, W = rgb.shape[:2]
    px = mcu_size(subsampling)
    y, cb, cr = ycc_planes(rgb, subsampling)
    qy = quantised_blocks(y, quant_table(quality, BASE_LUM))
    qcb = quantised_blocks(cb, quant_table(quality, BASE_CHROM))
    qcr = quantised_blocks(cr, quant_table(quality, BASE_CHROM))
    dc_codes = (codes(DC_LUM), codes(DC_CHROM))
    ac_codes = (codes(AC_LUM), codes(AC_CHROM))
    rows, mcus = -(-H // px), -(-W // px)
    bits = _Bits()
    for r in range(rows):
        pred = [0, 0, 0]
        for m in range(mcus):
            if subsampling == "420":
                blocks = [(0, qy[2 * r, 2 * m]), (0, qy[2 * r, 2 * m + 1]), (0, qy[2 * r + 1, 2 * m]),
                          (0, qy[2 * r + 1, 2 * m + 1]), (1, qcb[r, m]), (2, qcr[r, m])]
            else:
                blocks = [(0, qy[r, m]), (1, qcb[r, m]), (2, qcr[r, m])]
            for comp, blk in blocks:
                ti = 1 if comp else 0
                blk = [int(v) for v in blk]
                diff = blk[0] - pred[comp]
                pred[comp] = blk[0]
                n, mag = _magnitude(diff)
                stats["dc_categories"].add(n)
                stats["negative_dc"] += diff < 0
                stats["zero_dc"] += diff == 0
                stats["blocks"] += 1
                bits.put(*dc_codes[ti][n])
                bits.put(mag, n)
                run = 0
                for v in blk[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        bits.put(*ac_codes[ti][0xF0])
                        stats["zrl"] += 1
                        run -= 16
                    n, mag = _magnitude(v)
                    bits.put(*ac_codes[ti][(run << 4) | n])
                    bits.put(mag, n)
                    run = 0
                if run:
                    bits.put(*ac_codes[ti][0])
                else:
                    stats["no_eob"] += 1
        bits.flush_row(stats)
        stats["rows"] += 1
        if r + 1 < rows:
            bits.out += bytes([0xFF, 0xD0 + (r & 7)])
    return header(H, W, quality, subsampling) + bytes(bits.out) + b"\xff\xd9"


# ---- the decoder ----------------------------------------------------------------------------------------------------------

def segments(data):
    """[(marker, payload)] from SOI to SOS, and the offset of the scan"""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF, p
        marker = data[p + 1]
        n = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((marker, data[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return out, p


class _Reader:
    def __init__(self, raw):
        self.v, self.n = int.from_bytes(raw, "big"), 8 * len(raw)

    def take(self, k):
        self.n -= k
        assert self.n >= 0
        return (self.v >> self.n) & ((1 << k) - 1)

    def symbol(self, table):
        code, length = 0, 0
        while True:
            code, length = (code << 1) | self.take(1), length + 1
            if (code, length) in table:
                return table[(code, length)]
            assert length < 16


def _extend(bits, n):
    return bits if n == 0 or bits >> (n - 1) else bits - (1 << n) + 1


def decode(data):
    """a file written by `encode` (or by the library) -> RGB uint8 [H, W, 3]"""
    segs, p = segments(data)
    qt, huff = {}, {}
    for marker, body in segs:
        if marker == 0xDB:
            q = np.zeros(64, np.float64)
            q[ZIGZAG] = list(body[1:65])
            qt[body[0]] = q
        elif marker == 0xC4:
            bits, vals = list(body[1:17]), list(body[17:])
            huff[body[0]] = {cl: sym for sym, cl in codes((bits, vals)).items()}
        elif marker == 0xC0:
            H, W = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            sub = "420" if body[7] == 0x22 else "444"
        elif marker == 0xDD:
            interval = int.from_bytes(body, "big")
    assert data[-2:] == b"\xff\xd9"
    px = mcu_size(sub)
    rows, mcus = -(-H // px), -(-W // px)
    assert interval == mcus
    scan = data[p:-2]
    parts, start, i = [], 0, 0
    while i < len(scan) - 1:   # split at the RST markers
        if scan[i] == 0xFF and scan[i + 1] != 0:
            assert scan[i + 1] == 0xD0 + (len(parts) & 7)
            parts.append(scan[start:i])
            start = i = i + 2
        else:
            i += 2 if scan[i] == 0xFF else 1
    parts.append(scan[start:])
    assert len(parts) == rows
    basis = np.array([[(math.sqrt(0.5) if k == 0 else 1.0) / 2 * math.cos((2 * n + 1) * k * math.pi / 16) for n in range(8)]
                      for k in range(8)])
    planes = [np.zeros((rows * px, mcus * px)), np.zeros((rows * 8, mcus * 8)), np.zeros((rows * 8, mcus * 8))]
    if sub == "444":
        layout = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    else:
        layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)]
    for r, part in enumerate(parts):
        rd = _Reader(part.replace(b"\xff\x00", b"\xff"))
        pred = [0, 0, 0]
        for m in range(mcus):
            for comp, by, bx in layout:
                ti = 1 if comp else 0
                blk = np.zeros(64)
                n = rd.symbol(huff[ti])
                pred[comp] += _extend(rd.take(n), n)
                blk[0] = pred[comp]
                k = 1
                while k < 64:
                    sym = rd.symbol(huff[0x10 | ti])
                    if sym == 0:
                        break
                    k += sym >> 4
                    if sym != 0xF0:
                        blk[k] = _extend(rd.take(sym & 15), sym & 15)
                    k += 1
                f = np.zeros(64)
                f[ZIGZAG] = blk
                f = (f * qt[ti]).reshape(8, 8)
                s = basis.T @ f @ basis + 128.0
                per = 2 if comp == 0 and sub == "420" else 1
                y0, x0 = (r * per + by) * 8, (m * per + bx) * 8
                planes[comp][y0:y0 + 8, x0:x0 + 8] = s
        left = rd.n
        assert left < 8 and rd.take(left) == (1 << left) - 1   # only the row's 1-padding is left
    y, cb, cr = planes
    if sub == "420":
        cb, cr = cb.repeat(2, 0).repeat(2, 1), cr.repeat(2, 0).repeat(2, 1)
    y, cb, cr = y[:H, :W], cb[:H, :W] - 128.0, cr[:H, :W] - 128.0
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)
