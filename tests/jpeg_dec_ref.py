"""numpy restatement of include/codetr_jpeg_dec.h: `parse(data)` reads the header, `decode(data) -> (rgb, status)` is the
sequential decoder of the header's rule (general over tables, DRI and sampling) and `decode_chunked` the same scan decoded
as the self-synchronising chunked fixed point the kernels run.  Integer arithmetic throughout, so the kernels are held to
it byte for byte; test_jpeg_dec_cpu.py pins it to Pillow.

Everything is typed here on its own; only the numeric codes are compared with the header by the tests.  `stats` dicts
count what the entropy decoder met, for the coverage conditions of the case list.
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63]
CHUNK, RUN = 64, 256
E_BADARG, E_TOO_LARGE, E_UNSUPPORTED = -1, -3, -4
MAX_SIDE, MAX_FILE = 32767, (1 << 27) - 1
REASONS = ("", "progressive", "extended", "lossless", "hierarchical", "arithmetic", "precision", "components", "rgb_ids",
           "adobe", "sampling", "quant16", "multiscan", "scan_params")
R = {name: i for i, name in enumerate(REASONS) if name}
STATUS = ("ok", "bad_code", "dc_category", "index", "exhausted", "rst", "interval")
S = {name: i for i, name in enumerate(STATUS)}
DEAD = -1


class ParseError(ValueError):
    def __init__(self, code, reason=0, info=None):
        super().__init__(f"code {code}, reason {REASONS[reason] if reason else None}")
        self.code, self.reason, self.info = code, reason, info


def parse(data):
    """-> dict(H, W, ncomp, dri, scan_offset, scan_bytes, comps [(h, v, tq, td, ta)], hmax, vmax, mcus_x, mcus_y, bpm,
    nblocks, quant {t: [64] natural}, huff {(cls, t): (bits [16], vals [...])}); ParseError(code, reason) otherwise"""
    f, n = bytes(data), len(data)
    if n < 4 or f[:2] != b"\xff\xd8":
        raise ParseError(E_BADARG)
    if n > MAX_FILE:
        raise ParseError(E_TOO_LARGE)
    reasons, quant, huff, info, ids, p, too_large = set(), {}, {}, None, [], 2, False
    while True:
        if p + 2 > n or f[p] != 0xFF:
            raise ParseError(E_BADARG)
        m = f[p + 1]
        if m == 0xFF:
            p += 1
            continue
        p += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0x00, 0xD8, 0xD9) or p + 2 > n:
            raise ParseError(E_BADARG)
        ln = f[p] << 8 | f[p + 1]
        if ln < 2 or p + ln > n:
            raise ParseError(E_BADARG)
        s = f[p + 2:p + ln]
        if m == 0xDB:
            q = 0
            while q < len(s):
                pq, tq = s[q] >> 4, s[q] & 15
                size = 128 if pq else 64
                if tq > 3 or pq > 1 or q + 1 + size > len(s):
                    raise ParseError(E_BADARG)
                if pq:
                    reasons.add(R["quant16"])
                else:
                    t = [0] * 64
                    for k in range(64):
                        t[ZIGZAG[k]] = s[q + 1 + k]
                    quant[tq] = t
                q += 1 + size
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if q + 17 > len(s):
                    raise ParseError(E_BADARG)
                tc, th = s[q] >> 4, s[q] & 15
                bits = list(s[q + 1:q + 17])
                code = 0
                for l in range(16):
                    code += bits[l]
                    if code > 1 << (l + 1):
                        raise ParseError(E_BADARG)
                    code <<= 1
                if tc > 1 or th > 3 or sum(bits) > 256 or q + 17 + sum(bits) > len(s):
                    raise ParseError(E_BADARG)
                huff[(tc, th)] = (bits, list(s[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xDD:
            if len(s) != 2:
                raise ParseError(E_BADARG)
            dri = s[0] << 8 | s[1]
            info = dict(info or {}, dri=dri)
        elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):
            if (info and "H" in info) or len(s) < 6:
                raise ParseError(E_BADARG)
            H, W, nc = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            if len(s) != 6 + 3 * nc or nc < 1 or H == 0 or W == 0:
                raise ParseError(E_BADARG)
            info = dict(info or {}, H=H, W=W, ncomp=nc)
            too_large = H > MAX_SIDE or W > MAX_SIDE
            for name, cond in (("progressive", m == 0xC2), ("extended", m == 0xC1), ("lossless", m == 0xC3),
                               ("hierarchical", 0xC5 <= m <= 0xC7), ("arithmetic", m >= 0xC9), ("precision", m == 0xC0 and s[0] != 8)):
                if cond:
                    reasons.add(R[name])
            if nc not in (1, 3):
                reasons.add(R["components"])
            else:
                comps = []
                for c in range(nc):
                    ids.append(s[6 + 3 * c])
                    h, v, tq = s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]
                    if not (1 <= h <= 4 and 1 <= v <= 4 and tq <= 3):
                        raise ParseError(E_BADARG)
                    comps.append([h, v, tq, 0, 0])
                if nc == 1:
                    comps[0][0] = comps[0][1] = 1
                else:
                    if ids == [ord("R"), ord("G"), ord("B")]:
                        reasons.add(R["rgb_ids"])
                    if [c[:2] for c in comps[1:]] != [[1, 1], [1, 1]] or comps[0][:2] not in ([1, 1], [2, 1], [2, 2]):
                        reasons.add(R["sampling"])
                info["comps"] = comps
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe" and s[11] != 1:
                reasons.add(R["adobe"])
        elif m == 0xDA:
            if not info or "H" not in info or len(s) < 1:
                raise ParseError(E_BADARG)
            ns = s[0]
            if not 1 <= ns <= 4 or len(s) != 4 + 2 * ns:
                raise ParseError(E_BADARG)
            scan = p + ln
            eoi = f.rfind(b"\xff\xd9", scan)
            if eoi < 0:
                raise ParseError(E_BADARG)
            info.update(scan_offset=scan, scan_bytes=eoi - scan, dri=info.get("dri", 0))
            if too_large:
                raise ParseError(E_TOO_LARGE)
            if ns != info["ncomp"]:
                reasons.add(R["multiscan"])
            if tuple(s[1 + 2 * ns:]) != (0, 63, 0):
                reasons.add(R["scan_params"])
            if reasons:
                raise ParseError(E_UNSUPPORTED, min(reasons), info)
            for c, comp in enumerate(info["comps"]):
                td, ta = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if s[1 + 2 * c] != ids[c] or td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff or comp[2] not in quant:
                    raise ParseError(E_BADARG)
                comp[3], comp[4] = td, ta
            hmax, vmax = info["comps"][0][:2]
            info.update(hmax=hmax, vmax=vmax, mcus_x=-(-info["W"] // (8 * hmax)), mcus_y=-(-info["H"] // (8 * vmax)),
                        bpm=1 if info["ncomp"] == 1 else hmax * vmax + 2, quant=quant, huff=huff)
            info["nblocks"] = info["mcus_x"] * info["mcus_y"] * info["bpm"]
            info["comps"] = [tuple(c) for c in info["comps"]]
            return info
        p += ln


# ---- entropy decoding ---------------------------------------------------------------------------------------------------------
class ScanContext:
    """the scan with, for every raw position, the 40-bit window the reader sees there"""

    def __init__(self, info, scan):
        self.info, self.len = info, len(scan)
        n = len(scan)
        raw = np.frombuffer(bytes(scan), np.uint8).astype(np.int64)
        ext = np.concatenate([raw, [0xD9, 0xD9]])                       # (never read as data: positions >= n stop)
        ff = raw == 0xFF
        stuffed = ff & (np.arange(n) + 1 < n) & (ext[1:n + 1] == 0)
        stop = ff & ~stuffed
        nxt = np.where(stuffed, np.arange(n) + 2, np.arange(n) + 1)
        nxt_ext = np.concatenate([nxt, [n, n, n]])                       # positions n, n + 1: stay
        stop_ext = np.concatenate([stop, [True, True, True]])
        byte_ext = np.concatenate([raw, [0, 0, 0]])
        pos = np.arange(n + 3)
        acc, cnt, cur = np.zeros(n + 3, np.int64), np.zeros(n + 3, np.int64), pos.copy()
        halted = np.full(n + 3, -1, np.int64)
        for _ in range(5):
            live = (halted < 0) & ~stop_ext[cur]
            newly = (halted < 0) & stop_ext[cur]
            halted = np.where(newly, np.minimum(cur, n + 2), halted)
            acc = np.where(live, acc << 8 | byte_ext[cur], acc)
            cnt = cnt + live
            cur = np.where(live, nxt_ext[cur], cur)
        acc = acc << (8 * (5 - cnt))
        self.acc, self.cnt, self.stop = acc.tolist(), cnt.tolist(), halted.tolist()
        self.nxt, self.raw = nxt_ext.tolist(), bytes(scan)
        bpm, nc = info["bpm"], info["ncomp"]
        self.comp = [0 if nc == 1 or i < bpm - 2 else i - (bpm - 2) + 1 for i in range(bpm)]
        self.luts = {}
        for key, (bits, vals) in info["huff"].items():
            self.luts[key] = _lut(bits, vals)
        self.dc = [self.luts[(0, c[3])] for c in info["comps"]]
        self.ac = [self.luts[(1, c[4])] for c in info["comps"]]

    def rst_at(self, q):
        return 0 <= q and q + 1 < self.len and self.raw[q] == 0xFF and (self.raw[q + 1] & 0xF8) == 0xD0


def _lut(bits, vals):
    """16-bit prefix -> length << 8 | symbol, 0 where no code matches (the canonical rule of T.81 F.2.2.3)"""
    lut = np.zeros(1 << 16, np.int32)
    vals = list(vals) + [0] * (256 - len(vals))
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lut[code << (16 - l):(code + 1) << (16 - l)] = l << 8 | vals[k & 255]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def decode_chunk(cx, pos, mk, chunk_begin, chunk_end, final=False, first_blk=0, pred_in=(0, 0, 0), coef=None, stats=None, max_steps=None):
    """the symbols that start in [.., chunk_end) from the entry state (a dead one stands for the guess: chunk_begin,
    block 0, index 0) -> dict(pos, mk, nblk, reset, dc, err)"""
    info = cx.info
    bpm, nblocks, dri = info["bpm"], info["nblocks"], info["dri"]
    o = dict(pos=pos, mk=mk, nblk=0, reset=0, dc=list(pred_in) if final else [0, 0, 0], err=0)
    if pos < 0:
        pos, mk = chunk_begin * 8, 0
    p, b, blk, k = pos >> 3, pos & 7, mk >> 6, mk & 63
    dead, nblk, err, dc, step = False, 0, 0, o["dc"], 0
    acc, cnts, stops, nxt = cx.acc, cx.cnt, cx.stop, cx.nxt

    def wrap(v):
        return (v + 2 ** 31) % 2 ** 32 - 2 ** 31

    while p < chunk_end and (max_steps is None or step < max_steps):
        step += 1
        cnt = cnts[p]
        avail = min(max(cnt * 8 - b, 0), 32)
        w = ((acc[p] << b) >> 8) & 0xFFFFFFFF
        comp = cx.comp[blk]
        hit = (cx.dc[comp] if k == 0 else cx.ac[comp])[w >> 16]
        ln, sym = hit >> 8, hit & 255
        stopped, ssss, code = False, 0, 0
        if not ln:
            if avail >= 16:
                code = S["bad_code"]
            else:
                stopped = True
        elif ln > avail:
            stopped = True
        elif k == 0 and sym > 15:
            code = S["dc_category"]
        else:
            ssss = sym if k == 0 else sym & 15
            stopped = ln + ssss > avail
        if stopped:
            if cx.rst_at(stops[p]):
                if final and not err and first_blk + nblk < nblocks:
                    err = S["rst"]
                p, b, blk, k = stops[p] + 2, 0, 0, 0
                o["reset"], dc[0], dc[1], dc[2] = 1, 0, 0, 0
                continue
            code = S["exhausted"]
        g = first_blk + nblk
        done = False
        if not code:
            v = 0
            if ssss:
                v = ((w << ln) & 0xFFFFFFFF) >> (32 - ssss)
                if v < 1 << (ssss - 1):
                    v -= (1 << ssss) - 1
            if k == 0:
                dc[comp] = wrap(dc[comp] + v)
                if final and g < nblocks:
                    coef[g, 0] = min(max(dc[comp], -32768), 32767)
                if stats is not None and ssss > stats.get("max_dc_category", 0):
                    stats["max_dc_category"] = ssss
                k = 1
            elif ssss == 0:
                if sym >> 4 == 15:
                    k += 16
                    if stats is not None:
                        stats["zrl"] = stats.get("zrl", 0) + 1
                    if k > 63:
                        code = S["index"]
                else:
                    done = True
            else:
                k += sym >> 4
                if k > 63:
                    code = S["index"]
                else:
                    if final and g < nblocks:
                        coef[g, ZIGZAG[k]] = v
                    k += 1
                    if k == 64:
                        done = True
                        if stats is not None:
                            stats["no_eob"] = stats.get("no_eob", 0) + 1
        if code:
            if final and not err and g < nblocks:
                err = code
            dead = True
            break
        b += ln + ssss
        while b >= 8:
            p = nxt[p]
            b -= 8
        if done:
            nblk += 1
            k = 0
            blk += 1
            if blk >= bpm:
                blk = 0
                q = nxt[p] if b else p
                rst = cx.rst_at(q)
                if final and first_blk + nblk < nblocks and not err:
                    M = (first_blk + nblk) // bpm
                    expected = dri > 0 and M % dri == 0
                    if rst and not expected:
                        err = S["interval"]
                    elif rst and (cx.raw[q + 1] & 7) != ((M // dri - 1) & 7):
                        err = S["rst"]
                    elif not rst and expected:
                        err = S["rst"]
                if rst:
                    p, b = q + 2, 0
                    o["reset"], dc[0], dc[1], dc[2] = 1, 0, 0, 0
    o.update(pos=DEAD if dead else p * 8 + b, mk=0 if dead else blk * 64 + k, nblk=nblk, err=err)
    return o


def decode_coefficients(info, scan, stats=None):
    """the sequential decode -> (coefficients [nblocks, 64] int16 in natural order, status)"""
    cx = ScanContext(info, scan)
    coef = np.zeros((info["nblocks"], 64), np.int16)
    o = decode_chunk(cx, 0, 0, 0, 1 << 62, final=True, coef=coef, stats=stats)
    return coef, o["err"]


def decode_chunked(info, scan, chunk=CHUNK, run=RUN, stats=None):
    """the fixed point the kernels run: per run of chunks from guessed entries, then the runs linked in order, a scan of
    block counts and DC sums, and one final decode per chunk -> (coefficients, status); stats: rounds per run, rounds of
    the repaired runs, and per chunk the record [entry pos, entry mk, exit pos, exit mk, blocks, reset, dc sums]"""
    cx = ScanContext(info, scan)
    n = len(scan) // chunk + 1
    ends = [(c + 1) * chunk for c in range(n - 1)] + [1 << 62]
    steps = 8 * chunk + 40
    entry = [(c * chunk * 8, 0) for c in range(n)]
    lane = [None] * n

    def fixed_point(c0, c1, dirty):
        rounds = 0
        while dirty:
            rounds += 1
            for c in dirty:
                lane[c] = decode_chunk(cx, entry[c][0], entry[c][1], c * chunk, ends[c], max_steps=steps)
            again = []
            for c in range(c0 + 1, c1):
                want = (lane[c - 1]["pos"], lane[c - 1]["mk"])
                if want != entry[c]:
                    entry[c] = want
                    again.append(c)
            dirty = again
        return rounds

    rounds = [fixed_point(c0, min(c0 + run, n), list(range(c0, min(c0 + run, n)))) for c0 in range(0, n, run)]
    repaired = []
    for c0 in range(run, n, run):
        want = (lane[c0 - 1]["pos"], lane[c0 - 1]["mk"])
        if want != entry[c0]:
            entry[c0] = want
            repaired.append(fixed_point(c0, min(c0 + run, n), [c0]))
    if stats is not None:
        stats.update(rounds=rounds, repaired=repaired, chunks=n)
        stats["records"] = [[entry[c][0], entry[c][1], lane[c]["pos"], lane[c]["mk"], lane[c]["nblk"], lane[c]["reset"]] + lane[c]["dc"]
                            for c in range(n)]
    coef = np.zeros((info["nblocks"], 64), np.int16)
    blocks, pred, keys = 0, [0, 0, 0], []
    for c in range(n):
        o = decode_chunk(cx, entry[c][0], entry[c][1], c * chunk, ends[c], final=True, first_blk=blocks, pred_in=pred, coef=coef,
                         max_steps=steps)
        assert (o["pos"], o["mk"], o["nblk"]) == (lane[c]["pos"], lane[c]["mk"], lane[c]["nblk"])
        if o["err"]:
            keys.append(o["err"])
        blocks += lane[c]["nblk"]
        pred = list(lane[c]["dc"]) if lane[c]["reset"] else [(a + d + 2 ** 31) % 2 ** 32 - 2 ** 31 for a, d in zip(pred, lane[c]["dc"])]
    return coef, (keys[0] if keys else 0)


# ---- pixels ---------------------------------------------------------------------------------------------------------------------
def _pass(v, shift):
    """one 1-D pass of jidctint over v[..., 8] (uint32 arithmetic, arithmetic shift of the signed reinterpretation)"""
    u = np.uint32
    v = v.astype(np.uint32)
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., i] for i in range(8))
    z1 = (v2 + v6) * u(4433)
    t2, t3 = z1 - v6 * u(15137), z1 + v2 * u(6270)
    t0, t1 = (v0 + v4) << u(13), (v0 - v4) << u(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v7, v5, v3, v1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * u(9633)
    neg = lambda c: u(2 ** 32 - c)   # noqa: E731
    a0, a1, a2, a3 = a0 * u(2446), a1 * u(16819), a2 * u(25172), a3 * u(12299)
    z1, z2 = z1 * neg(7373), z2 * neg(20995)
    z3, z4 = z3 * neg(16069) + z5, z4 * neg(3196) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)
    return (out + u(1 << (shift - 1))).view(np.int32) >> shift


def idct(coef, q):
    """coef [n, 64] int16 (natural order), q [64] -> samples [n, 8, 8] uint8"""
    with np.errstate(over="ignore"):
        a = (coef.astype(np.int32).astype(np.uint32) * np.asarray(q, np.uint32)).view(np.int32).reshape(-1, 8, 8)
        t = _pass(a.transpose(0, 2, 1), 11).transpose(0, 2, 1)   # columns
        o = _pass(t, 18)                                          # rows
    return np.clip(o + 128, 0, 255).astype(np.uint8)


def planes(info, coef):
    """the component planes over the whole block grid"""
    nc, bpm, mx, my = info["ncomp"], info["bpm"], info["mcus_x"], info["mcus_y"]
    blocks = coef.reshape(my, mx, bpm, 64)
    out, i = [], 0
    for c, (h, v, tq, _, _) in enumerate(info["comps"]):
        n = h * v if nc > 1 else 1
        hh, vv = (h, v) if nc > 1 else (1, 1)
        px = idct(blocks[:, :, i:i + n].reshape(-1, 64), info["quant"][tq]).reshape(my, mx, vv, hh, 8, 8)
        out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * vv * 8, mx * hh * 8))
        i += n
    return out


def upsample(pl, dw, dh, hs, vs, H, W):
    """the chroma plane at full resolution, H x W (the header's fancy rule, replication for dw <= 2)"""
    a = pl[:dh, :dw].astype(np.int32)
    if hs == 1:
        return a[:H, :W]
    if dw <= 2:
        return np.repeat(np.repeat(a, vs, 0), 2, 1)[:H, :W]
    if vs == 1:
        out = np.empty((dh, 2 * dw), np.int32)
        left, right = np.concatenate([a[:, :1], a[:, :-1]], 1), np.concatenate([a[:, 1:], a[:, -1:]], 1)
        out[:, 0::2] = (3 * a + left + 1) >> 2
        out[:, 1::2] = (3 * a + right + 2) >> 2
        out[:, 0], out[:, -1] = a[:, 0], a[:, -1]
        return out[:H, :W]
    up, down = np.concatenate([a[:1], a[:-1]], 0), np.concatenate([a[1:], a[-1:]], 0)
    s = np.empty((2 * dh, dw), np.int32)
    s[0::2], s[1::2] = 3 * a + up, 3 * a + down
    out = np.empty((2 * dh, 2 * dw), np.int32)
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    out[:, 0], out[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    return out[:H, :W]


def pixels(info, coef):
    H, W, hm, vm = info["H"], info["W"], info["hmax"], info["vmax"]
    pl = planes(info, coef)
    Y = pl[0][:H, :W].astype(np.int32)
    if info["ncomp"] == 1:
        return np.repeat(Y[..., None], 3, 2).astype(np.uint8)
    dw, dh = -(-W // hm), -(-H // vm)
    cb = upsample(pl[1], dw, dh, hm, vm, H, W) - 128
    cr = upsample(pl[2], dw, dh, hm, vm, H, W) - 128
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def scan_of(data, info):
    return bytes(data)[info["scan_offset"]:info["scan_offset"] + info["scan_bytes"]]


def decode(data, stats=None):
    """-> (rgb [H, W, 3] uint8, status)"""
    info = parse(data)
    coef, status = decode_coefficients(info, scan_of(data, info), stats)
    return pixels(info, coef), status
