"""Reference for codetr_frames_to_rgb_u8 (not a test module).

Restates, in numpy int64, the conversion include/codetr_hip.h gives under "Frames": the eight frame formats as planes of
byte rows, nearest chroma (pixel (y, x) reads chroma sample (y >> 1, x >> 1)) and the fixed-point YUV -> RGB with its
four constant sets, recomputed here from (Kr, Kb) and from OpenCV's five published decimals.  Also builds frames of every
format, lays their planes out in a flat buffer with chosen offsets and pitches, and turns a frame into the item the
Inferencer takes."""
import numpy as np

FORMATS = {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3, "gray": 4, "nv12": 5, "nv21": 6, "i420": 7}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
OPENCV_BT601_LIMITED = (1.164, 1.596, -0.391, -0.813, 2.018)   # CY, CRV, CGU, CGV, CBU


def real_coefficients(matrix, range_):
    """(CY, CRV, CGU, CGV, CBU) as real numbers"""
    if (matrix, range_) == ("bt601", "limited"):
        return OPENCV_BT601_LIMITED
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    k = [1.0, 2.0 * (1.0 - kr), -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg, 2.0 * (1.0 - kb)]
    if range_ == "limited":
        k = [k[0] * 255.0 / 219.0] + [c * 255.0 / 224.0 for c in k[1:]]
    return tuple(k)


def coefficients(matrix, range_):
    """the integers round(k * 2^20) and y0"""
    return tuple(int(round(k * (1 << 20))) for k in real_coefficients(matrix, range_)) + (16 if range_ == "limited" else 0,)


def yuv_to_rgb(Y, U, V, matrix="bt601", range_="limited"):
    """arrays of one shape -> uint8 [..., 3]"""
    cy, crv, cgu, cgv, cbu, y0 = coefficients(matrix, range_)
    c = np.maximum(0, np.asarray(Y, np.int64) - y0)
    d, e = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    half = 1 << 19
    rgb = np.stack(((cy * c + crv * e + half) >> 20, (cy * c + cgu * d + cgv * e + half) >> 20,
                    (cy * c + cbu * d + half) >> 20), -1)
    assert np.abs(np.stack((cy * c + crv * e, cy * c + cgu * d + cgv * e, cy * c + cbu * d))).max() < 1 << 30
    return np.clip(rgb, 0, 255).astype(np.uint8)


def plane_shapes(fmt, H, W):
    """[(rows, row bytes)] of the format's planes"""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    if fmt in ("rgb", "bgr"):
        return [(H, 3 * W)]
    if fmt in ("rgba", "bgra"):
        return [(H, 4 * W)]
    if fmt == "gray":
        return [(H, W)]
    if fmt in ("nv12", "nv21"):
        return [(H, W), (ch, 2 * cw)]
    return [(H, W), (ch, cw), (ch, cw)]


def random_planes(fmt, H, W, rng):
    return [rng.integers(0, 256, shape, dtype=np.uint8) for shape in plane_shapes(fmt, H, W)]


def planes_to_rgb(fmt, H, W, planes, matrix="bt601", range_="limited"):
    """the planes (byte rows) of one frame -> RGB uint8 [H, W, 3]"""
    p = [np.asarray(a, np.uint8) for a in planes]
    assert [a.shape for a in p] == plane_shapes(fmt, H, W)
    if fmt in ("rgb", "bgr", "rgba", "bgra"):
        px = p[0].reshape(H, W, -1)
        return np.ascontiguousarray(px[..., [2, 1, 0]] if fmt[0] == "b" else px[..., :3])
    if fmt == "gray":
        return np.repeat(p[0][:, :, None], 3, 2)
    yi, xi = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    if fmt == "i420":
        U, V = p[1][yi, xi], p[2][yi, xi]
    else:
        pairs = p[1].reshape(p[1].shape[0], -1, 2)
        first, second = pairs[yi, xi, 0], pairs[yi, xi, 1]
        U, V = (first, second) if fmt == "nv12" else (second, first)
    return yuv_to_rgb(p[0], U, V, matrix, range_)


def item(fmt, H, W, planes, stacked=None):
    """the planes as the item the Inferencer takes: [H, W, C] / [H, W]; for the YUV formats the 2-D [H * 3 / 2, W] array
    decoders hand out (`stacked`; default: when H and W are even) or the tuple of planes, uv as [ch, cw, 2]"""
    if fmt in ("rgb", "bgr", "rgba", "bgra"):
        return planes[0].reshape(H, W, -1)
    if fmt == "gray":
        return planes[0]
    if stacked is None:
        stacked = H % 2 == 0 and W % 2 == 0
    if stacked:
        return np.concatenate([a.reshape(-1) for a in planes]).reshape(H * 3 // 2, W)
    if fmt == "i420":
        return tuple(planes)
    return planes[0], planes[1].reshape(planes[1].shape[0], -1, 2)


def to_rgb(it, fmt, matrix="bt601", range_="limited"):
    """an Inferencer item (see `item`) -> RGB uint8 [H, W, 3]"""
    if isinstance(it, tuple):
        H, W = it[0].shape
        planes = [np.asarray(a).reshape(a.shape[0], -1) for a in it]
    elif fmt in ("nv12", "nv21", "i420"):
        H, W = it.shape[0] * 2 // 3, it.shape[1]
        flat, planes, at = np.asarray(it).reshape(-1), [], 0
        for rows, rb in plane_shapes(fmt, H, W):
            planes.append(flat[at:at + rows * rb].reshape(rows, rb))
            at += rows * rb
    else:
        H, W = it.shape[:2]
        planes = [np.asarray(it).reshape(H, -1)]
    return planes_to_rgb(fmt, H, W, planes, matrix, range_)


def pack(frames, pad=0, fill=0, start=0, residues=None, dst_residues=None, dst_start=0):
    """Lay frames [(fmt, H, W, planes)] out in one flat source buffer: every plane with pitch = row bytes + pad, the gaps
    and everything else `fill`; plane k (counted over the whole call) starts at the next address whose residue mod 4 is
    residues[k % len(residues)] (default: 0); outputs likewise with dst_residues, one per frame.
    -> (buffer uint8, rows10 [(code, H, W, off0, pitch0, off1, pitch1, off2, pitch2, dst_offset)], dst_bytes).  The last
    plane ends flush with the buffer."""
    residues, dst_residues = residues or [0], dst_residues or [0]
    at, k, dst, placed, rows = start, 0, dst_start, [], []
    for n, (fmt, H, W, planes) in enumerate(frames):
        cols = []
        for a in planes:
            while at % 4 != residues[k % len(residues)]:
                at += 1
            k += 1
            R, rb = a.shape
            pitch = rb + pad
            placed.append((at, pitch, a))
            cols += [at, pitch]
            at += (R - 1) * pitch + rb
        while dst % 4 != dst_residues[n % len(dst_residues)]:
            dst += 1
        rows.append((FORMATS[fmt], H, W) + tuple(cols) + (0,) * (6 - len(cols)) + (dst,))
        dst += H * W * 3
    buf = np.full((at,), fill, np.uint8)
    for off, pitch, a in placed:
        for r in range(a.shape[0]):
            buf[off + r * pitch:off + r * pitch + a.shape[1]] = a[r]
    return buf, rows, dst


def expected_output(frames, rows, dst_bytes, sentinel, matrix="bt601", range_="limited"):
    """the whole output buffer: `sentinel` everywhere but in the images"""
    out = np.full((dst_bytes,), sentinel, np.uint8)
    for (fmt, H, W, planes), row in zip(frames, rows):
        out[row[9]:row[9] + H * W * 3] = planes_to_rgb(fmt, H, W, planes, matrix, range_).reshape(-1)
    return out
