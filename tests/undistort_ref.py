"""The rule of include/codetr_undistort.h restated in numpy, vectorised: fp32 with one rounding per operation (numpy's
float32 operations fuse nothing) for steps 1-3, integers for step 4; and the header's bound 1 with the real-number
position it is about, in float64.  `params` are the sixteen fp32 parameters of `hip_ops.undistort_settings(...)["params"]`."""
import numpy as np

F = np.float32
C = [F(float.fromhex(h)) for h in ("0x1p+0", "-0x1.5550f2p-2", "0x1.98d60ep-3", "-0x1.1e3d86p-3", "0x1.912bdep-4",
                                   "-0x1.d947a4p-5", "0x1.797cd6p-6", "-0x1.1d6f08p-8")]
DELTA = 2.0 ** -22   # the header's bound of |ATAN - atan|


def atan(r):
    """the header's ATAN on a float32 array r >= 0"""
    inv = r > F(1)
    z = np.where(inv, F(1) / np.where(inv, r, F(1)), r)
    w = z * z
    p = np.full_like(w, C[7])
    for c in C[6::-1]:
        p = c + w * p
    q = z * p
    return np.where(inv, F(float.fromhex("0x1.921fb6p+0")) - q, q)


def positions(params, model, Ho, Wo):
    """steps 1-3 for every output pixel -> (X, Y, valid): [Ho, Wo] int64 and bool"""
    fx, fy, cx, cy, fxn, fyn, cxn, cyn = (F(v) for v in params[:8])
    k = [F(v) for v in params[8:]]
    v, u = np.mgrid[0:Ho, 0:Wo]
    with np.errstate(all="ignore"):
        x, y = (u.astype(F) - cxn) / fxn, (v.astype(F) - cyn) / fyn
        xx, yy = x * x, y * y
        r2 = xx + yy
        if model == "fisheye":
            r = np.sqrt(r2)
            t = atan(r)
            t2 = t * t
            td = t * (F(1) + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
            s = np.where(r2 == 0, F(1), td / np.where(r2 == 0, F(1), r))
            xd, yd = x * s, y * s
        else:
            num = F(1) + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
            den = F(1) + r2 * (k[5] + r2 * (k[6] + r2 * k[7]))
            kr, xy = num / den, x * y
            xd = ((x * kr) + ((k[2] + k[2]) * xy)) + (k[3] * (r2 + (xx + xx)))
            yd = ((y * kr) + ((k[3] + k[3]) * xy)) + (k[2] * (r2 + (yy + yy)))
        fX, fY = np.floor((fx * xd + cx) * F(32) + F(0.5)), np.floor((fy * yd + cy) * F(32) + F(0.5))
        assert fX.dtype == F and r2.dtype == F
        valid = (fX >= -2 ** 20) & (fX <= 2 ** 20) & (fY >= -2 ** 20) & (fY <= 2 ** 20)   # (a NaN fails)
    return np.where(valid, fX, 0).astype(np.int64), np.where(valid, fY, 0).astype(np.int64), valid


def remap(image, settings, size=None):
    """a stored [H, W, 3] uint8 image under completed settings -> the rectified [H', W', 3] image"""
    H, W = image.shape[:2]
    Ho, Wo = size or settings["size"] or (H, W)
    X, Y, valid = positions(settings["params"], settings["model"], Ho, Wo)
    xi, yi, a, b = X >> 5, Y >> 5, (X & 31)[..., None], (Y & 31)[..., None]
    fill = np.array(settings["fill"], dtype=np.int64)

    def tap(y, x):
        inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        return np.where(inside[..., None], image[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), fill)

    out = ((32 - a) * (32 - b) * tap(yi, xi) + a * (32 - b) * tap(yi, xi + 1) + (32 - a) * b * tap(yi + 1, xi)
           + a * b * tap(yi + 1, xi + 1) + 512) >> 10
    return np.where(valid[..., None], out, fill).astype(np.uint8)


def real_and_bound(params, model, u, v):
    """float64: the real-number position (us, vs) of steps 1-3 and the header's E of bound 1 for X and for Y"""
    fx, fy, cx, cy, fxn, fyn, cxn, cyn = params[:8]
    k = np.abs(params[8:]), params[8:]
    e, G = 2.0 ** -24, 1 + 2.0 ** -8
    x, y = (np.asarray(u, np.float64) - cxn) / fxn, (np.asarray(v, np.float64) - cyn) / fyn
    r2 = x * x + y * y
    if model == "fisheye":
        r = np.sqrt(r2)
        t = np.arctan(r)
        Sp, P = (1 + t * t * (c[0] + t * t * (c[1] + t * t * (c[2] + t * t * c[3]))) for c in k)
        Dt, td = DELTA + 4 * e * t, t * P
        Etd = np.abs(P) * Dt + Sp * (12 * e * t + 8 * Dt) + e * np.abs(td)
        s = np.where(r2 == 0, 1.0, td / np.where(r2 == 0, 1.0, r))
        xd, yd = x * s, y * s
        Ex, Ey = fx * (Etd + 9 * e * np.abs(xd)), fy * (Etd + 9 * e * np.abs(yd))
    else:
        (Sn, Sd), (num, den) = ((1 + r2 * (c[0] + r2 * (c[1] + r2 * c[4])), 1 + r2 * (c[5] + r2 * (c[6] + r2 * c[7]))) for c in k)
        kr, (p1, p2) = num / den, params[10:12]
        Ek = e * (24 * Sn / np.abs(den) + 24 * Sd * np.abs(kr) / np.abs(den) + np.abs(kr))
        tx = x * kr, 2 * p1 * x * y, p2 * (r2 + 2 * x * x)
        ty = y * kr, 2 * p2 * x * y, p1 * (r2 + 2 * y * y)
        xd, yd = sum(tx), sum(ty)
        Ex = fx * (np.abs(x) * Ek + 11 * e * sum(np.abs(t) for t in tx))
        Ey = fy * (np.abs(y) * Ek + 11 * e * sum(np.abs(t) for t in ty))
    us, vs = fx * xd + cx, fy * yd + cy
    return us, vs, G * (Ex + e * (2 * np.abs(us) + 1)), G * (Ey + e * (2 * np.abs(vs) + 1))
