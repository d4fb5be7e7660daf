"""The Inferencer's lens stage (hip_ops re-exports these names): the stored frames of a wide-angle or fisheye camera
remapped into the rectilinear images the models were trained on, behind the conversion / decoding and in front of everything
that reads the chunk's RGB buffer.  GPU-only, as hip_ops, but for `distort_points`; include/codetr_undistort.h states the
rule, csrc/undistort.hip holds the kernel.
"""
import numpy as np
import torch

from . import _cabi, _undistort
from . import _operands as _check

__all__ = ["UNDISTORT_MODELS", "UNDISTORT_DEFAULTS", "undistort_settings", "undistort_frames", "distort_points"]

UNDISTORT_MODELS = _undistort.MODELS   # "brown": OpenCV's rational model; "fisheye": cv::fisheye (Kannala-Brandt)
UNDISTORT_DEFAULTS = dict(model="brown", camera_matrix=None, dist_coeffs=(), new_camera_matrix=None, size=None, fill=(0, 0, 0))
_COEFFS = {"brown": (0, 4, 5, 8), "fisheye": (0, 4)}   # how many numbers dist_coeffs may hold


def _camera(v):
    """a 3 x 3 camera matrix without skew, or (fx, fy, cx, cy) -> (fx, fy, cx, cy) inside the header's admitted ranges"""
    what = (f"a 3 x 3 camera matrix without skew or (fx, fy, cx, cy): finite, focal lengths in (0, {_undistort.MAX_FOCAL}], "
            f"the principal point within +-{_undistort.MAX_CENTRE}")
    try:
        a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
    except (TypeError, ValueError):
        raise _check._Not(what) from None
    if a.shape == (3, 3):
        if a[0, 1] != 0 or a[1, 0] != 0 or a[2].tolist() != [0.0, 0.0, 1.0]:
            raise _check._Not(what)
        a = np.array([a[0, 0], a[1, 1], a[0, 2], a[1, 2]])
    if a.shape != (4,) or not np.isfinite(a).all() or not (0 < np.float32(a[:2])).all() or \
            (np.float32(a[:2]) > _undistort.MAX_FOCAL).any() or (np.abs(np.float32(a[2:])) > _undistort.MAX_CENTRE).any():
        raise _check._Not(what)
    return tuple(float(x) for x in a)


def _size(v):
    if v is None:
        return None
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise _check._Not(f"None or (H, W), each in 1..{_cabi.FRAME_MAX_SIDE}")
    side = _check.whole(1, _cabi.FRAME_MAX_SIDE)
    try:
        return (side(v[0]), side(v[1]))
    except _check._Not:
        raise _check._Not(f"None or (H, W), each in 1..{_cabi.FRAME_MAX_SIDE}") from None


def undistort_settings(undistort, H=None, W=None):
    """`undistort` of `Inferencer.__call__` (one image's dict) -> the completed dict plus what the kernel takes:
      model              a name of UNDISTORT_MODELS
      camera_matrix      required: the calibration of the camera that took the frame, 3 x 3 without skew or (fx, fy, cx, cy);
                         returned as (fx, fy, cx, cy)
      dist_coeffs        "brown": OpenCV's k1 k2 p1 p2 [k3 [k4 k5 k6]] -- 0, 4, 5 or 8 numbers; "fisheye": k1..k4 -- 0 or 4
      new_camera_matrix  the rectified image's camera; None: the camera's own
      size               (H', W') of the rectified image; None: the stored frame's (H, W), filled in when H and W are given
      fill               the RGB bytes of samples outside the stored frame
      code, params       the model's code and the sixteen parameters of include/codetr_undistort.h, each rounded to fp32
                         once (Python floats that hold fp32 values): what the kernel, the restatement and distort_points see
    ValueError for an unknown key or value, a missing camera_matrix, a skewed matrix, a non-finite number, a focal length
    <= 0 or a value outside the header's admitted ranges."""
    if not isinstance(undistort, dict):
        raise ValueError(f"undistort: a dict of {sorted(UNDISTORT_DEFAULTS)}, got {undistort!r}")
    given = dict(undistort)
    given.pop("code", None), given.pop("params", None)   # (a completed dict is taken again)
    if given.get("camera_matrix") is None:
        raise ValueError("undistort: camera_matrix is required (3 x 3, or (fx, fy, cx, cy))")
    s = _check.validated("undistort", UNDISTORT_DEFAULTS, given, dict(
        model=_check.one_of(tuple(UNDISTORT_MODELS)), camera_matrix=_camera, size=_size, fill=_check.colour,
        new_camera_matrix=lambda v: None if v is None else _camera(v)))
    try:
        k = np.float32(np.asarray(s["dist_coeffs"], dtype=np.float64).ravel()).tolist()
    except (TypeError, ValueError):
        k = None
    if k is None or len(k) not in _COEFFS[s["model"]] or not np.isfinite(k).all():
        raise ValueError(f"undistort dist_coeffs must be {' or '.join(map(str, _COEFFS[s['model']]))} finite numbers for "
                         f"model {s['model']!r}, got {s['dist_coeffs']!r}")
    s["dist_coeffs"] = tuple(k)
    if s["new_camera_matrix"] is None:
        s["new_camera_matrix"] = s["camera_matrix"]
    if s["size"] is None and H is not None:
        s["size"] = _size((H, W))
    s["code"] = UNDISTORT_MODELS[s["model"]]
    s["params"] = tuple(float(np.float32(x)) for x in s["camera_matrix"] + s["new_camera_matrix"]) + tuple(k) + (0.0,) * (8 - len(k))
    return s


def undistort_frames(src_u8, rows, settings, out=None):
    """Stored packed RGB frames -> the rectified images, one launch per PREPROCESS_BATCH_MAX images (csrc/undistort.hip).
      src_u8    one flat contiguous uint8 device buffer, only read
      rows      per image (H, W, offset, pitch): the stored size, the byte offset of the stored frame in src_u8 and its row
                pitch in bytes (>= 3 W)
      settings  `undistort_settings(...)` or what it takes: one dict for every image, or a list of one per image
      out       a flat uint8 buffer on src_u8's GPU, of at least the layout's bytes and not src_u8, to write into instead
                of a new one
    -> (the buffer, [(offset, H', W')] per image); images start at multiples of 16 bytes, as stage_chunk lays them out.
    ValueError for settings undistort_settings refuses and for a wrong dtype or shape; whatever else is inconsistent the
    entry point rejects before it launches."""
    _check._gpu(src_u8, "undistort_frames")
    _check.flat_u8("undistort_frames", src_u8)
    if not len(rows) or any(len(r) != 4 for r in rows):
        raise ValueError("undistort_frames: at least one row, four values each (H, W, offset, pitch)")
    rows = [tuple(int(v) for v in r) for r in rows]
    per_image = list(settings) if isinstance(settings, (list, tuple)) else [settings] * len(rows)
    if len(per_image) != len(rows):
        raise ValueError(f"undistort_frames: {len(per_image)} settings for {len(rows)} images")
    # (a completed dict with its size is taken as it is, as raw_to_rgb takes its settings: the entry point checks the values)
    per_image = [s if isinstance(s, dict) and "params" in s and s["size"] is not None else undistort_settings(s, r[0], r[1])
                 for s, r in zip(per_image, rows)]
    staged, table, total = [], [], 0
    for (H, W, off, pitch), s in zip(rows, per_image):
        Ho, Wo = s["size"]
        staged.append((total, Ho, Wo))
        r, g, b = s["fill"]
        table.append((s["code"], H, W, off, pitch, Ho, Wo, total, r << 16 | g << 8 | b))
        total = -(-(total + Ho * Wo * 3) // 16) * 16
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=src_u8.device)
    elif (not torch.is_tensor(out) or out.device != src_u8.device or out.dtype != torch.uint8 or out.dim() != 1
          or not out.is_contiguous() or out.numel() < total):
        raise ValueError(f"undistort_frames: out must be a contiguous flat uint8 buffer of at least {total} bytes on the "
                         "source's GPU")
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(len(rows)):
            _undistort.remap(src_u8, table[i:j], [s["params"] for s in per_image[i:j]], out)
    return out, staged


def distort_points(points, settings):
    """Points (x, y) of the rectified image -> the same points in the stored frame: steps 1-3 of the rule in real numbers
    (float64, the library's atan, no quantisation) on the settings' fp32 parameters.  For callers who must report boxes
    in sensor coordinates.  Host only.  points: [K, 2] array-like -> a new float64 array [K, 2]."""
    s = undistort_settings(settings)
    fx, fy, cx, cy, fxn, fyn, cxn, cyn = s["params"][:8]
    k = s["params"][8:]
    p = np.array(points, dtype=np.float64).reshape(-1, 2)
    x, y = (p[:, 0] - cxn) / fxn, (p[:, 1] - cyn) / fyn
    r2 = x * x + y * y
    if s["model"] == "fisheye":
        r = np.sqrt(r2)
        t = np.arctan(r)
        t2 = t * t
        td = t * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
        scale = np.where(r2 == 0, 1.0, td / np.where(r2 == 0, 1.0, r))
        xd, yd = x * scale, y * scale
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            kr = (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))) / (1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7])))
        xd = x * kr + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        yd = y * kr + 2 * k[3] * x * y + k[2] * (r2 + 2 * y * y)
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)
