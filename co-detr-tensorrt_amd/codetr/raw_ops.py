"""The Inferencer's raw Bayer stage (hip_ops re-exports these names): the colour-filter mosaic an industrial, automotive or
embedded camera delivers -- one sample per pixel, 8 to 16 bits -- normalised, demosaiced and toned into the packed RGB images
every other kernel reads.  GPU-only, as hip_ops; include/codetr_raw.h states the rule, csrc/raw.hip holds the kernel.
"""
import numpy as np
import torch

from . import _raw
from . import _operands as _check

__all__ = ["RAW_FORMATS", "RAW_METHODS", "RAW_DEFAULTS", "raw_settings", "raw_to_rgb"]

RAW_FORMATS = _raw.FORMATS    # name -> code: the colours of the pixels (0,0), (0,1), (1,0), (1,1)
RAW_METHODS = _raw.METHODS    # "malvar": Malvar-He-Cutler 5 x 5; "bilinear": the 3 x 3 averages
RAW_DEFAULTS = dict(bits=8, black_level=0, white_level=None, white_balance=(1.0, 1.0, 1.0), method="malvar", tone="linear")

_LUTS = {}   # (device, the table's bytes) -> the table on that device: uploaded once per distinct table


def _gains(v):
    if not isinstance(v, (tuple, list)) or len(v) != 3:
        raise _check._Not("three finite numbers >= 0 (red, green, blue)")
    try:
        return tuple(_check.number(0.0, float("inf"), finite=True)(g) for g in v)
    except _check._Not:
        raise _check._Not("three finite numbers >= 0 (red, green, blue)") from None


def _tone(v):
    """the 4096-entry table of the rule's step 4, built in float64 and rounded once"""
    x = np.arange(4096, dtype=np.float64) / 4095.0
    if isinstance(v, str):
        if v == "linear":
            return ((np.arange(4096, dtype=np.int64) * 255 + 2047) // 4095).astype(np.uint8)
        if v == "srgb":
            y = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
            return np.floor(255.0 * y + 0.5).astype(np.uint8)
    elif isinstance(v, _check._REAL) and not isinstance(v, bool):
        if v == v and 0.0 < v < float("inf"):
            return np.floor(255.0 * np.power(x, 1.0 / float(v)) + 0.5).astype(np.uint8)
    else:
        a = v.detach().cpu().numpy() if torch.is_tensor(v) else v
        if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (4096,):
            return np.ascontiguousarray(a)
    raise _check._Not('"linear", "srgb", a gamma > 0 (out = in ** (1 / gamma)) or a uint8 array of 4096 entries')


def raw_settings(raw=None):
    """`raw` of `Inferencer.__call__` (None: RAW_DEFAULTS) -> the completed dict plus what the kernel takes:
      bits           8 (uint8 frames) or 9..16 (uint16 frames, the sample in the low `bits` bits)
      black_level    subtracted from every sample; white_level: the sample that maps to full scale, None = 2**bits - 1
      white_balance  gains (red, green, blue), applied to the mosaic before interpolation
      method         a name of RAW_METHODS; tone: "linear", "srgb", a gamma, or a 4096-entry uint8 table indexed by the top
                     12 bits of the 16-bit result
      operands       (method code, black, white, m_red, m_green, m_blue) of include/codetr_raw.h, step 1
      lut            the table as a numpy array
    ValueError for an unknown key or value, white_level <= black_level or above 2**bits - 1, and gains whose multiplier
    gain * 65535 * 65536 / (white - black) reaches 2**32."""
    given = dict(raw or {})
    given.pop("operands", None), given.pop("lut", None)   # (a completed dict is taken again)
    s = _check.validated("raw", RAW_DEFAULTS, given, dict(
        bits=_check.whole(8, 16), black_level=_check.whole(0, 65535), white_balance=_gains,
        white_level=lambda v: None if v is None else _check.whole(0, 65535)(v),
        method=_check.one_of(tuple(RAW_METHODS)), tone=lambda v: (_tone(v), v)[1]))
    lut, top = _tone(s["tone"]), 2 ** s["bits"] - 1
    if s["white_level"] is None:
        s["white_level"] = top
    if not s["black_level"] < s["white_level"] <= top:
        raise ValueError(f"raw: need black_level < white_level <= {top} for bits={s['bits']}, got {s['black_level']} and "
                         f"{s['white_level']}")
    m = _raw.multipliers(s["black_level"], s["white_level"], s["white_balance"])
    if m is None:
        raise ValueError(f"raw white_balance {s['white_balance']}: gain * 65535 * 65536 / (white_level - black_level) must "
                         "stay below 2**32")
    s["operands"] = (RAW_METHODS[s["method"]], s["black_level"], s["white_level"]) + m
    s["lut"] = lut
    return s


def _device_lut(lut, device):
    key = (str(device), lut.tobytes())
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(lut).to(device)
    return _LUTS[key]


def raw_to_rgb(src_u8, rows, dst_bytes, settings=None, out=None):
    """Raw Bayer frames -> packed RGB HWC images in one flat uint8 device buffer of `dst_bytes` bytes, one launch per
    PREPROCESS_BATCH_MAX frames (csrc/raw.hip; include/codetr_raw.h states the rule).
      src_u8    one flat contiguous uint8 device buffer that holds every frame, only read
      rows      per frame (pattern, bits, H, W, src_offset, pitch_bytes, dst_offset): a name of RAW_FORMATS or its code, the
                settings' bits, the offset of sample (0, 0) and the row pitch in bytes (16-bit frames: both even)
      settings  `raw_settings(...)` or what it takes
      out       a flat uint8 buffer of dst_bytes on src_u8's GPU to write into instead of a new one
    -> the buffer; bytes outside the images are not written.  ValueError for an unknown pattern, bits that are not the
    settings', an odd offset or pitch of a 16-bit frame and a wrong dtype or shape; whatever else is inconsistent the
    entry point rejects before it launches."""
    _check._gpu(src_u8, "raw_to_rgb")
    _check.flat_u8("raw_to_rgb", src_u8)
    if settings is None or "operands" not in settings:
        settings = raw_settings(settings)
    checked = []
    for r in rows:
        if len(r) != 7:
            raise ValueError("raw_to_rgb: seven values per row (pattern, bits, H, W, src_offset, pitch_bytes, dst_offset)")
        code = RAW_FORMATS.get(r[0]) if isinstance(r[0], str) else r[0]
        if code is None or isinstance(code, bool) or int(code) not in RAW_FORMATS.values():
            raise ValueError(f"raw_to_rgb: unknown pattern {r[0]!r}; known: {sorted(RAW_FORMATS)}")
        row = (int(code),) + tuple(int(v) for v in r[1:])
        if row[1] != settings["bits"]:
            raise ValueError(f"raw_to_rgb: a row of bits={row[1]} under settings of bits={settings['bits']}")
        if row[1] > 8 and ((src_u8.data_ptr() + row[4]) % 2 or row[5] % 2):
            raise ValueError(f"raw_to_rgb: a 16-bit frame needs an even byte offset and an even pitch, got offset {row[4]} "
                             f"(buffer at {src_u8.data_ptr() % 2} mod 2) and pitch {row[5]}")
        checked.append(row)
    if not checked or int(dst_bytes) <= 0:
        raise ValueError("raw_to_rgb: no frames")
    if out is None:
        out = torch.empty((int(dst_bytes),), dtype=torch.uint8, device=src_u8.device)
    elif (not torch.is_tensor(out) or out.device != src_u8.device or out.dtype != torch.uint8 or out.dim() != 1
          or not out.is_contiguous() or out.numel() != int(dst_bytes)):
        raise ValueError("raw_to_rgb: out must be a contiguous flat uint8 buffer of dst_bytes on the source's GPU")
    lut = _device_lut(settings["lut"], src_u8.device)
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(len(checked)):
            _raw.to_rgb(src_u8, checked[i:j], settings["operands"], lut, out)
    return out
