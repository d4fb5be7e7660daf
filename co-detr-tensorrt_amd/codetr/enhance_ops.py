"""The Inferencer's contrast stage (hip_ops re-exports these names): CLAHE -- contrast-limited adaptive histogram
equalisation -- of the luma of a chunk's packed RGB frames, the last stage in front of everything that reads the chunk's
RGB buffer.  GPU-only, as hip_ops; include/codetr_enhance.h states the rule in integers, csrc/enhance.hip holds the two
kernels.
"""
import math

import torch

from . import _enhance
from . import _operands as _check

__all__ = ["ENHANCE_MAX_GRID", "ENHANCE_DEFAULTS", "enhance_settings", "enhance_frames"]

ENHANCE_MAX_GRID = _enhance.MAX_GRID
ENHANCE_DEFAULTS = dict(grid=(8, 8), clip_limit=2.0)
_CLIP = _check.number(1 / 256, 256)


def _grid(v):
    side = _check.whole(1, ENHANCE_MAX_GRID)
    try:
        if not isinstance(v, (tuple, list)) or len(v) != 2:
            raise _check._Not("")
        return (side(v[0]), side(v[1]))
    except _check._Not:
        raise _check._Not(f"(gy, gx), each an integer in 1..{ENHANCE_MAX_GRID}") from None


def _clip_limit(v):
    try:
        return None if v is None else _CLIP(v)
    except _check._Not as e:
        raise _check._Not(f"None or {e}") from None


def enhance_settings(enhance, H=None, W=None):
    """`enhance` of `Inferencer.__call__` (one image's dict) -> the completed dict:
      grid        (gy, gx) tiles, each in 1..ENHANCE_MAX_GRID
      clip_limit  None: no clipping (plain adaptive equalisation; global equalisation with grid (1, 1)), or a number in
                  [1/256, 256]: a bin may hold at most clip_limit times the mean bin (OpenCV's meaning)
      clip_count  with H and W given: the rule's C for an H x W frame, max(1, (round(256 clip_limit) T) >> 16), T for None
    ValueError for an unknown key or value, and with H and W for a grid above a side or a tile above the header's 2^22 samples."""
    if not isinstance(enhance, dict):
        raise ValueError(f"enhance: a dict of {sorted(ENHANCE_DEFAULTS)}, got {enhance!r}")
    given = dict(enhance)
    given.pop("clip_count", None)   # (a completed dict is taken again)
    s = _check.validated("enhance", ENHANCE_DEFAULTS, given, dict(grid=_grid, clip_limit=_clip_limit))
    if H is not None:
        (gy, gx), H, W = s["grid"], int(H), int(W)
        if H < 1 or W < 1 or gy > H or gx > W:
            raise ValueError(f"enhance grid {s['grid']} has more tiles along a side than the {H} x {W} frame has pixels")
        T = -(-H // gy) * -(-W // gx)
        if T > _enhance.MAX_TILE:
            raise ValueError(f"enhance grid {s['grid']} gives tiles of {T} samples on a {H} x {W} frame; at most {_enhance.MAX_TILE}")
        s["clip_count"] = T if s["clip_limit"] is None else max(1, (math.floor(256 * s["clip_limit"] + 0.5) * T) >> 16)
    return s


def enhance_frames(src_u8, rows, settings, out=None, workspace=None):
    """Packed RGB frames -> the enhanced frames, two launches per PREPROCESS_BATCH_MAX images (csrc/enhance.hip).
      src_u8     one flat contiguous uint8 device buffer
      rows       per image (H, W, offset, pitch): the size, the byte offset of the frame in src_u8 and its row pitch in bytes
                 (>= 3 W)
      settings   what `enhance_settings` takes: one dict for every image, or a list of one per image
      out        None: a new buffer; a flat uint8 buffer on src_u8's GPU of at least the layout's bytes; or src_u8 itself:
                 in place, every pitch 3 W (a pixel's result depends on itself and the tables only)
      workspace  a dict the caller keeps between calls: device -> the scratch tensor of the kernels, grown when a call needs
                 more; None: allocated per call
    -> (the buffer, [(offset, H, W)] per image); out of place the images start at multiples of 16 bytes, as stage_chunk lays
    them out, in place where they are.  ValueError for settings enhance_settings refuses and for a wrong dtype or shape;
    whatever else is inconsistent the entry point rejects before it launches."""
    _check._gpu(src_u8, "enhance_frames")
    _check.flat_u8("enhance_frames", src_u8)
    if not len(rows) or any(len(r) != 4 for r in rows):
        raise ValueError("enhance_frames: at least one row, four values each (H, W, offset, pitch)")
    rows = [tuple(int(v) for v in r) for r in rows]
    per_image = list(settings) if isinstance(settings, (list, tuple)) else [settings] * len(rows)
    if len(per_image) != len(rows):
        raise ValueError(f"enhance_frames: {len(per_image)} settings for {len(rows)} images")
    per_image = [enhance_settings(s, r[0], r[1]) for s, r in zip(per_image, rows)]
    in_place = out is src_u8
    staged, table, total = [], [], 0
    for (H, W, off, pitch), s in zip(rows, per_image):
        if in_place and pitch != 3 * W:
            raise ValueError(f"enhance_frames: in place the frames are packed, got pitch {pitch} for width {W}")
        at, dpitch = (off, pitch) if in_place else (total, 3 * W)
        staged.append((at, H, W))
        table.append((H, W, off, pitch, at, dpitch) + s["grid"] + (s["clip_count"],))
        total = -(-(total + H * W * 3) // 16) * 16
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=src_u8.device)
    elif not in_place and (not torch.is_tensor(out) or out.device != src_u8.device or out.dtype != torch.uint8 or out.dim() != 1
                           or not out.is_contiguous() or out.numel() < total):
        raise ValueError(f"enhance_frames: out must be src_u8 itself or a contiguous flat uint8 buffer of at least {total} "
                         "bytes on the source's GPU")
    groups = [table[i:j] for i, j in _check.chunks(len(rows))]
    need = max(_enhance.workspace_bytes(g) for g in groups)
    cache = workspace if workspace is not None else {}
    ws = cache.get(src_u8.device)
    if ws is None or ws.numel() * 4 < need:
        ws = cache[src_u8.device] = torch.empty((need // 4,), dtype=torch.int32, device=src_u8.device)
    with torch.cuda.device(src_u8.device):
        for g in groups:   # (one stream: a group's apply pass has read the scratch before the next group's writes)
            _enhance.enhance(src_u8, g, out, ws)
    return out, staged
