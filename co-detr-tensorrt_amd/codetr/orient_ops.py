"""The Inferencer's orientation stage (hip_ops re-exports these names): the stored images of a chunk turned and mirrored
into the upright ones an EXIF orientation 1..8 asks for, behind the conversion / decoding and in front of everything that
reads the chunk's RGB buffer.  GPU-only, as hip_ops; include/codetr_orient.h states the rule, csrc/orient.hip holds the
kernel.
"""
import numpy as np
import torch

from . import _cabi, _orient
from . import _operands as _check

__all__ = ["ORIENTATIONS", "oriented_size", "jpeg_orientation", "orient_frames", "unorient_boxes"]

ORIENTATIONS = tuple(range(1, 9))   # EXIF's: 1 as stored, 2 mirrored, 3 half turn, 4 upside down, 5..8 rows become columns


def _orientation(name, o):
    if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or o not in ORIENTATIONS:
        raise ValueError(f"{name}: an orientation is an integer in 1..8 (EXIF's), got {o!r}")
    return int(o)


def oriented_size(o, H, W):
    """(H', W') of the upright image of a stored H x W one: 5..8 swap the sides"""
    return (int(W), int(H)) if _orientation("oriented_size", o) >= 5 else (int(H), int(W))


def jpeg_orientation(data) -> int:
    """the EXIF orientation 1..8 of a JPEG file (bytes, a 1-D uint8 array or host tensor, or a path), 1 when the file names
    none; host only (codetr_orient_exif: include/codetr_orient.h states which bytes are read)"""
    from .image_ops import jpeg_file_bytes

    return _orient.exif(jpeg_file_bytes(data))


def orient_frames(src_u8, rows, out=None):
    """Stored packed RGB images -> the upright ones, one launch per PREPROCESS_BATCH_MAX images (csrc/orient.hip).
      src_u8  one flat contiguous uint8 device buffer, only read
      rows    per image (o, H, W, offset, pitch): the orientation 1..8, the stored size, the byte offset of the stored image
              in src_u8 and its row pitch in bytes (>= 3 W)
      out     a flat uint8 buffer on src_u8's GPU, of at least the layout's bytes and not src_u8, to write into instead of
              a new one
    -> (the buffer, [(offset, H', W')] per image); images start at multiples of 16 bytes, as stage_chunk lays them out.
    An image with o = 1 is copied.  ValueError for an o outside 1..8 and for a wrong dtype or shape; whatever else is
    inconsistent the entry point rejects before it launches."""
    _check._gpu(src_u8, "orient_frames")
    _check.flat_u8("orient_frames", src_u8)
    if not len(rows) or any(len(r) != 5 for r in rows):
        raise ValueError("orient_frames: at least one row, five values each (o, H, W, offset, pitch)")
    rows = [(_orientation("orient_frames", r[0]),) + tuple(int(v) for v in r[1:]) for r in rows]
    staged, total = [], 0
    for o, H, W, _, _ in rows:
        staged.append((total,) + oriented_size(o, H, W))
        total = -(-(total + H * W * 3) // 16) * 16
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=src_u8.device)
    elif (not torch.is_tensor(out) or out.device != src_u8.device or out.dtype != torch.uint8 or out.dim() != 1
          or not out.is_contiguous() or out.numel() < total):
        raise ValueError(f"orient_frames: out must be a contiguous flat uint8 buffer of at least {total} bytes on the "
                         "source's GPU")
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(len(rows)):
            _orient.orient(src_u8, [r + (s[0],) for r, s in zip(rows[i:j], staged[i:j])], out)
    return out, staged


def unorient_boxes(bboxes, o, H, W):
    """xyxy boxes of the upright image -> the same regions in the coordinates of the stored H x W image, for tools that
    ignore the orientation tag.  Coordinates are pixel edges (a mirrored x is W - x, as the TTA un-flip has it), so a box
    that covers whole pixels maps to the box that covers the same pixels.  bboxes: [K, 4] array-like -> a new float array
    [K, 4] (float64 unless the input is a float array), corners ordered."""
    o = _orientation("unorient_boxes", o)
    b = np.asarray(bboxes)
    b = np.array(b, dtype=b.dtype if b.dtype.kind == "f" else np.float64).reshape(-1, 4)
    xa, ya, xb, yb = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    if o >= 5:          # the upright x runs along the stored y and the other way round
        xa, ya, xb, yb = ya, xa, yb, xb
    if o in (2, 3, 7, 8):   # the stored x runs against the upright axis it lies along
        xa, xb = W - xb, W - xa
    if o in (3, 4, 6, 7):
        ya, yb = H - yb, H - ya
    return np.stack([np.minimum(xa, xb), np.minimum(ya, yb), np.maximum(xa, xb), np.maximum(ya, yb)], axis=1)
