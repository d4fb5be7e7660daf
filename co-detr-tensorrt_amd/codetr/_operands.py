"""What the operator front ends (hip_ops, detection_ops, image_ops, track_ops) ask of their arguments, written once:
the GPU-only rule, the settings dicts (`validated` and its value checks), the flat image buffer with its (offset, H, W)
rows, a Detections-like operand, and the launch groups of PREPROCESS_BATCH_MAX rows.
"""
import math

import numpy as np
import torch

from . import _cabi

PREPROCESS_BATCH_MAX = _cabi.PREPROCESS_BATCH_MAX
FLOATS = (torch.float16, torch.bfloat16, torch.float32)
_WHOLE = (int, np.integer)
_REAL = (int, float, np.integer, np.floating)


def _gpu(x, what):
    if not x.is_cuda:
        raise RuntimeError(
            f"codetr.hip_ops.{what}: got a {x.device.type} tensor; this package computes on MI355X only "
            "(the CPU formulation is the oracle in oracle/, not a fallback)"
        )


class _Not(Exception):
    """a value check's refusal; its text completes "<key> must be ..." """


def number(lo=None, hi=None, finite=True, coerce=False):
    """check: a Python or numpy number, no bool and no NaN, finite unless told otherwise, inside [lo, hi] -> float.
    coerce: whatever else float() takes (a numeric string, a one-element array or tensor) counts as that number."""
    what = ("a finite number" if finite else "a number") + ("" if lo is None else f" in [{lo}, {hi}]")

    def check(v):
        if coerce and not isinstance(v, (bool,) + _REAL):
            try:
                v = float(v)
            except ValueError:
                raise _Not(what) from None
        if isinstance(v, bool) or not isinstance(v, _REAL) or v != v or (lo is not None and not lo <= v <= hi) or \
                (finite and not math.isfinite(v)):
            raise _Not(what)
        return float(v)
    return check


def whole(lo, hi, floats=False):
    """check: a Python or numpy integer (floats: or a float with a whole value), no bool, in lo..hi -> int"""
    def check(v):
        if isinstance(v, bool) or not isinstance(v, _REAL if floats else _WHOLE) or not lo <= v <= hi or int(v) != v:
            raise _Not(f"an integer in {lo}..{hi}")
        return int(v)
    return check


def one_of(choices):
    """check: one of these names (or of these integers, given as a Python or numpy integer) -> str (int)"""
    names = all(isinstance(c, str) for c in choices)

    def check(v):
        if isinstance(v, bool) or not isinstance(v, str if names else _WHOLE) or v not in choices:
            raise _Not(f"one of {list(choices)}")
        return str(v) if names else int(v)
    return check


def colour(v):
    """check: three whole values in 0..255 -> tuple of int"""
    if not isinstance(v, (tuple, list)) or len(v) != 3 or \
            any(not isinstance(c, _REAL) or not 0 <= c <= 255 or int(c) != c for c in v):
        raise _Not("three whole values in 0..255")
    return tuple(int(c) for c in v)


def validated(label, defaults, given, checks, sep=" "):
    """A settings dict: `defaults` completed from `given` (None: nothing given), every key of `checks` normalised by its
    check -> a new dict.  ValueError, led by `label`, for an unknown key and for a value its check refuses."""
    out = dict(defaults)
    given = dict(given or {})
    unknown = set(given) - set(out)
    if unknown:
        raise ValueError(f"{label}: unknown key(s) {sorted(unknown)}; known: {sorted(out)}")
    out.update(given)
    for key, check in checks.items():
        try:
            out[key] = check(out[key])
        except _Not as e:
            raise ValueError(f"{label}{sep}{key} must be {e}, got {out[key]!r}") from None
    return out


def chunks(N):
    """(i, j) of every launch group: PREPROCESS_BATCH_MAX rows, the last one shorter"""
    for i in range(0, N, PREPROCESS_BATCH_MAX):
        yield i, min(N, i + PREPROCESS_BATCH_MAX)


def flat_u8(name, buf):
    if not torch.is_tensor(buf) or not buf.is_cuda:
        raise ValueError(f"{name}: the image buffer must be a tensor on a GPU")
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError(f"{name}: expected one contiguous flat uint8 buffer")


def image_rows(name, buf, rows, max_side):
    """the flat uint8 device buffer of RGB HWC images and its (offset, H, W) rows -> the rows as tuples of int;
    ValueError for an image outside the buffer or with a side outside 1..max_side"""
    flat_u8(name, buf)
    rows = [tuple(int(v) for v in r) for r in rows]
    for off, H, W in rows:
        if not (1 <= H <= max_side and 1 <= W <= max_side) or off < 0 or off + H * W * 3 > buf.numel():
            raise ValueError(f"{name}: image (offset {off}, {H}x{W}) outside the buffer or larger than {max_side} a side")
    return rows


def same_gpu(name, device, **tensors):
    for key, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda or t.device != device:
            raise ValueError(f"{name}: {key} must be a tensor on the same GPU as the other operands")


def detections(name, dets, device, max_q, N=None):
    """a Detections-like operand on `device`: boxes [N,Q,4] and scores [N,Q] in one dtype of f16 / bf16 / f32, labels
    [N,Q] int64, count [N] int32, Q <= max_q (N given: that many rows) -> (N, Q)"""
    same_gpu(name, device, boxes=dets.boxes, scores=dets.scores, labels=dets.labels, count=dets.count)
    if dets.scores.dtype not in FLOATS or dets.boxes.dtype != dets.scores.dtype or dets.labels.dtype != torch.int64 or \
            dets.count.dtype != torch.int32:
        raise ValueError(f"{name}: boxes and scores in one dtype of f16 / bf16 / f32, labels int64, count int32")
    shape = tuple(dets.scores.shape)
    if len(shape) != 2 or N not in (None, shape[0]) or tuple(dets.boxes.shape) != shape + (4,) or \
            tuple(dets.labels.shape) != shape or tuple(dets.count.shape) != shape[:1]:
        raise ValueError(f"{name}: boxes [N,Q,4], scores [N,Q], labels [N,Q], count [N]" + (", N = len(rows)" if N is not None else ""))
    if shape[1] > max_q:
        raise ValueError(f"{name}: at most {max_q} detection rows per image, got {shape[1]}")
    return shape
