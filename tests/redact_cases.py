"""The inputs of the redaction tests (tests/test_redact_cpu.py, tests/test_redact_gpu.py): images in one flat buffer at
odd byte offsets and detection rows chosen to take every branch of the rule of include/codetr_redact.h."""
import numpy as np

SIZES = [(70, 131), (5, 7), (64, 128)]   # (H, W): two tiles each way with clipped edge cells; smaller than a cell; exact tiles
C = 4                                    # labels of the select table
SELECT = [1, 0, 1, 1]                    # label 1 is not redacted
THR = 0.25                               # exact in f16, bf16 and f32
GUARD = 64
Q = 16


def buffer(sizes, seed):
    """images of `sizes` in one flat buffer at odd byte offsets, random bytes between them and a guard region behind
    the last -> (uint8 numpy, rows [(offset, H, W)])"""
    rng = np.random.default_rng(seed)
    rows, offset = [], 1
    for i, (H, W) in enumerate(sizes):
        rows.append((offset, H, W))
        offset += H * W * 3 + (3, 5, 2)[i % 3]
    total = rows[-1][0] + sizes[-1][0] * sizes[-1][1] * 3 + GUARD
    return rng.integers(0, 256, total, dtype=np.uint8), rows


def mix(H, W):
    """Q = 16 rows of one H x W image, count 15 -> (boxes [Q, 4], scores [Q], labels [Q], count, names of the rows)"""
    nan, inf = float("nan"), float("inf")
    rows = [
        ("overlap_a", (W * 0.10, H * 0.15, W * 0.45, H * 0.60), 0.9, 0),
        ("overlap_b", (W * 0.30, H * 0.40, W * 0.62, H * 0.85), 0.8, 2),
        ("tile_corner", (58.5, 57.25, 70.5, 69.0), 0.7, 0),          # straddles (64, 64) where the image reaches it
        ("partly_outside", (-9.5, -4.0, W * 0.2, H * 0.3), 0.9, 3),
        ("wholly_outside", (W + 12.0, H + 8.0, W + 40.0, H + 30.0), 0.9, 0),
        ("zero_width", (W * 0.7, H * 0.1, W * 0.7, H * 0.5), 0.9, 0),
        ("nan_coordinate", (2.0, nan, W * 0.9, H * 0.9), 0.9, 0),
        ("inf_coordinate", (2.0, 2.0, inf, H * 0.9), 0.9, 0),
        ("score_at_thr", (0.0, 0.0, W, H), THR, 0),
        ("unselected_label", (0.0, 0.0, W, H), 0.9, 1),
        ("label_below", (0.0, 0.0, W, H), 0.9, -1),
        ("label_above", (0.0, 0.0, W, H), 0.9, C),
        ("nan_score", (0.0, 0.0, W, H), nan, 0),
        ("bottom_right", (W - 6.5, H - 4.25, W + 3.0, H + 9.0), 0.6, 2),
        ("small", (W * 0.8, H * 0.6, W * 0.8 + 2.5, H * 0.6 + 1.5), 0.5, 3),
        ("beyond_count", (0.0, 0.0, W, H), 0.9, 0),
    ]
    assert len(rows) == Q
    boxes = np.asarray([r[1] for r in rows], np.float32)
    scores = np.asarray([r[2] for r in rows], np.float32)
    labels = np.asarray([r[3] for r in rows], np.int64)
    return boxes, scores, labels, Q - 1, [r[0] for r in rows]


def batch(sizes=SIZES):
    """mix() of every image, stacked -> boxes [N, Q, 4], scores [N, Q], labels [N, Q], count [N]"""
    parts = [mix(H, W) for H, W in sizes]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
            np.asarray([p[3] for p in parts], np.int32))


def crowd(H, W, n, seed, thr=0.3):
    """n random overlapping boxes on an H x W image with scores around thr -> boxes [n, 4], scores [n], labels [n]"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, (W, H), (n, 2))
    wh = rng.uniform(1, (W / 3, H / 3), (n, 2))
    boxes = np.concatenate((c - wh / 2, c + wh / 2), 1).astype(np.float32)
    scores = rng.uniform(thr - 0.1, 1.0, n).astype(np.float32)
    return boxes, scores, rng.integers(0, C, n)
