"""The Inferencer's operators on image buffers (hip_ops re-exports them): pre-processing of uploaded images into the model's
batch, drawing and redaction on them, the JPEG encoder and decoder, and the conversion of decoder frames to RGB.  GPU-only,
as hip_ops; the flat uint8 buffer and its (offset, H, W) rows are checked in _operands.
"""
import os

import numpy as np
import torch

from . import _cabi, _jpeg, _jpeg_dec, _redact
from . import _operands as _check
from . import orient_ops as _orient_ops
from ._operands import _gpu

# the public names (hip_ops re-exports exactly these)
__all__ = [
    "preprocess_image", "PREPROCESS_BATCH_MAX", "preprocess_batch", "preprocess_views", "preprocess_tiles",
    "DRAW_MAX_Q", "DRAW_MAX_SIDE", "DRAW_NAME_ROW", "DRAW_STYLE", "draw_style", "draw_names_table",
    "draw_detections", "REDACT", "REDACT_MODES", "REDACT_SHAPES", "REDACT_CELLS", "redact_style",
    "redact_detections", "JPEG_SETTINGS", "JPEG_DOWNLOADS", "jpeg_settings", "jpeg_out_stride", "encode_jpeg",
    "JPEG_DECODE_STATS", "jpeg_file_bytes", "jpeg_parse", "jpeg_host_decode", "jpeg_reason", "jpeg_info",
    "jpeg_stage", "jpeg_decode_staged", "jpeg_status_error", "decode_jpeg", "FRAME_FORMATS", "FRAME_COLOR",
    "frames_to_rgb",
]


def preprocess_image(src_u8, resized_hw, pad_hw, mean, std, pad_value=(0, 0, 0), dtype=torch.float16):
    """uint8 HWC RGB image on the GPU -> (normalised [3, Hp, Wp], mask [Hp, Wp]): cv2-exact bilinear resize to
    `resized_hw`, right / bottom padding with `pad_value` to `pad_hw`, (x - mean) / std (csrc/prepost.hip)."""
    _gpu(src_u8, "preprocess_image")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 3 or src_u8.shape[2] != 3:
        raise ValueError("expected a uint8 [H, W, 3] image")
    with torch.cuda.device(src_u8.device):
        return _cabi.preprocess_u8(src_u8.contiguous(), resized_hw, pad_hw, mean, std, pad_value, dtype)


PREPROCESS_BATCH_MAX = _check.PREPROCESS_BATCH_MAX


def _preprocess_rows(name, launch, src_u8, rows, batch_hw, mean, std, pad_val, pad_value, dtype, with_mask):
    """the body of preprocess_batch and preprocess_views: one `launch` per PREPROCESS_BATCH_MAX rows into one batch"""
    _gpu(src_u8, name)
    _check.flat_u8(name, src_u8)
    if dtype not in _check.FLOATS:
        raise ValueError(f"{name} writes f16, bf16 or f32, not {dtype}")
    N = len(rows)
    H, W = (int(v) for v in batch_hw)
    x = torch.empty((N, 3, H, W), dtype=dtype, device=src_u8.device)
    m = torch.empty((N, H, W), dtype=dtype, device=src_u8.device) if with_mask else None
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(N):
            launch(src_u8, rows[i:j], (H, W), mean, std, pad_val, pad_value, x[i:j], m[i:j] if m is not None else None)
    return x, m


def preprocess_batch(src_u8, images, batch_hw, mean, std, pad_val=(0, 0, 0), pad_value=0.0, dtype=torch.float16,
                     with_mask=True):
    """Many uint8 HWC RGB images of different sizes, back to back in ONE flat device buffer -> the stacked
    (batch_inputs [N, 3, H, W], img_masks [N, H, W] or None), batch_hw = (H, W).  images: one row per image,
    (src_offset, H_src, W_src, H_resized, W_resized, H_pad, W_pad).  Per image preprocess_image's arithmetic into its
    (H_pad, W_pad) Pad region; beyond it `pad_value` as is and mask 1 (DetDataPreprocessor's divisor padding and
    stack_batch).  One launch per PREPROCESS_BATCH_MAX images (csrc/prepost.hip)."""
    return _preprocess_rows("preprocess_batch", _cabi.preprocess_batch_u8, src_u8, images, batch_hw, mean, std, pad_val,
                            pad_value, dtype, with_mask)


def preprocess_views(src_u8, rows8, batch_hw, mean, std, pad_val=(0, 0, 0), pad_value=0.0, dtype=torch.float16,
                     with_mask=True):
    """preprocess_batch for test-time augmentation's views: rows8 has one row per VIEW, (src_offset, H_src, W_src,
    H_resized, W_resized, H_pad, W_pad, flip).  flip = 1 writes the resized image mirrored left to right inside its
    resized width (mmdet flips after Resize and before any padding: the padding stays on the right, the mask does not
    change); rows may share a src_offset, so the views of an image read its one uploaded copy.  -> (batch_inputs
    [N, 3, H, W], img_masks [N, H, W] or None), N = len(rows8); one launch per PREPROCESS_BATCH_MAX rows."""
    if any(len(r) != 8 for r in rows8):
        raise ValueError("preprocess_views: eight values per row, the last one the flip (0 or 1)")
    return _preprocess_rows("preprocess_views", _cabi.preprocess_views_u8, src_u8, rows8, batch_hw, mean, std, pad_val,
                            pad_value, dtype, with_mask)


def preprocess_tiles(src_u8, rows11, batch_hw, mean, std, pad_val=(0, 0, 0), pad_value=0.0, dtype=torch.float16,
                     with_mask=True):
    """preprocess_batch for sliced inference's tiles: rows11 has one row per TILE, (src_offset, H_img, W_img, y0, x0,
    H_crop, W_crop, H_resized, W_resized, H_pad, W_pad).  A row is, bit for bit, what preprocess_batch writes for a
    contiguous copy of the H_crop x W_crop window at (y0, x0) of its image: the tile is resized as an image of its own
    and never reads a pixel outside the crop.  Rows may share a src_offset, so the tiles of an image read its one
    uploaded copy.  -> (batch_inputs [N, 3, H, W], img_masks [N, H, W] or None), N = len(rows11); one launch per
    PREPROCESS_BATCH_MAX rows."""
    if any(len(r) != 11 for r in rows11):
        raise ValueError("preprocess_tiles: eleven values per row (src_offset, H_img, W_img, y0, x0, H_crop, W_crop, "
                         "H_resized, W_resized, H_pad, W_pad)")
    return _preprocess_rows("preprocess_tiles", _cabi.preprocess_tiles_u8, src_u8, rows11, batch_hw, mean, std, pad_val,
                            pad_value, dtype, with_mask)


DRAW_MAX_Q = _cabi.DRAW_MAX_Q
DRAW_MAX_SIDE = _cabi.DRAW_MAX_SIDE
DRAW_NAME_ROW = 24    # bytes per row of the names table: the length, then up to 23 characters
# the defaults of mmdet's DetLocalVisualizer (line_width, alpha, text_color) and of the Inferencer's pred_score_thr
DRAW_STYLE = dict(line_width=3, alpha=0.8, score_thr=0.3, text_color=(200, 200, 200), font_scale=1, draw_labels=True)


def draw_style(style=None):
    """the style of draw_detections, validated: the keys of DRAW_STYLE (missing ones take its values) -> a new dict.
    ValueError for an unknown key, line_width outside 1..15, alpha outside [0, 1], font_scale outside 1..4, a
    text_color that is not three values in 0..255, a score_thr that is not a number."""
    return _check.validated("draw style", DRAW_STYLE, style, dict(
        line_width=_check.whole(1, 15, floats=True), font_scale=_check.whole(1, 4, floats=True), alpha=_check.number(0, 1),
        score_thr=_check.number(finite=False), text_color=_check.colour, draw_labels=bool), sep=": ")


def draw_names_table(classes):
    """class names -> the [C, 24] uint8 table draw_detections reads (a CPU tensor): byte 0 of a row is the length, the
    name truncated to 23 characters; a character outside ASCII 32..126 becomes '?'"""
    rows = []
    for name in classes:
        text = "".join(ch if 32 <= ord(ch) <= 126 else "?" for ch in str(name))[:DRAW_NAME_ROW - 1]
        rows.append(bytes([len(text)]) + text.encode("ascii") + bytes(DRAW_NAME_ROW - 1 - len(text)))
    return torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).view(len(rows), DRAW_NAME_ROW)


def draw_detections(buf_u8, rows, dets, names, palette, style=None):
    """The Inferencer's visualisation in one launch per PREPROCESS_BATCH_MAX images (csrc/draw.hip; the rendering is
    stated in include/codetr_hip.h): per detection with a score above style['score_thr'] a box outline in its class
    colour and, after all outlines, "<name>: <percent>" on a darkened patch at the box's top-left corner.  In place.
      buf_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows      (offset, H, W) per image
      dets      Detections / SoftDetections over [N, Q] rows, N = len(rows), Q <= 4096, boxes in image coordinates
      names     [C, 24] uint8 on the device (draw_names_table); palette [C, 3] uint8 on the device
      style     the keys of DRAW_STYLE
    -> buf_u8.  ValueError for Q > 4096, a bad style value, a wrong dtype or shape, CPU tensors.  Nothing is launched
    when N == 0 or Q == 0."""
    st = draw_style(style)
    rows = _check.image_rows("draw_detections", buf_u8, rows, DRAW_MAX_SIDE)
    _check.same_gpu("draw_detections", buf_u8.device, names=names, palette=palette)
    C = palette.shape[0] if palette.dim() == 2 else 0
    if names.dtype != torch.uint8 or palette.dtype != torch.uint8 or C == 0 or tuple(palette.shape) != (C, 3) or \
            tuple(names.shape) != (C, DRAW_NAME_ROW):
        raise ValueError("draw_detections: names [C, 24] and palette [C, 3] in uint8, C > 0")
    N, Q = _check.detections("draw_detections", dets, buf_u8.device, DRAW_MAX_Q, len(rows))
    if N == 0 or Q == 0:
        return buf_u8
    boxes, scores, labels, count = (t.contiguous() for t in (dets.boxes, dets.scores, dets.labels, dets.count))
    tc = st["text_color"]
    with torch.cuda.device(buf_u8.device):
        for i, j in _check.chunks(N):
            _cabi.draw_detections(buf_u8, rows[i:j], boxes[i:j], scores[i:j], labels[i:j], count[i:j],
                                  palette.contiguous(), names.contiguous(), st["line_width"], st["alpha"], st["score_thr"],
                                  (tc[0] << 16) | (tc[1] << 8) | tc[2], st["font_scale"], st["draw_labels"])
    return buf_u8


# redaction of detected regions (include/codetr_redact.h states the rule and its limits).  "blur" is the library's own: a
# box filter over fixed cells and a tent reconstruction; parity with OpenCV's blur is unpinned (cv2 is not installed here)
REDACT = dict(mode="pixelate", score_thr=0.3, expand=0.1, shape="box", cell=16, fill=(0, 0, 0))
REDACT_MODES = tuple(_redact.MODES)
REDACT_SHAPES = tuple(_redact.SHAPES)
REDACT_CELLS = _redact.CELLS
_redact_work = {}   # device -> the "blur" workspace on it (uint8), grown when a call needs more


def redact_style(settings=None):
    """the settings of redact_detections, validated and completed from REDACT -> a new dict.  ValueError, naming the key,
    for an unknown key, a mode outside REDACT_MODES, a shape outside REDACT_SHAPES, a cell outside REDACT_CELLS, an expand
    outside [0, 1], a score_thr that is not a number, a fill that is not three whole values in 0..255."""
    return _check.validated("redact", REDACT, settings, dict(
        mode=_check.one_of(REDACT_MODES), shape=_check.one_of(REDACT_SHAPES), cell=_check.one_of(REDACT_CELLS),
        score_thr=_check.number(finite=False), expand=_check.number(0, 1), fill=_check.colour), sep=": ")


def redact_detections(buf_u8, rows, dets, settings=None, select=None):
    """Redaction of the detected regions in one launch per PREPROCESS_BATCH_MAX images ("blur": two) and without a
    synchronisation (csrc/redact.hip; include/codetr_redact.h states the rule): the pixels under every detection with a
    score above settings['score_thr'] and a selected label -- its box grown by settings['expand'], or the ellipse inside
    it -- become the mean of their cell ("pixelate"), the tent interpolation of the cell means ("blur") or
    settings['fill'].  In place; an unmasked pixel is never written.
      buf_u8    one flat uint8 device buffer holding RGB HWC images (Inferencer.upload's)
      rows      (offset, H, W) per image
      dets      Detections / SoftDetections over [N, Q] rows, N = len(rows), Q <= 4096, boxes in image coordinates
      settings  the keys of REDACT
      select    [C] uint8 on the device, 1 = redact this label (any other label is left); None = every label
    -> buf_u8.  ValueError for Q > 4096, a bad setting, a wrong dtype or shape, CPU tensors.  Nothing is launched when
    N == 0 or Q == 0.  "blur" keeps one workspace per device and grows it."""
    st = redact_style(settings)
    rows = _check.image_rows("redact_detections", buf_u8, rows, DRAW_MAX_SIDE)
    if select is not None:
        _check.same_gpu("redact_detections", buf_u8.device, select=select)
        if select.dtype != torch.uint8 or select.dim() != 1 or select.numel() == 0:
            raise ValueError("redact_detections: select must be a [C] uint8 table, C > 0")
    N, Q = _check.detections("redact_detections", dets, buf_u8.device, DRAW_MAX_Q, len(rows))
    if N == 0 or Q == 0:
        return buf_u8
    boxes, scores, labels, count = (t.contiguous() for t in (dets.boxes, dets.scores, dets.labels, dets.count))
    select = None if select is None else select.contiguous()
    fill = st["fill"]
    with torch.cuda.device(buf_u8.device):
        for i, j in _check.chunks(N):
            work = None
            if st["mode"] == "blur":   # (launches on one stream run in order: the next group may reuse the workspace)
                need, key = _redact.work_bytes(rows[i:j], st["cell"]), str(buf_u8.device)
                work = _redact_work.get(key)
                if work is None or work.numel() < need:
                    work = _redact_work[key] = torch.empty((need,), dtype=torch.uint8, device=buf_u8.device)
            _redact.redact_detections(buf_u8, rows[i:j], boxes[i:j], scores[i:j], labels[i:j], count[i:j], select,
                                      _redact.MODES[st["mode"]], _redact.SHAPES[st["shape"]], st["cell"], st["score_thr"],
                                      st["expand"], (fill[0] << 16) | (fill[1] << 8) | fill[2], work)
    return buf_u8


JPEG_SETTINGS = dict(quality=90, subsampling="420")
JPEG_DOWNLOADS = {"copies": 0, "bytes": 0}   # device-to-host copies encode_jpeg made in this process


def jpeg_settings(settings=None):
    """quality / subsampling of encode_jpeg, validated: the keys of JPEG_SETTINGS (missing ones take its values) -> a new
    dict.  ValueError for an unknown key, a quality that is not an integer in 1..100, a subsampling other than '420' /
    '444'."""
    return _check.validated("jpeg", JPEG_SETTINGS, settings, dict(
        quality=_check.whole(1, 100, floats=True), subsampling=_check.one_of(_jpeg.SUBSAMPLINGS)), sep=": ")


def jpeg_out_stride(rows, subsampling="420"):
    """the bytes encode_jpeg reserves per image of a launch group on its first attempt: an eighth of the largest raw image
    plus 4 KB, never more than the proven bound of the largest scan, rounded up to 16.  (A drawn 1080p frame at quality
    90 / 4:2:0 takes about a twentieth of its raw size; noise at quality 100 exceeds the raw size and takes the retry.)"""
    sub = _jpeg.SUBSAMPLINGS[subsampling]
    guess = max(H * W * 3 for _, H, W in rows) // 8 + 4096
    bound = max(_jpeg.scan_bound(H, W, sub) for _, H, W in rows)
    return (min(guess, bound) + 15) // 16 * 16


def encode_jpeg(src, rows, quality=90, subsampling="420", out_stride=None):
    """RGB images on the device -> complete baseline JPEG files, encoded on the GPU (csrc/jpeg.hip; the file is stated in
    include/codetr_jpeg.h): the scan comes from two launches per PREPROCESS_BATCH_MAX images, the header from the
    library's host builder.
      src       one flat uint8 device buffer holding RGB HWC images (the buffer draw_detections drew on)
      rows      (offset, H, W) per image
      quality   1..100 (the IJG scale); subsampling '420' | '444'
      out_stride  bytes reserved per image on the first attempt (default: jpeg_out_stride).  An image whose scan does not
                fit is encoded once more with the proven worst case reserved, in one launch group with the others that
                did not fit.
    -> list[bytes], one file per row.  One device-to-host copy per launch group: the int32 lengths and the slots travel
    in one buffer.  ValueError for a bad setting, a wrong dtype or shape, a CPU tensor, an image outside the buffer."""
    st = jpeg_settings(dict(quality=quality, subsampling=subsampling))
    rows = _check.image_rows("encode_jpeg", src, rows, DRAW_MAX_SIDE)
    if out_stride is not None and (int(out_stride) != out_stride or out_stride < 1):
        raise ValueError(f"encode_jpeg: out_stride must be a positive integer, got {out_stride!r}")
    sub = _jpeg.SUBSAMPLINGS[st["subsampling"]]
    scans = [None] * len(rows)

    def group(index, stride):
        """one launch group: encode rows[index] into slots of `stride` bytes -> the indices that did not fit"""
        part = [rows[i] for i in index]
        head = (4 * len(part) + 15) // 16 * 16   # the lengths lead the buffer, so that one copy brings both
        out = torch.empty((head + len(part) * stride,), dtype=torch.uint8, device=src.device)
        ws = torch.empty((_jpeg.workspace_bytes(part, sub, stride),), dtype=torch.uint8, device=src.device)
        _jpeg.encode(src, part, st["quality"], sub, out[head:], stride, out[:head].view(torch.int32), ws)
        host = out.cpu().numpy()
        JPEG_DOWNLOADS["copies"] += 1
        JPEG_DOWNLOADS["bytes"] += host.size
        lengths = host[:head].view(np.int32)
        missed = []
        for k, i in enumerate(index):
            if lengths[k] < 0:
                missed.append(i)
            else:
                scans[i] = host[head + k * stride:head + k * stride + int(lengths[k])].tobytes()
        return missed

    with torch.cuda.device(src.device):
        retry = []
        for i, j in _check.chunks(len(rows)):
            index = list(range(i, j))
            stride = int(out_stride) if out_stride is not None else jpeg_out_stride([rows[k] for k in index], st["subsampling"])
            retry += group(index, stride)
        for i, j in _check.chunks(len(retry)):
            index = retry[i:j]
            bound = max(_jpeg.scan_bound(rows[k][1], rows[k][2], sub) for k in index)
            if group(index, (bound + 15) // 16 * 16):
                raise RuntimeError("encode_jpeg: a scan exceeded its proven bound")
    return [_jpeg.header(H, W, st["quality"], sub) + scans[i] + b"\xff\xd9" for i, (_, H, W) in enumerate(rows)]


JPEG_DECODE_STATS = {"host_fallbacks": 0}   # files the GPU decoder does not support, decoded with Pillow on the host


def jpeg_file_bytes(item):
    """one JPEG file as a contiguous 1-D uint8 numpy array: bytes / bytearray / memoryview, a 1-D uint8 numpy array or
    host tensor, or a str / os.PathLike path"""
    if isinstance(item, (str, os.PathLike)):
        with open(item, "rb") as f:
            item = f.read()
    if isinstance(item, (bytes, bytearray, memoryview)):
        return np.frombuffer(item, np.uint8)
    if torch.is_tensor(item) and not item.is_cuda:
        item = item.detach().numpy()
    if isinstance(item, np.ndarray) and item.dtype == np.uint8 and item.ndim == 1:
        return np.ascontiguousarray(item)
    raise ValueError(f"jpeg: a file is bytes, a 1-D uint8 array or host tensor, or a path; got {type(item).__name__}")


def jpeg_parse(data):
    """the header of one file (a contiguous 1-D uint8 numpy array) -> (return code, info, tables) of
    codetr_jpegdec_parse; host only"""
    return _jpeg_dec.parse(data)


def jpeg_host_decode(data):
    """the file decoded on the host with Pillow -> RGB uint8 [H, W, 3], counted in JPEG_DECODE_STATS; None when Pillow
    does not import"""
    try:
        import io

        from PIL import Image
    except ImportError:
        return None
    rgb = np.asarray(Image.open(io.BytesIO(data.tobytes())).convert("RGB"))
    JPEG_DECODE_STATS["host_fallbacks"] += 1
    return rgb


def jpeg_reason(rc, info):
    if rc == 0:
        return None
    if rc == _cabi._D["CODETR_E_UNSUPPORTED"]:
        return _jpeg_dec.REASONS.get(int(info[6]), "unsupported")
    return "too_large" if rc == _cabi._D["CODETR_E_TOO_LARGE"] else "bad_header"


def jpeg_info(data):
    """What the header of a JPEG file says (host only; include/codetr_jpeg_dec.h's parser)
    -> dict(supported, reason, height, width, components, sampling [(h, v)], restart_interval, scan_offset, scan_bytes);
    reason: None, a name of the header's CODETR_JPEGDEC_R_* in lower case, 'too_large' or 'bad_header'; size and sampling
    are those of the frame header when it was read, else 0 / []."""
    rc, info, _ = _jpeg_dec.parse(jpeg_file_bytes(data))
    nc = int(info[2])
    return dict(supported=rc == 0, reason=jpeg_reason(rc, info), height=int(info[0]), width=int(info[1]), components=nc,
                sampling=[(int(info[9 + 5 * c]), int(info[10 + 5 * c])) for c in _range(min(nc, 3))] if nc in (1, 3) else [],
                restart_interval=int(info[3]), scan_offset=int(info[4]), scan_bytes=int(info[5]))


def jpeg_stage(parsed, pos=0):
    """Where the scans and tables of parsed files (file bytes, info, tables) go in a staging buffer, from byte `pos`:
    -> (copies [(offset, uint8 array)], per launch group of PREPROCESS_BATCH_MAX (index list, tables offset), end).  The
    scans lie back to back as they are in the files; a group's tables are contiguous and 16-byte aligned."""
    copies, groups, scan_at = [], [], []
    for data, info, _ in parsed:
        scan_at.append(pos)
        copies.append((pos, data[int(info[4]):int(info[4]) + int(info[5])]))
        pos += int(info[5])
    for i, j in _check.chunks(len(parsed)):
        index = list(_range(i, j))
        pos = -(-pos // 16) * 16
        groups.append((index, pos))
        for k in index:
            copies.append((pos, parsed[k][2]))
            pos += _jpeg_dec.TABLE_BYTES
    return copies, groups, scan_at, pos


def jpeg_decode_staged(up, parsed, groups, scan_at, dst_offsets, dst):
    """the decoder's launches behind the upload of a buffer laid out by jpeg_stage: image k of `parsed` goes to
    dst[dst_offsets[k]:] -> the int32 status words on the device, one per file (not fetched: no synchronisation)"""
    status = torch.empty((len(parsed),), dtype=torch.int32, device=up.device)
    with torch.cuda.device(up.device):
        for index, tables_at in groups:
            rows = [(scan_at[k], int(parsed[k][1][5]), int(parsed[k][1][0]), int(parsed[k][1][1]), dst_offsets[k]) for k in index]
            infos = np.stack([parsed[k][1] for k in index])
            ws = torch.empty((_jpeg_dec.workspace_bytes(rows, infos),), dtype=torch.uint8, device=up.device)
            _jpeg_dec.decode(up, rows, infos, up[tables_at:tables_at + len(index) * _jpeg_dec.TABLE_BYTES], dst,
                             status[index[0]:index[0] + len(index)], ws)
    return status


def jpeg_status_error(status, names):
    """ValueError naming the first file with a non-zero status word, or None; status: the words on the host"""
    for s, name in zip(status, names):
        if int(s) != 0:
            return ValueError(f"jpeg: {name}: the scan does not decode ({_jpeg_dec.STATUS.get(int(s), int(s))})")
    return None


def decode_jpeg(files, out=None, device="cuda:0", orientation=None):
    """Baseline JPEG files -> packed RGB HWC images on the device, decoded on the GPU (csrc/jpeg_dec.hip; the rule and the
    supported files are stated in include/codetr_jpeg_dec.h): only the headers are read on the host, the scans are
    uploaded as they are in the files, in one copy with their tables, and decoded by five launches per
    PREPROCESS_BATCH_MAX files.
      files   each bytes / bytearray / memoryview, a 1-D uint8 array or host tensor, or a path
      out     a flat uint8 device buffer to decode into (at least the returned layout's bytes) instead of a new one
      orientation  None: the images as they are stored.  "exif": every file turned as its EXIF orientation tag asks
              (jpeg_orientation); an int 1..8 for every file, or a list with one per file: the decoder writes a scratch
              buffer and one orient_frames launch per PREPROCESS_BATCH_MAX files writes the upright images (into `out`),
              whose sizes the returned list then holds
    -> (the flat uint8 buffer, [(offset, H, W)] per image); images start at multiples of 16 bytes, as stage_chunk lays
    them out.  ValueError naming the image and the reason for a bad header, a file outside the supported set, or a scan
    that does not decode."""
    if not len(files):
        raise ValueError("decode_jpeg: no files")
    parsed = []
    for i, item in enumerate(files):
        data = jpeg_file_bytes(item)
        rc, info, tables = _jpeg_dec.parse(data)
        if rc != 0:
            raise ValueError(f"decode_jpeg: image {i}: {jpeg_reason(rc, info)}")
        parsed.append((data, info, tables))
    staged, total = [], 0
    for _, info, _ in parsed:
        staged.append((total, int(info[0]), int(info[1])))
        total += _jpeg_dec.output_bytes(info[0], info[1])
    if orientation is not None:
        if isinstance(orientation, str) and orientation == "exif":
            orientation = [_orient_ops.jpeg_orientation(data) for data, _, _ in parsed]
        elif not isinstance(orientation, (list, tuple)):
            orientation = [orientation] * len(parsed)
        if len(orientation) != len(parsed):
            raise ValueError(f"decode_jpeg: {len(orientation)} orientations for {len(parsed)} files")
        upright, out = out, None   # the decoder's buffer is a scratch of this call
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=device)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
          or out.numel() < total):
        raise ValueError(f"decode_jpeg: out must be a contiguous flat uint8 buffer of at least {total} bytes on a GPU")
    copies, groups, scan_at, end = jpeg_stage(parsed)
    staging = torch.empty((end,), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    for at, part in copies:
        host[at:at + part.size] = part
    up = staging.to(out.device, non_blocking=True)
    status = jpeg_decode_staged(up, parsed, groups, scan_at, [o for o, _, _ in staged], out)
    err = jpeg_status_error(status.cpu().numpy(), [f"image {i}" for i in _range(len(parsed))])
    if err is not None:
        raise err
    if orientation is not None:
        return _orient_ops.orient_frames(out, [(o, H, W, at, 3 * W) for o, (at, H, W) in zip(orientation, staged)], upright)
    return out, staged


FRAME_FORMATS = _cabi.FRAME_FORMATS
FRAME_COLOR = dict(matrix="bt601", range="limited")   # what OpenCV's cvtColor(..., COLOR_YUV2RGB_NV12) computes
_range = range    # (frames_to_rgb has a parameter of that name)


def frames_to_rgb(src_u8, rows10, dst_bytes, matrix="bt601", range="limited", out=None):
    """Frames as decoders hand them out -> packed RGB HWC images in one new flat uint8 device buffer of `dst_bytes`
    bytes, one launch per PREPROCESS_BATCH_MAX frames (csrc/frames.hip; include/codetr_hip.h states the conversion).
      src_u8    one flat contiguous uint8 device buffer that holds every plane
      rows10    per frame (format, H, W, plane0_offset, plane0_pitch, plane1_offset, plane1_pitch, plane2_offset,
                plane2_pitch, dst_offset); format a name of FRAME_FORMATS or its code, offsets in bytes, the columns of
                a plane the format does not have 0
      matrix    'bt601' | 'bt709'; range 'limited' | 'full' (the YUV formats; ignored by the others)
      out       a flat uint8 buffer of dst_bytes on src_u8's GPU to write into instead of a new one (the frames of a
                chunk that lie in several source buffers: one call per source)
    -> the buffer; bytes outside the frames' images are not written.  ValueError for an unknown format, matrix or range
    and for a wrong dtype or shape; whatever else is inconsistent the entry point rejects before it launches."""
    _gpu(src_u8, "frames_to_rgb")
    _check.flat_u8("frames_to_rgb", src_u8)
    if matrix not in _cabi.COLOR_MATRICES or range not in _cabi.COLOR_RANGES:
        raise ValueError(f"frames_to_rgb: matrix one of {sorted(_cabi.COLOR_MATRICES)} and range one of "
                         f"{sorted(_cabi.COLOR_RANGES)}, got {matrix!r} / {range!r}")
    rows = []
    for r in rows10:
        if len(r) != 10:
            raise ValueError("frames_to_rgb: ten values per row (format, H, W, three (offset, pitch) pairs, dst_offset)")
        fmt = FRAME_FORMATS.get(r[0], r[0]) if isinstance(r[0], str) else r[0]
        if isinstance(fmt, str) or int(fmt) not in FRAME_FORMATS.values():
            raise ValueError(f"frames_to_rgb: unknown frame format {r[0]!r}; known: {sorted(FRAME_FORMATS)}")
        rows.append((int(fmt),) + tuple(int(v) for v in r[1:]))
    if not rows or int(dst_bytes) <= 0:
        raise ValueError("frames_to_rgb: no frames")
    if out is None:
        out = torch.empty((int(dst_bytes),), dtype=torch.uint8, device=src_u8.device)
    elif (not torch.is_tensor(out) or out.device != src_u8.device or out.dtype != torch.uint8 or out.dim() != 1
          or not out.is_contiguous() or out.numel() != int(dst_bytes)):
        raise ValueError("frames_to_rgb: out must be a contiguous flat uint8 buffer of dst_bytes on the source's GPU")
    dst = out
    with torch.cuda.device(src_u8.device):
        for i, j in _check.chunks(len(rows)):
            _cabi.frames_to_rgb(src_u8, rows[i:j], _cabi.COLOR_MATRICES[matrix],
                                _cabi.COLOR_RANGES[range], dst)
    return dst

