"""The host layer's shared pieces, on the CPU: the companion-header binder, the settings checker behind the eight
`*_settings` / `*_style` functions, the packed result's layout, and hip_ops' re-exports of the moved operators."""
import math
import types

import numpy as np
import pytest
import torch

from codetr import (_appearance, _assign, _cabi, _jpeg, _jpeg_dec, _motion, _redact, _wbf, detection_ops, hip_ops, image_ops,
                    track_ops)

COMPANIONS = ((_assign, "ASSIGN"), (_wbf, "WBF"), (_motion, "MOTION"), (_appearance, "APPEARANCE"), (_redact, "REDACT"),
              (_jpeg, "JPEG"), (_jpeg_dec, "JPEGDEC"))


def _stand_in(functions, version):
    """a plain object with one Python function per entry point; the version function answers `version`"""
    lib = types.SimpleNamespace()
    for name in functions:
        setattr(lib, name, (lambda v: lambda *a: v)(version if name.endswith("_abi_version") else 0))
    return lib


def test_companion_binder(monkeypatch):
    path, functions, defines, signatures, load = _cabi.companion("codetr_assign.h", "assign", "assignment")
    assert path == _assign.HEADER_PATH and functions == _assign.functions and signatures == _assign.SIGNATURES
    header = defines["CODETR_ASSIGN_ABI_VERSION"]

    lacking = _stand_in(functions, header)
    del lacking.codetr_assign_i32
    monkeypatch.setattr(_cabi, "_lib", lacking)
    with pytest.raises(ImportError, match="codetr_assign_i32") as e:
        load()
    assert _cabi.LIB_PATH in str(e.value)

    monkeypatch.setattr(_cabi, "_lib", _stand_in(functions, header + 1))
    with pytest.raises(ImportError, match=f"assignment ABI version {header + 1}, host expects {header};"):
        load()

    good = _stand_in(functions, header)
    monkeypatch.setattr(_cabi, "_lib", good)
    assert load() is good
    for name, (res, args) in signatures.items():
        assert getattr(good, name).restype is res and getattr(good, name).argtypes == args
    monkeypatch.setattr(_cabi, "_lib", _stand_in(functions, header + 1))   # not looked at again: the result is cached
    assert load() is good

    with pytest.raises(ImportError, match="codetr_absent.h"):
        _cabi.companion("codetr_absent.h", "absent", "absent")


@pytest.mark.parametrize("module,stem", COMPANIONS, ids=[s.lower() for _, s in COMPANIONS])
def test_companion_modules(module, stem):
    assert module.SIGNATURES.keys() == module.functions.keys() and callable(module.load)
    assert module.ABI_VERSION == module.defines[f"CODETR_{stem}_ABI_VERSION"]
    assert f"codetr_{stem.lower()}_abi_version" in module.functions


# ---- settings: (function, what its messages start with, the defaults, {numeric key: (lo, hi, step, NaN is refused)}) --
# lo / hi None: no such end.  The expected dicts are what the functions returned before they shared one checker.
INT_MAX = 2 ** 31 - 1
SETTINGS = [
    ("wbf_settings", "wbf", dict(iou_threshold=0.55, skip_box_thr=0.0, conf_type="avg", weights=None),
     dict(iou_threshold=(None, None, 0, True), skip_box_thr=(None, None, 0, True))),
    ("slice_merge_settings", "slice merge", dict(type="nmm", metric="ios", threshold=0.5, class_agnostic=False),
     dict(threshold=(None, None, 0, True))),
    ("draw_style", "draw style:", dict(line_width=3, alpha=0.8, score_thr=0.3, text_color=(200, 200, 200), font_scale=1,
                                       draw_labels=True),
     dict(line_width=(1, 15, 1, True), font_scale=(1, 4, 1, True), alpha=(0, 1, 0.01, True), score_thr=(None, None, 0, False))),
    ("redact_style", "redact:", dict(mode="pixelate", score_thr=0.3, expand=0.1, shape="box", cell=16, fill=(0, 0, 0)),
     dict(expand=(0, 1, 0.01, True), score_thr=(None, None, 0, False), cell=(4, 64, 1, True))),
    ("jpeg_settings", "jpeg:", dict(quality=90, subsampling="420"), dict(quality=(1, 100, 1, True))),
    ("track_settings", "tracker", dict(obj_score_thrs=dict(high=0.6, low=0.1), init_track_thr=0.7,
                                       weight_iou_with_det_scores=True, match_iou_thrs=dict(high=0.1, low=0.5, tentative=0.3),
                                       num_frames_retain=30, num_tentatives=3, max_tracks=256),
     dict(init_track_thr=(None, None, 0, True), num_frames_retain=(1, INT_MAX, 1, True), num_tentatives=(1, INT_MAX, 1, True),
          max_tracks=(1, 512, 1, True))),
    ("appearance_settings", "appearance", dict(appearance_thr=0.75, proximity_thr=0.5, reid_gate=1.5),
     dict(appearance_thr=(0, 1, 0.01, True), proximity_thr=(0, 1, 0.01, True), reid_gate=(0, None, 0.01, True))),
    ("motion_settings", "motion", dict(grid=160, search=8, texture=2, min_blocks=4),
     dict(grid=(32, 160, 1, True), search=(1, 16, 1, True), texture=(0, 65535, 1, True), min_blocks=(1, 100, 1, True))),
]
# (function, a valid input, what it returned before)
VALID = [
    ("wbf_settings", dict(iou_threshold=1, skip_box_thr=0.25, conf_type="max", weights=(1, 2.5)),
     dict(iou_threshold=1.0, skip_box_thr=0.25, conf_type="max", weights=[1.0, 2.5])),
    ("slice_merge_settings", dict(type="nms", metric="iou", threshold=1, class_agnostic=1),
     dict(type="nms", metric="iou", threshold=1.0, class_agnostic=True)),
    ("draw_style", dict(line_width=2.0, alpha=1, score_thr=0, text_color=[1.0, 2, 255], font_scale=4, draw_labels=0),
     dict(line_width=2, alpha=1.0, score_thr=0.0, text_color=(1, 2, 255), font_scale=4, draw_labels=False)),
    ("redact_style", dict(mode="fill", score_thr=1, expand=0, shape="ellipse", cell=64, fill=[1.0, 2, 255]),
     dict(mode="fill", score_thr=1.0, expand=0.0, shape="ellipse", cell=64, fill=(1, 2, 255))),
    ("jpeg_settings", dict(quality=75.0, subsampling="444"), dict(quality=75, subsampling="444")),
    ("track_settings", dict(obj_score_thrs=dict(low=0), match_iou_thrs=dict(tentative=1), init_track_thr=1,
                            weight_iou_with_det_scores=0, num_frames_retain=1, num_tentatives=2, max_tracks=512),
     dict(obj_score_thrs=dict(high=0.6, low=0.0), init_track_thr=1.0, weight_iou_with_det_scores=False,
          match_iou_thrs=dict(high=0.1, low=0.5, tentative=1.0), num_frames_retain=1, num_tentatives=2, max_tracks=512)),
    ("appearance_settings", dict(appearance_thr=1, proximity_thr=0, reid_gate=7),
     dict(appearance_thr=1.0, proximity_thr=0.0, reid_gate=7.0)),
    ("motion_settings", dict(grid=32, search=16, texture=0, min_blocks=100), dict(grid=32, search=16, texture=0, min_blocks=100)),
]


def _same(a, b):
    """equal dicts with values of equal types (1 and 1.0 are not the same result)"""
    return a == b and all(type(a[k]) is type(b[k]) and (not isinstance(a[k], dict) or _same(a[k], b[k])) for k in a)


@pytest.mark.parametrize("name,prefix,defaults,numeric", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_settings_table(name, prefix, defaults, numeric):
    f = getattr(hip_ops, name)
    assert _same(f(None), defaults) and _same(f({}), defaults) and f() is not f()
    with pytest.raises(ValueError) as e:
        f(dict(no_such_key=1))
    assert str(e.value).startswith(prefix.rstrip(":") + ":") and "no_such_key" in str(e.value)
    assert all(repr(k) in str(e.value) for k in defaults)            # the known keys are listed
    for key, (lo, hi, step, nan) in numeric.items():
        bad = [True, "x"] + ([float("nan")] if nan else [])
        bad += ([] if lo is None else [lo - step]) + ([] if hi is None else [hi + step])
        for v in bad:
            with pytest.raises(ValueError, match=key) as e:
                f({key: v})
            assert str(e.value).startswith(prefix), (key, v, str(e.value))
        whole = isinstance(defaults[key], int)
        for v in (defaults[key], lo, hi):
            if v is not None:
                scalar = np.int64(v) if whole else np.float64(v)
                assert _same(f({key: scalar}), f({key: int(v) if whole else float(v)})), (key, v)


@pytest.mark.parametrize("name,given,expected", VALID, ids=[v[0] for v in VALID])
def test_settings_valid_inputs(name, given, expected):
    assert _same(getattr(hip_ops, name)(given), expected)


def test_settings_cross_field_rules():
    track = hip_ops.track_settings
    assert track(dict(obj_score_thrs=dict(low=0.6)))["obj_score_thrs"] == dict(high=0.6, low=0.6)
    with pytest.raises(ValueError, match="obj_score_thrs: low must not exceed high"):
        track(dict(obj_score_thrs=dict(low=0.7)))
    with pytest.raises(ValueError, match="obj_score_thrs: low must not exceed high"):
        track(dict(obj_score_thrs=dict(high=0.05)))
    # the nested dicts are partial: the other thresholds keep their defaults, and the defaults are not written to
    got = track(dict(match_iou_thrs=dict(low=np.float32(0.25))))
    assert _same(got["match_iou_thrs"], dict(high=0.1, low=0.25, tentative=0.3)) and hip_ops.TRACKER["match_iou_thrs"]["low"] == 0.5
    assert got["obj_score_thrs"] is not hip_ops.TRACKER["obj_score_thrs"]
    for bad in (dict(obj_score_thrs=0.5), dict(obj_score_thrs=dict(middle=0.5)), dict(match_iou_thrs=[0.1, 0.5, 0.3])):
        with pytest.raises(ValueError, match=f"tracker {list(bad)[0]}"):
            track(bad)
    for bad in (True, "x", float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"tracker obj_score_thrs\.high"):
            track(dict(obj_score_thrs=dict(high=bad)))
    for conf in ("box_and_model_avg", "absent_model_aware_avg"):
        with pytest.raises(NotImplementedError, match=conf):
            hip_ops.wbf_settings(dict(conf_type=conf))
    with pytest.raises(ValueError, match="conf_type"):
        hip_ops.wbf_settings(dict(conf_type="median"))
    with pytest.raises(ValueError, match="wbf must be None or a dict"):
        hip_ops.wbf_settings("avg")


def test_settings_numpy_values_and_coercion():
    # numpy scalars inside a colour, for a cell, and numpy strings for a name
    assert _same(hip_ops.draw_style(dict(text_color=[np.uint8(1), np.float32(2), np.int64(255)])),
                 hip_ops.draw_style(dict(text_color=(1, 2, 255))))
    assert _same(hip_ops.redact_style(dict(fill=(np.int32(7), np.float64(8), 9), cell=np.int64(32), mode=np.str_("blur"))),
                 hip_ops.redact_style(dict(fill=(7, 8, 9), cell=32, mode="blur")))
    for bad in ([np.int64(256), 0, 0], [np.float32(0.5), 0, 0], np.zeros(3, np.uint8)):
        with pytest.raises(ValueError, match="fill"):
            hip_ops.redact_style(dict(fill=bad))
    with pytest.raises(ValueError, match="cell"):
        hip_ops.redact_style(dict(cell=np.float64(16)))
    assert hip_ops.slice_merge_settings(dict(type=np.str_("nms")))["type"] == "nms"
    # the thresholds of wbf and slice merge went through float() and still take what float() takes; only a bool is refused
    for value in ("0.5", np.float32(0.5), np.array(0.5), torch.tensor(0.5), np.bool_(False)):
        want = float(value)
        assert _same(hip_ops.wbf_settings(dict(iou_threshold=value, skip_box_thr=value)),
                     dict(hip_ops.WBF, iou_threshold=want, skip_box_thr=want))
        assert _same(hip_ops.slice_merge_settings(dict(threshold=value)), dict(hip_ops.SLICE_MERGE, threshold=want))
    for value in (None, [0.5, 0.5]):            # what float() cannot take is a TypeError, as it was
        with pytest.raises(TypeError):
            hip_ops.wbf_settings(dict(iou_threshold=value))
        with pytest.raises(TypeError):
            hip_ops.slice_merge_settings(dict(threshold=value))
    for value in (False, "nan", float("inf"), torch.tensor(float("inf"))):
        with pytest.raises(ValueError, match="skip_box_thr"):
            hip_ops.wbf_settings(dict(skip_box_thr=value))
        with pytest.raises(ValueError, match="threshold"):
            hip_ops.slice_merge_settings(dict(threshold=value))
    with pytest.raises(ValueError, match="alpha"):                      # a huge int is out of range, not an overflow
        hip_ops.draw_style(dict(alpha=10 ** 400))
    with pytest.raises(ValueError, match="line_width"):
        hip_ops.draw_style(dict(line_width=float("inf")))


# ---- the packed result ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,es", [(torch.float16, 2), (torch.float32, 4)], ids=["f16", "f32"])
@pytest.mark.parametrize("kind", ["Detections", "SoftDetections", "WbfDetections"])
def test_packed_layout(kind, dtype, es):
    N, Q = 2, 3
    index, votes = kind != "Detections", kind == "WbfDetections"
    dets = detection_ops.packed_detections(N, Q, dtype, index, votes, device="cpu", zeros=True)
    assert type(dets) is getattr(hip_ops, kind) and dets.packed.dtype == torch.uint8 and dets.packed.dim() == 1
    # labels, count, [index], [votes], boxes, scores, back to back
    at = dict(labels=0, count=8 * N * Q)
    ints = 8 * N * Q + 4 * N
    if index:
        at["index"] = ints
        ints += 4 * N * Q
    if votes:
        at["votes"] = ints
        ints += 4 * N * Q
    at["boxes"], at["scores"] = ints, ints + 4 * N * Q * es
    assert dets.packed.numel() == ints + 5 * N * Q * es
    want = dict(labels=(torch.int64, (N, Q)), count=(torch.int32, (N,)), index=(torch.int32, (N, Q)),
                votes=(torch.int32, (N, Q)), boxes=(dtype, (N, Q, 4)), scores=(dtype, (N, Q)))
    assert set(at) == set(dets._fields) - {"packed"}
    for field, offset in at.items():
        view = getattr(dets, field)
        assert view.dtype == want[field][0] and tuple(view.shape) == want[field][1], field
        assert view.data_ptr() - dets.packed.data_ptr() == offset, field
    # a CPU-resident result comes back from detections_to_host as equal views of a buffer laid out the same way
    dets.packed.copy_(torch.arange(dets.packed.numel()) % 120)
    host = hip_ops.detections_to_host(dets)
    assert type(host) is type(dets) and torch.equal(host.packed, dets.packed)
    for field in at:
        assert torch.equal(getattr(host, field), getattr(dets, field)), field
        assert getattr(host, field).data_ptr() - host.packed.data_ptr() == at[field], field


# ---- hip_ops still holds every public name it had before the Inferencer-side operators moved out -----------------------
PUBLIC = [
    'APPEARANCE', 'APPEARANCE_BINS', 'ASSIGN_MAX_COLS', 'ASSIGN_MAX_GAIN', 'ASSIGN_MAX_ROWS', 'DRAW_MAX_Q', 'DRAW_MAX_SIDE',
    'DRAW_NAME_ROW', 'DRAW_STYLE', 'Detections', 'ENC_POSGEN', 'ENC_PROJ_FUSED', 'FFN_FUSED_MIN_ROWS', 'FFN_OPROJ', 'FP8',
    'FP8_MAX', 'FP8_MIN_TILES', 'FRAME_COLOR', 'FRAME_FORMATS', 'JPEG_DECODE_STATS', 'JPEG_DOWNLOADS', 'JPEG_SETTINGS',
    'KERNEL_PROFILE', 'LINEAR_PP', 'LINEAR_PROFILE', 'LN_GEMM', 'MERGE_LN', 'MOTION', 'MOTION_MODELS', 'MSDA_ENCODER',
    'MSDA_FP32_REF', 'MSDA_V4', 'MSDA_V4_HEAD_MAJOR', 'MSDA_V4_LDS_BUDGET', 'MSDA_V4_MARGIN_CAP', 'MSDA_V4_REGION',
    'MSDA_V4_THREADS', 'MotionState', 'NATIVE', 'PREPROCESS_BATCH_MAX', 'R50_CONV_IM2COL', 'R50_NATIVE', 'REDACT',
    'REDACT_CELLS', 'REDACT_MODES', 'REDACT_SHAPES', 'SLICE_MAX_VIEWS', 'SLICE_MERGE', 'SWIN_MLP', 'SWIN_MLP_MIN_ROWS',
    'SoftDetections', 'TRACKER', 'TRACK_ASSOCIATIONS', 'TRACK_MAX_TRACKS', 'TTA_MAX_CANDIDATES', 'TTA_MAX_VIEWS',
    'TrackState', 'WBF', 'WBF_MAX_CANDIDATES', 'WINDOW_BIAS_LANE', 'WbfDetections', 'XADD', 'XADD_MIN_ROWS', 'add',
    'appearance_descriptors', 'appearance_settings', 'appearance_state_to_host', 'batched_nms', 'cast_fp8', 'cast_fp8mx',
    'conv2d', 'conv_tokens', 'decode_boxes', 'decode_boxes_supported', 'decode_jpeg', 'derived', 'detections_to_host',
    'draw_detections', 'draw_names_table', 'draw_style', 'encode_jpeg', 'encoder_geometry', 'encoder_projections',
    'estimate_motion', 'ffn_fp8', 'ffn_fp8_supported', 'ffn_fp8_weights', 'ffn_fused', 'ffn_fused_supported',
    'ffn_oproj_fused', 'fp8_weight', 'frames_to_rgb', 'gather_rows', 'group_norm', 'groupnorm_tokens_into',
    'groupnorm_tokens_supported', 'im2col_tokens', 'jpeg_decode_staged', 'jpeg_file_bytes', 'jpeg_host_decode', 'jpeg_info',
    'jpeg_out_stride', 'jpeg_parse', 'jpeg_reason', 'jpeg_settings', 'jpeg_stage', 'jpeg_status_error', 'layer_norm',
    'layer_norm_fp8', 'layer_norm_fp8mx', 'level_cums', 'linear', 'linear_assignment', 'linear_fp8', 'linear_fp8_supported',
    'linear_fp8mx', 'linear_ln', 'linear_ln_supported', 'linear_xadd', 'linear_xadd_supported', 'mask_pyramid',
    'maxpool_tokens', 'mha_self_attention', 'motion_settings', 'motion_state_to_host', 'msda', 'msda_encoder_packed',
    'msda_encoder_packed_supported', 'msda_encoder_windows_packed', 'msda_fused', 'msda_fused_supported',
    'msda_head_major_supported', 'msda_packed_projection', 'mx_dequant', 'new_appearance_state', 'new_motion_state',
    'new_track_state', 'nondefault_switches', 'patch_embed', 'patch_embed_supported', 'patch_merge_layernorm',
    'patch_merge_layernorm_supported', 'postprocess_detections', 'postprocess_detections_soft', 'preprocess_batch',
    'preprocess_image', 'preprocess_tiles', 'preprocess_views', 'query_sine_embed', 'query_sine_embed_supported',
    'redact_detections', 'redact_style', 'row_max', 'sigmoid', 'sine_pos_tokens_into', 'slice_merge', 'slice_merge_settings',
    'soft_nms', 'stem_conv_tokens', 'swin_mlp', 'swin_mlp_supported', 'swin_window_attention',
    'swin_window_attention_supported', 'topk', 'track_settings', 'track_state_to_host', 'track_streams', 'track_update',
    'tta_merge', 'valid_ratios', 'value_projection_f16', 'wbf_merge', 'wbf_settings', 'weighted_boxes_fusion',
    'window_attention']


def test_hip_ops_reexports():
    homes = (detection_ops, image_ops, track_ops)
    for name in PUBLIC:
        assert hasattr(hip_ops, name), name
    exported = [name for home in homes for name in home.__all__]
    assert len(exported) == len(set(exported)) and set(exported) <= set(PUBLIC)     # each moved name has one home
    for home in homes:
        for name in home.__all__:
            assert getattr(hip_ops, name) is vars(home)[name], (name, home.__name__)
        # what a module does not list stays its own: an imported module or a helper is no name of hip_ops
        assert not [n for n in vars(home) if not n.startswith("_") and n not in home.__all__ and hasattr(hip_ops, n)
                    and n not in ("torch", "math")], home.__name__
    assert hip_ops.Detections is detection_ops.Detections and hip_ops.DRAW_STYLE is image_ops.DRAW_STYLE
    assert hip_ops.track_update is track_ops.track_update and track_ops.track_update.__module__ == "codetr.track_ops"
    assert hip_ops.JPEG_DOWNLOADS is image_ops.JPEG_DOWNLOADS     # the counters are the one object, not a copy
    assert math.isclose(hip_ops.WBF["iou_threshold"], 0.55) and hip_ops.linear.__module__ == "codetr.hip_ops"
