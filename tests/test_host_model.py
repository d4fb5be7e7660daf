"""CPU: host logic of the product package -- config loading, model construction, checkpoint-key
parity with the reference, loader behaviour.  No compute (the product computes on the GPU only)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from helpers_model import unpack_param_spec

CFG_DIR = os.path.join(ROOT, "co-detr-tensorrt_amd", "configs")
SWIN_CFG = os.path.join(CFG_DIR, "co_dino_5scale_swin_l_16xb1_16e_o365tococo.py")
R50_CFG = os.path.join(CFG_DIR, "co_dino_5scale_r50_8xb2_1x_coco.py")


def test_config_base_chain_delete_and_base_refs():
    from codetr.config import Config

    cfg = Config.fromfile(SWIN_CFG)
    m = cfg.model
    assert m.type == "CoDETR"
    assert m.backbone.type == "SwinTransformer" and "depth" not in m.backbone          # _delete_=True
    assert m.backbone.depths == [2, 2, 18, 2] and m.backbone.num_heads == [6, 12, 24, 48]
    assert m.neck.in_channels == [192, 384, 768, 1536] and m.neck.num_outs == 5       # deep merge
    assert m.query_head.transformer.encoder.with_cp == 6                               # 3-level deep merge
    assert m.query_head.transformer.encoder.num_layers == 6
    assert m.query_head.positional_encoding.temperature == 20
    assert m.use_lsj is False                                                          # from the r50 child
    assert cfg.dataset_type == "CocoDataset"                                           # from the mmdet:: base
    r50 = Config.fromfile(R50_CFG)
    assert r50.model.backbone.type == "ResNet"
    assert r50.test_pipeline[0]["backend_args"] is None                                # `_base_.backend_args`


def _tuples(d):
    return tuple(d["__tuple__"]) if set(d) == {"__tuple__"} else d


def test_reference_config_files_load_and_agree():
    """The reference's own Swin-L config file, read through the same loader (its inference-relevant model section,
    captured into tests/golden/ref_config_swin_l.json by make_golden.py), equals ours."""
    from codetr.config import Config

    with open(os.path.join(GOLDEN, "ref_config_swin_l.json")) as f:
        ref = json.load(f, object_hook=_tuples)
    ours = Config.fromfile(SWIN_CFG)
    assert ref["backbone"] == dict(ours.model.backbone)
    assert ref["neck"] == ours.model.neck
    for k in ("num_query", "num_classes", "as_two_stage", "transformer", "positional_encoding"):
        assert ref["query_head"][k] == ours.model.query_head[k], k
    assert ref["test_cfg0"] == ours.model.test_cfg[0]
    assert ref["data_preprocessor_mean"] == ours.model.data_preprocessor.mean


@pytest.fixture(scope="module")
def swin_l_model():
    import codetr

    return codetr.build_CoDETR(SWIN_CFG, None, "cpu")


def test_state_dict_matches_reference_keys_and_shapes(swin_l_model):
    g = np.load(os.path.join(GOLDEN, "state_dict_keys.npz"))
    ref = dict(unpack_param_spec(g))
    own = {k: tuple(v.shape) for k, v in swin_l_model.state_dict().items()}
    for k, shp in ref.items():
        assert k in own, f"reference key {k} missing"
        assert own[k] == shp, (k, own[k], shp)
    # backbone, transformer AND the head's own parameters (class / box branches, `downsample`) are pinned by the
    # reference-built key list: nothing of ours under those prefixes may be missing from it either
    extra = [k for k in own if k.startswith(("backbone.", "query_head.")) and k not in ref]
    assert not extra, extra
    assert sum(1 for k in ref if k.startswith("query_head.cls_branches.")) == 14        # 7 x (weight, bias)
    assert sum(1 for k in ref if k.startswith("query_head.reg_branches.")) == 42        # 7 x 3 Linears
    assert ref["query_head.downsample.0.weight"] == (256, 256, 3, 3)
    blk = swin_l_model.backbone.stages[0].blocks[0].attn.w_msa
    assert np.array_equal(blk.relative_position_index.numpy(), g["rel_index"])
    # the neck's keys follow mmdet's ConvModule names (mmdet is absent: no reference-built list) -- spot-check the
    # contract of SURVEY 8(f)-2
    for k in ("neck.convs.0.conv.weight", "neck.convs.3.gn.bias", "neck.extra_convs.0.conv.weight",
              "neck.extra_convs.0.gn.weight", "query_head.cls_branches.6.weight", "query_head.reg_branches.6.4.bias",
              "query_head.reg_branches.0.0.weight", "query_head.downsample.0.weight", "query_head.downsample.1.bias"):
        assert k in own, k
    assert "neck.convs.0.conv.bias" not in own  # conv followed by GN has no bias
    assert own["query_head.cls_branches.0.weight"] == (80, 256)


def test_model_sizes(swin_l_model):
    nb = sum(p.numel() for p in swin_l_model.backbone.parameters())
    nt = sum(p.numel() for p in swin_l_model.query_head.transformer.parameters())
    assert abs(nb / 1e6 - 195.2) < 0.05 and abs(nt / 1e6 - 18.0) < 0.05  # SURVEY section 8 [probe]


def test_build_returns_model_only_without_weights_and_pair_with(tmp_path, swin_l_model):
    import codetr

    assert isinstance(swin_l_model, codetr.CoDETR) and not swin_l_model.training
    sd = {k: v for k, v in swin_l_model.state_dict().items()}
    sd["rpn_head.rpn_conv.weight"] = torch.zeros(1)          # training-only keys are ignored
    sd["query_head.label_embedding.weight"] = torch.zeros(1)
    path = tmp_path / "ckpt.pth"
    torch.save({"state_dict": sd, "meta": {"dataset_meta": {"CLASSES": ("a", "b")}}}, path)
    with pytest.warns(UserWarning, match="unexpected keys"):
        model, meta = codetr.build_CoDETR(SWIN_CFG, str(path), "cpu")
    assert meta["classes"] == ("a", "b") and meta["palette"] == "coco"
    assert torch.equal(model.state_dict()["backbone.norm3.weight"], sd["backbone.norm3.weight"])


def test_r50_config_builds():
    import codetr

    m = codetr.build_CoDETR(R50_CFG, None, "cpu")
    assert type(m.backbone).__name__ == "ResNet"
    assert m.neck.convs[3].conv.weight.shape == (256, 2048, 1, 1)
    assert "backbone.layer3.5.conv2.weight" in m.state_dict()


def test_msda_module_contract():
    from codetr.multi_scale_deformable_attention import MultiScaleDeformableAttention

    with pytest.raises(ValueError, match="divisible"):
        MultiScaleDeformableAttention(embed_dims=100, num_heads=8)
    m = MultiScaleDeformableAttention(embed_dims=256, num_levels=5)
    assert m.sampling_offsets.weight.shape == (8 * 5 * 4 * 2, 256) and m.attention_weights.weight.shape == (160, 256)
    # grid-pattern bias: head 0 points along +x with magnitudes 1..4
    b = m.sampling_offsets.bias.view(8, 5, 4, 2)
    torch.testing.assert_close(b[0, :, :, 0], torch.arange(1.0, 5.0).expand(5, 4))
    assert float(b[0, :, :, 1].abs().max()) < 1e-6
    # hip_ops itself never computes on the CPU (the module's CPU dispatch is its own torch-only branch, tested below)
    from codetr import hip_ops

    with pytest.raises(RuntimeError, match="MI355X only"):
        hip_ops.linear(torch.zeros(3, 256), m.value_proj.weight, m.value_proj.bias)


def test_msda_module_cpu_dispatch_vs_reference_module():
    """CPU tensors take the module's torch-only branch + ops.multi_scale_deformable_attention_pytorch, as the
    reference's module does (multi_scale_deformable_attention.py:203-210); checked against outputs captured from the
    REFERENCE's module (tests/golden/model_msda_module.npz, 2-d and 4-d reference points, padding mask)."""
    from codetr.multi_scale_deformable_attention import MultiScaleDeformableAttention
    from helpers_model import seeded_params

    g = np.load(os.path.join(GOLDEN, "model_msda_module.npz"))
    m = MultiScaleDeformableAttention(embed_dims=256, num_levels=5, dropout=0.0).eval()
    m.load_state_dict(seeded_params(unpack_param_spec(g), int(g["seed"])))
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    ss, ls = t("spatial_shapes"), t("level_start_index")
    with torch.no_grad():
        out2 = m(t("value"), value=None, query_pos=t("query_pos"), key_padding_mask=t("key_padding_mask"),
                 reference_points=t("ref2"), spatial_shapes=ss, level_start_index=ls)
        out4 = m(t("query4"), value=t("value"), query_pos=t("query_pos4"), key_padding_mask=t("key_padding_mask"),
                 reference_points=t("ref4"), spatial_shapes=ss, level_start_index=ls)
    np.testing.assert_allclose(out2.numpy(), g["out2"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(out4.numpy(), g["out4"], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("name", ["msda_g1", "msda_g2", "msda_g3_dec"])
def test_pytorch_formulation_of_the_op_vs_reference_goldens(name):
    """ops.multi_scale_deformable_attention_pytorch (explicit corner gather) against the reference's own outputs"""
    from codetr.ops import multi_scale_deformable_attention_pytorch as f

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    t = lambda k: torch.from_numpy(np.asarray(g[k]))  # noqa: E731
    out = f(t("value").double(), t("spatial_shapes"), t("sampling_loc").double(), t("attn_weight").double())
    ref = g["out_f64"] if "out_f64" in g.files else g["out"]
    # (the g3 fixture stores its inputs rounded to fp32 next to an output computed before the rounding)
    tol = 1e-9 if name != "msda_g3_dec" else 1e-6
    np.testing.assert_allclose(out.numpy(), ref, rtol=tol, atol=tol * 1e-2)
    # differentiable, like the reference's formulation (torch.autograd.gradcheck is what its test runs on the op)
    v = t("value").double()[:, :, :1, :2].clone().requires_grad_(True)
    loc = t("sampling_loc").double()[:, :2, :1].clone().requires_grad_(True)
    w = t("attn_weight").double()[:, :2, :1].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: f(a, t("spatial_shapes"), b, c), (v, loc, w), eps=1e-6, atol=1e-4)


def test_swin_converter_known_answer():
    from codetr.swin import swin_converter

    C = 2
    red = torch.arange(3 * 4 * C, dtype=torch.float32).view(3, 4 * C)  # official order: [x0 | x1 | x2 | x3] blocks of C
    norm = torch.arange(4 * C, dtype=torch.float32)
    out = swin_converter({"layers.0.downsample.reduction.weight": red, "layers.0.downsample.norm.weight": norm,
                          "layers.1.blocks.0.attn.qkv.weight": torch.zeros(1), "layers.1.blocks.0.mlp.fc1.bias": torch.zeros(1),
                          "patch_embed.proj.weight": torch.zeros(1), "head.weight": torch.zeros(1)})
    assert set(out) == {"backbone.stages.0.downsample.reduction.weight", "backbone.stages.0.downsample.norm.weight",
                        "backbone.stages.1.blocks.0.attn.w_msa.qkv.weight", "backbone.stages.1.blocks.0.ffn.layers.0.0.bias",
                        "backbone.patch_embed.projection.weight"}
    # unfold order is channel-major: new[c*4 + j] = old[perm[j]*C + c] with perm = (0, 2, 1, 3)
    exp = torch.tensor([norm[p * C + c] for c in range(C) for p in (0, 2, 1, 3)])
    torch.testing.assert_close(out["backbone.stages.0.downsample.norm.weight"], exp)
    torch.testing.assert_close(out["backbone.stages.0.downsample.reduction.weight"][1], red[1][exp.long()])


def test_derived_weight_cache_lives_on_the_parameter_and_tracks_changes():
    """hip_ops.derived: rebuilt on in-place edits, on `param.data = ...` and when the parameter object is
    replaced; not rebuilt otherwise; gone with the parameter."""
    from codetr import hip_ops

    lin = torch.nn.Linear(4, 3)
    calls = []

    def get():
        w = lin.weight
        return hip_ops.derived((w, lin.bias), "_t_cache", lambda: (calls.append(1), w.detach().clone() * 2)[1])

    a = get()
    assert get() is a and len(calls) == 1
    with torch.no_grad():
        lin.weight.mul_(3.0)                       # in-place: version counter
    b = get()
    assert len(calls) == 2 and torch.equal(b, lin.weight.detach() * 2)
    lin.weight.data = torch.ones(3, 4)             # storage swap, same object, same version
    c = get()
    assert len(calls) == 3 and torch.equal(c, torch.full((3, 4), 2.0))
    lin.bias = torch.nn.Parameter(torch.zeros(3))  # a source other than the owner is replaced
    get()
    assert len(calls) == 4
    lin.weight = torch.nn.Parameter(torch.ones(3, 4))   # the owner is replaced: the cache went with the old object
    assert not hasattr(lin.weight, "_t_cache")
    get()
    assert len(calls) == 5


def test_swin_load_pretrained_resizes_relative_position_tables():
    """reference swin.py:705-720: a table trained with another window size is resized bicubically, [L1,nH] ->
    [1,nH,S1,S1] -> (S2,S2) -> [L2,nH]; official-Swin key names are converted when convert_weights is set"""
    from codetr.swin import SwinTransformer

    kw = dict(embed_dims=32, depths=(2, 2), num_heads=(1, 2), strides=(4, 2), out_indices=(0, 1), patch_norm=True)
    src = SwinTransformer(window_size=4, **kw)
    src.init_weights()
    dst = SwinTransformer(window_size=6, **kw)
    res = dst.load_pretrained({"state_dict": {"backbone." + k: v for k, v in src.state_dict().items()}})
    assert not res.unexpected_keys
    key = "stages.1.blocks.0.attn.w_msa.relative_position_bias_table"
    pre = src.state_dict()[key]                                   # [(2*4-1)^2, 2]
    want = torch.nn.functional.interpolate(pre.permute(1, 0).reshape(1, 2, 7, 7), size=(11, 11), mode="bicubic")
    torch.testing.assert_close(dst.state_dict()[key], want.view(2, 121).permute(1, 0))
    assert torch.equal(dst.state_dict()["stages.0.blocks.1.ffn.layers.1.weight"], src.state_dict()["stages.0.blocks.1.ffn.layers.1.weight"])
    # official key names (layers / attn / mlp.fc1 / patch_embed.proj) through swin_converter
    official = {}
    for k, v in src.state_dict().items():
        if "relative_position_index" in k:
            continue
        k2 = k.replace("stages", "layers", 1).replace("attn.w_msa.", "attn.").replace("ffn.layers.0.0.", "mlp.fc1.") \
            .replace("ffn.layers.1.", "mlp.fc2.").replace("patch_embed.projection", "patch_embed.proj")
        official[k2] = v
    dst2 = SwinTransformer(window_size=4, convert_weights=True, **kw)
    res2 = dst2.load_pretrained({"model": official})
    assert not res2.unexpected_keys and all("relative_position_index" in k for k in res2.missing_keys)
    assert torch.equal(dst2.state_dict()["stages.0.blocks.0.attn.w_msa.qkv.weight"], src.state_dict()["stages.0.blocks.0.attn.w_msa.qkv.weight"])


def test_checkpoint_loader_refuses_pickled_objects_unless_opted_in(tmp_path):
    from codetr.checkpoint import load_checkpoint

    good = tmp_path / "good.pth"
    torch.save({"state_dict": {"w": torch.zeros(2)}, "meta": {"CLASSES": ("a", "b")}}, good)
    assert load_checkpoint(str(good))["meta"]["CLASSES"] == ("a", "b")

    import fractions

    bad = tmp_path / "bad.pth"   # an arbitrary (non-allow-listed) pickled object: weights_only refuses it
    torch.save({"state_dict": {"w": torch.zeros(2)}, "meta": fractions.Fraction(1, 2)}, bad)
    with pytest.raises(RuntimeError, match="allow_pickle"):
        load_checkpoint(str(bad))
    assert load_checkpoint(str(bad), allow_pickle=True)["meta"] == fractions.Fraction(1, 2)


def test_fragment_major_packing_layout():
    """codetr.transformer.pack_fragment_major: element (tile, ks, lane = 16 g + r, e) of the packed blob is
    w[16 tile + r][32 ks + 8 g + e] (the layout include/codetr_hip.h documents for codetr_decoder_layer_f16)"""
    import torch
    from codetr.transformer import pack_fragment_major

    g = torch.Generator().manual_seed(0)
    w = torch.randn(20, 96, generator=g)
    p = pack_fragment_major(w, rows=32)
    assert p.shape == (32 * 96,)
    K = 96
    for tile, ks, gq, r, e in [(0, 0, 0, 0, 0), (0, 2, 3, 15, 7), (1, 1, 2, 3, 5), (1, 0, 0, 4, 0), (1, 2, 1, 9, 3)]:
        lane = 16 * gq + r
        got = float(p[((tile * (K // 32) + ks) * 64 + lane) * 8 + e])
        row, col = 16 * tile + r, 32 * ks + 8 * gq + e
        assert got == (float(w[row, col]) if row < 20 else 0.0)
