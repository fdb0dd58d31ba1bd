"""Distilled DeiT, the parts that need no GPU: the additive C ABI (new symbols, ABI still 7, argument refusals of ssp2_create_ext and
ssp2_attention_prefix_bf16 before the device is touched), ingest of the timm / old-HF / transformers DeiT anatomies and their state
dicts into the flat dictionary, refusal of the layouts the engine cannot represent, and the model table."""
import copy
import ctypes as C
import os

import pytest
import torch
import torch.nn as nn

from conftest import PKG
from deit_models import build_distilled


def _lib():
    from ssp2vit import _lib
    return _lib, _lib.load()


def _w(name="deit_test_distilled_patch16_32", **kw):
    from ssp2vit.weights import synthetic_weights
    return synthetic_weights(name, classes=10, seed=1, **kw)


def test_new_entries_are_exported_and_the_abi_stays_7():
    L, lib = _lib()
    assert L.ABI_VERSION == 7 and lib.ssp2_abi_version() == 7
    for name in ("ssp2_create_ext", "ssp2_attention_prefix_bf16"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert L.OPT_COUNT == 14
    assert L.T_KINDS[-3:] == ["dist", "head_dist_w", "head_dist_b"] and L.T_KINDS.index("head_b") == 19
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "ssp2vit.h")).read()
    assert "#define SSP2_ABI_VERSION 7" in hdr
    assert "SSP2_T_DIST, SSP2_T_HEAD_DIST_W, SSP2_T_HEAD_DIST_B,\n  SSP2_T_COUNT" in hdr
    assert "typedef struct {\n  int32_t prefix_tokens;\n  int32_t dist_head;\n} ssp2_vit_ext;" in hdr


def test_create_ext_refuses_bad_layouts_before_touching_the_device():
    """Every refusal is SSP2_EINVAL (-1); a valid layout reaches the device query, which fails here with SSP2_EHIP (-2) — so a -1 proves
    the refusal came first."""
    L, lib = _lib()
    d_int = (C.c_int32 * 2)(1536, 1536)
    desc = L.VitDesc(224, 16, 384, 6, 2, 10, 1e-6, 4, d_int)
    h = C.c_void_p()
    for prefix, dist_head in ((0, 0), (3, 0), (-1, 0), (1, 1), (2, 2), (2, -1), (1, 2)):
        ext = L.VitExt(prefix, dist_head)
        assert lib.ssp2_create_ext(C.byref(desc), None, C.byref(ext), C.byref(h)) == -1, (prefix, dist_head)
        assert lib.ssp2_last_error() and not h.value
    opt = (C.c_int32 * L.OPT_COUNT)(*([-1] * L.OPT_COUNT))
    opt[L.OPTIONS["attn_stream"]] = 3
    assert lib.ssp2_create_ext(C.byref(desc), opt, C.byref(L.VitExt(2, 1)), C.byref(h)) == -1
    assert lib.ssp2_create_ext(None, None, C.byref(L.VitExt(2, 1)), C.byref(h)) == -1
    if not torch.cuda.is_available():       # the valid layouts get past every check and stop at the missing device
        for ext in (None, L.VitExt(1, 0), L.VitExt(2, 0), L.VitExt(2, 1)):
            assert lib.ssp2_create_ext(C.byref(desc), None, C.byref(ext) if ext is not None else None, C.byref(h)) == -2


def test_prefix_attention_refuses_bad_arguments_before_touching_the_device():
    L, lib = _lib()
    fake = C.c_void_p(0x1000)           # never dereferenced

    def call(qkv=fake, n=2, tokens=198, heads=3, d_h=64, group=0, q=fake, out=fake, ldo=192, n_prefix=2, stream=0):
        return lib.ssp2_attention_prefix_bf16(None, qkv, n, tokens, heads, d_h, group, q, out, ldo, n_prefix, stream)

    bad = {
        "n_prefix 0": dict(n_prefix=0), "n_prefix 3": dict(n_prefix=3), "n_prefix > tokens": dict(tokens=1, d_h=16, heads=4, ldo=64),
        "stream 2": dict(stream=2), "stream -1": dict(stream=-1),
        "resident at 578 tokens": dict(tokens=578), "stream with d_h 16": dict(d_h=16, heads=4, ldo=64, tokens=6, stream=1),
        "stream above the maximum": dict(tokens=L.ATTN_STREAM_MAX_TOKENS + 1, stream=1), "d_h 80 at 198": dict(d_h=80, ldo=240),
        "ldo below dim": dict(ldo=184), "ldo not a multiple of 8": dict(ldo=196), "null qkv": dict(qkv=None), "null q": dict(q=None),
        "null out": dict(out=None), "group < 0": dict(group=-1), "n 0": dict(n=0), "heads 0": dict(heads=0), "tokens 0": dict(tokens=0),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert lib.ssp2_last_error()


# ---------------------------------------------------------------------------------------------------------- model table
def test_model_table_and_synthetic_weights():
    from ssp2vit.weights import DISTILLED, VIT_CONFIGS, n_tokens, prefix_tokens_of, synthetic_weights
    for name in ("deit_tiny_distilled_patch16_224", "deit_small_distilled_patch16_224", "deit_base_distilled_patch16_224",
                 "deit_base_distilled_patch16_384", "deit_small_distilled_patch16_224_d2", "deit_base_distilled_patch16_384_d2",
                 "deit_test_distilled_patch16_32"):
        assert name in VIT_CONFIGS and name in DISTILLED and len(VIT_CONFIGS[name]) == 6 and prefix_tokens_of(name) == 2
    assert "vit_base_patch16_224" not in DISTILLED and prefix_tokens_of("vit_base_patch16_224") == 1
    expect = {"deit_base_distilled_patch16_224": 198, "deit_base_distilled_patch16_384": 578, "deit_test_distilled_patch16_32": 6,
              "vit_base_patch16_224": 197}
    for name, tok in expect.items():
        img, patch, dim, heads, d_int, depth = VIT_CONFIGS[name]
        assert n_tokens(dict(img=img, patch=patch, prefix_tokens=prefix_tokens_of(name))) == tok, name
    w = synthetic_weights("deit_test_distilled_patch16_32", classes=7, seed=0)
    assert w["prefix_tokens"] == 2 and w["pos"].shape == (1, 6, 64) and w["dist"].shape == (1, 1, 64)
    assert w["head_dist_w"].shape == (7, 64) and w["head_dist_b"].shape == (7,)
    v = synthetic_weights("vit_test_patch16_32", classes=7, seed=0)
    assert "prefix_tokens" not in v and "dist" not in v and v["pos"].shape == (1, 5, 64)


# ------------------------------------------------------------------------------------------------------------------ ingest
def _same(a, b):
    return torch.equal(a.reshape(-1), b.reshape(-1))


def _check_flat(f, w, teacher=True):
    assert f["prefix_tokens"] == 2 and _same(f["dist"], w["dist"]) and _same(f["pos"], w["pos"]) and _same(f["cls"], w["cls"])
    assert f["img"] == w["img"] and f["patch"] == w["patch"] and f["depth"] == w["depth"] and f["classes"] == w["classes"]
    assert _same(f["head_w"], w["head_w"]) and _same(f["head_b"], w["head_b"])
    if teacher:
        assert _same(f["head_dist_w"], w["head_dist_w"]) and _same(f["head_dist_b"], w["head_dist_b"])
    else:
        assert "head_dist_w" not in f
    for i in range(int(w["depth"])):
        for k in ("qkv_w", "fc1_w", "fc2_b", "ln2_g"):
            assert _same(f[f"{k}.{i}"], w[f"{k}.{i}"]), (k, i)
    from ssp2vit.weights import n_tokens
    assert n_tokens(f) == 6


@pytest.mark.parametrize("layout,teacher", [("timm", True), ("hf", True), ("hf", False)])
def test_duck_typed_modules_and_their_state_dicts_give_the_flat_fields(layout, teacher):
    from ssp2vit.weights import from_module, from_state_dict, token_layout
    w = _w()
    m = build_distilled(w, layout, teacher)
    f = from_module(m)
    _check_flat(f, w, teacher)
    assert f["layout"] == layout and token_layout(m) == (2, int(teacher))
    sd = {k: v for k, v in m.state_dict().items()}
    g = from_state_dict(sd, {"num_attention_heads": int(w["heads"])})
    _check_flat(g, w, teacher)


@pytest.mark.parametrize("teacher", [True, False])
def test_transformers_deit_models_and_their_state_dicts(teacher):
    transformers = pytest.importorskip("transformers")
    from ssp2vit.weights import from_module, from_state_dict, token_layout
    cfg = transformers.DeiTConfig(image_size=32, patch_size=16, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                                  intermediate_size=128, num_labels=10)
    cls = transformers.DeiTForImageClassificationWithTeacher if teacher else transformers.DeiTForImageClassification
    m = cls(cfg).eval()
    f = from_module(m)
    emb = m.deit.embeddings
    assert f["prefix_tokens"] == 2 and _same(f["dist"], emb.distillation_token.detach()) and f["img"] == 32 and f["heads"] == 4
    assert f["eps"] == pytest.approx(cfg.layer_norm_eps) and token_layout(m) == (2, int(teacher))
    head = m.cls_classifier if teacher else m.classifier
    assert _same(f["head_w"], head.weight.detach())
    assert ("head_dist_w" in f) == teacher
    if teacher:
        assert _same(f["head_dist_w"], m.distillation_classifier.weight.detach())
    g = from_state_dict(m.state_dict(), cfg.to_dict())
    assert g["prefix_tokens"] == 2 and ("head_dist_w" in g) == teacher and g["img"] == 32 and g["layout"] == "hf5"
    for k in ("qkv_w.1", "fc1_w.0", "pos", "dist", "head_w"):
        assert _same(g[k], f[k]), k


def test_engine_vit_container_round_trips_the_distillation_tensors():
    from ssp2vit.modules import EngineViT
    from ssp2vit.weights import from_module, from_state_dict
    w = _w()
    m = EngineViT(w)
    assert hasattr(m, "dist_token") and hasattr(m, "head_dist")
    _check_flat(from_module(m), w)
    sd = m.state_dict()
    assert "dist_token" in sd and "head_dist.weight" in sd
    _check_flat(from_state_dict(sd, {"num_attention_heads": 4}), w)
    plain = EngineViT(_w("vit_test_patch16_32"))
    assert not hasattr(plain, "dist_token") and not hasattr(plain, "head_dist")


# ---------------------------------------------------------------------------------------------------------------- refusals
def _timm(**attrs):
    m = build_distilled(_w(), "timm")
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


@pytest.mark.parametrize("attrs,word", [
    (dict(reg_token=nn.Parameter(torch.zeros(1, 4, 64))), "reg_token"),
    (dict(num_reg_tokens=4), "reg_token"),
    (dict(no_embed_class=True), "no_embed_class"),
    (dict(global_pool="avg"), "global_pool"),
    (dict(global_pool="map"), "global_pool"),
    (dict(fc_norm=nn.LayerNorm(64)), "fc_norm"),
    (dict(num_prefix_tokens=3), "num_prefix_tokens"),
])
def test_unrepresentable_timm_layouts_are_refused_by_name(attrs, word):
    from ssp2vit.weights import from_module
    with pytest.raises(ValueError, match=word):
        from_module(_timm(**attrs))


def test_unrepresentable_checkpoints_are_refused_by_name():
    from ssp2vit.weights import from_state_dict
    sd = dict(build_distilled(_w(), "timm").state_dict())
    with pytest.raises(ValueError, match="reg_token"):
        from_state_dict({**sd, "reg_token": torch.zeros(1, 4, 64)}, {"num_attention_heads": 4})
    with pytest.raises(ValueError, match="fc_norm"):
        from_state_dict({**sd, "fc_norm.weight": torch.ones(64), "fc_norm.bias": torch.zeros(64)}, {"num_attention_heads": 4})
    with pytest.raises(ValueError, match="pos_embed"):     # position embeddings without the prefix rows (no_embed_class)
        from_state_dict({**sd, "pos_embed": torch.zeros(1, 4, 64)}, {"num_attention_heads": 4})
    nodist = {k: v for k, v in sd.items() if k != "dist_token"}
    with pytest.raises(ValueError, match="head_dist"):
        from_state_dict(nodist, {"num_attention_heads": 4})


def test_hf_register_tokens_are_refused():
    from ssp2vit.weights import from_module
    m = build_distilled(_w(), "hf")
    m.deit.embeddings.register_tokens = nn.Parameter(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError, match="register_tokens"):
        from_module(m)


def test_plain_vit_ingest_is_unchanged():
    """One prefix token: no new keys in the flat dictionary, the side from patches + 1."""
    from oracle.vit_modules import build_from_flat
    from ssp2vit.weights import from_module, token_layout
    w = _w("vit_test_patch16_32")
    for layout in ("timm", "hf"):
        m = build_from_flat(w, layout)
        f = from_module(m)
        assert "prefix_tokens" not in f and "dist" not in f and "head_dist_w" not in f and f["img"] == 32
        assert token_layout(m) == (1, 0)


# ------------------------------------------------------------------------------------------- the reference's outputs (goldens)
GOLDEN_CASES = [(tag, layout) for tag in ("deit_test", "deit_s16") for layout in ("timm", "hf")]


@pytest.mark.parametrize("tag,layout", GOLDEN_CASES)
def test_cpu_restatement_reproduces_the_reference_goldens_bit_for_bit(tag, layout):
    """tests/golden/make_golden_deit.py ran the REAL reference on the distilled duck modules; the CPU restatement (oracle/ref_cpu.py on the
    same modules) reproduces its bf16 stage-1 scores, autocast logits, top-1, depth importances (with every bypassed model's logits), the
    masks at the stored plan and the K selection, bit for bit."""
    import numpy as np
    from deit_models import DEIT_GOLDEN_CASES, bf16_from_bits, load_golden
    from oracle import ref_cpu
    w, batches, z = load_golden(tag, layout)
    model = build_distilled(w, layout, teacher=True)
    depth = int(w["depth"])
    _, _, _, t, min_rem, K, _ = DEIT_GOLDEN_CASES[tag]
    for i, b in enumerate(batches):
        assert torch.equal(ref_cpu.logits_of(model, b["pixel_values"]), bf16_from_bits(z[f"logits_bf16bits.{i}"])), i
    imps = ref_cpu.ffn_activation_importance(model, batches)
    for l, s in enumerate(imps):
        assert torch.equal(s, bf16_from_bits(z[f"s1_imp_bf16bits.{l}"])), l
    assert ref_cpu.evaluate_top1(model, batches) == float(z["top1"])
    att = ref_cpu.att_depth_importance(model, batches)
    assert torch.equal(att, torch.from_numpy(z["att_imp"]))
    for blk in range(depth):
        trial = copy.deepcopy(model)
        ref_cpu.bypass_attention_(trial, blk)
        for i, b in enumerate(batches):
            assert torch.equal(ref_cpu.logits_of(trial, b["pixel_values"]), bf16_from_bits(z[f"bypass_logits_bf16bits.{blk}.{i}"])), (blk, i)
    masks, _ = ref_cpu.width_prune_selection([s.to(torch.float32) for s in imps], [t] * depth, min_remaining=min_rem)
    assert np.array_equal(np.packbits(np.asarray(masks, dtype=np.uint8), axis=1), z[f"mask.t{t}"])
    assert ref_cpu.select_blocks_torch_argsort(att, K) == z[f"s2_selected_k{K}"].tolist()
