"""Register tokens and class-free positions (timm reg_token / no_embed_class: DeiT-III, DINOv2-reg), the parts that need no GPU: the
CPU restatement of tests/regtoken_models.py against the real reference's fixtures bit for bit, the loaders (live module, state dict,
export round trip), the state dict's inference of no_embed_class and its ambiguity error, every refusal by name, the planner and
parameter counts, and the additive C ABI (new symbols, ABI still 7, argument refusals before the device is touched)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import PKG
from regtoken_models import REG_GOLDEN_CASES, bf16_from_bits, build_regtoken, embed_tokens, load_golden, weak_neurons

NEW_NAMES = {  # name -> (tokens, register tokens, class-free positions, LayerScale)
    "deit3_small_patch16_224": (197, 0, True, True), "deit3_base_patch16_224": (197, 0, True, True),
    "deit3_large_patch16_224": (197, 0, True, True), "deit3_base_patch16_384": (577, 0, True, True),
    "vit_small_patch14_reg4_dinov2": (1374, 4, True, True), "vit_base_patch14_reg4_dinov2": (1374, 4, True, True),
    "vit_large_patch14_reg4_dinov2": (1374, 4, True, True), "vit_small_patch14_reg4_dinov2_224": (261, 4, True, True),
    "vit_base_patch14_reg4_dinov2_224": (261, 4, True, True), "vit_large_patch14_reg4_dinov2_224": (261, 4, True, True),
    "vit_test_patch16_32_reg4": (9, 4, True, True), "vit_test_patch16_32_reg2_pe": (7, 2, False, False),
    "deit3_small_patch16_224_d2": (197, 0, True, True), "vit_small_patch14_reg4_dinov2_224_d2": (261, 4, True, True),
    "vit_small_patch14_reg4_dinov2_d2": (1374, 4, True, True),
}


def _lib():
    from ssp2vit import _lib
    return _lib, _lib.load()


def _w(name="vit_test_patch16_32_reg4", **kw):
    from ssp2vit.weights import synthetic_weights
    return synthetic_weights(name, classes=10, seed=1, **kw)


def _same(a, b):
    return torch.equal(a.reshape(-1).cpu(), b.reshape(-1).cpu())


def _check_flat(f, w):
    for k, v in w.items():
        if isinstance(v, torch.Tensor):
            assert _same(f[k], v), k
    for k in ("img", "patch", "dim", "heads", "depth", "classes"):
        assert int(f[k]) == int(w[k]), k
    assert int(f.get("prefix_tokens", 1)) == int(w.get("prefix_tokens", 1))
    assert bool(f.get("no_embed_class", False)) == bool(w.get("no_embed_class", False))
    assert ("reg" in f) == ("reg" in w) and ("dist" not in f)
    assert sorted(k for k in f if k.startswith("ls")) == sorted(k for k in w if k.startswith("ls"))


# ------------------------------------------------------------------------------------- the reference's outputs (fixtures)
@pytest.fixture
def eight_threads():
    """The fixtures were captured with torch.set_num_threads(8): the CPU GEMMs' reduction order depends on the thread count."""
    before = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(before)


@pytest.mark.parametrize("tag", list(REG_GOLDEN_CASES))
def test_cpu_restatement_reproduces_the_reference_fixtures_bit_for_bit(tag, eight_threads):
    """tests/golden/make_golden_regtokens.py ran the REAL reference on the duck module; the CPU restatement (oracle/ref_cpu.py on the
    same module) reproduces its bf16 stage-1 scores (summed over all tokens, registers included), autocast logits (row 0), top-1, depth
    importances with every bypassed model's logits, the masks at the stored plan and the K selection, bit for bit."""
    from oracle import ref_cpu
    from ssp2vit.mask_parity import mask_parity_report
    w, batches, z = load_golden(tag)
    model = build_regtoken(w)
    depth = int(w["depth"])
    t, min_rem, K = REG_GOLDEN_CASES[tag][3:6]
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
    rep = mask_parity_report([bf16_from_bits(z[f"s1_imp_bf16bits.{l}"]).float() for l in range(depth)], [t] * depth, min_rem, eps=2.0 ** -5)
    assert rep["blocks_guaranteed"] == depth, rep
    for l in range(depth):
        assert torch.equal(torch.nonzero(torch.as_tensor(masks[l])).view(-1), weak_neurons(tag, l)), l


def test_the_module_embeds_as_the_statement_says_and_the_layout_matters():
    """The duck module's _pos_embed equals the host statement (embed_tokens) in both position forms; a shifted position row / reversed
    registers give other logits than the stored ones."""
    from oracle import ref_cpu
    for tag in ("reg_test4", "reg_test2pe"):
        w, batches, z = load_golden(tag)
        m = build_regtoken(w)
        px = batches[0]["pixel_values"]
        with torch.no_grad(), torch.autocast("cpu"):
            y = m.patch_embed(px)
            assert y.dtype == torch.bfloat16
            x = m._pos_embed(y)
        assert x.dtype == torch.float32 and torch.equal(x, embed_tokens(w, y.float()))
        P = int(w["prefix_tokens"])
        assert x.shape[1] == 4 + P
        if w.get("no_embed_class"):
            assert torch.equal(x[0, :P], torch.cat([w["cls"].view(1, -1), w["reg"].view(P - 1, -1)]))
        # (registers without position rows are interchangeable for the CLS logits: there the planted defect is a shifted position row;
        # with positions for every token it is the registers in reversed order)
        planted = dict(w, pos=w["pos"].roll(1, 1)) if w.get("no_embed_class") else dict(w, reg=w["reg"].flip(1))
        assert not torch.equal(ref_cpu.logits_of(build_regtoken(planted), px), bf16_from_bits(z["logits_bf16bits.0"]))


# ---------------------------------------------------------------------------------------------------------------- loaders
def test_model_table_and_synthetic_registers():
    from ssp2vit.weights import (DISTILLED, LAYER_SCALE, NO_EMBED_CLASS, REG_TOKENS, VIT_CONFIGS, check_flat_layout, n_tokens,
                                 prefix_tokens_of, synthetic_weights)
    for name, (tok, regs, nec, ls) in NEW_NAMES.items():
        assert name in VIT_CONFIGS and len(VIT_CONFIGS[name]) == 6 and name not in DISTILLED
        assert (REG_TOKENS.get(name, 0), name in NO_EMBED_CLASS, name in LAYER_SCALE) == (regs, nec, ls), name
        img, patch = VIT_CONFIGS[name][:2]
        assert prefix_tokens_of(name) == 1 + regs and n_tokens(dict(img=img, patch=patch, prefix_tokens=1 + regs)) == tok, name
    # present names keep their answers
    assert prefix_tokens_of("vit_base_patch16_224") == 1 and prefix_tokens_of("deit_base_distilled_patch16_224") == 2
    assert "vit_base_patch16_224" not in NO_EMBED_CLASS and "vit_small_patch14_dinov2" not in REG_TOKENS
    assert "vit_base_patch16_224" not in LAYER_SCALE and "deit_base_distilled_patch16_224" not in LAYER_SCALE
    w = _w()
    assert w["prefix_tokens"] == 5 and w["no_embed_class"] is True and w["reg"].shape == (1, 4, 64) and w["pos"].shape == (1, 4, 64)
    assert n_tokens(w) == 9 and check_flat_layout(w) == (5, 4, True) and "ls1.0" in w
    pe = _w("vit_test_patch16_32_reg2_pe")
    assert pe["prefix_tokens"] == 3 and "no_embed_class" not in pe and pe["reg"].shape == (1, 2, 64) and pe["pos"].shape == (1, 7, 64)
    assert check_flat_layout(pe) == (3, 2, False) and "ls1.0" not in pe
    d3 = _w("deit3_small_patch16_224_d2")
    assert "reg" not in d3 and "prefix_tokens" not in d3 and d3["no_embed_class"] is True and d3["pos"].shape == (1, 196, 384)
    # the registers come from a generator of their own: the plain test model's tensors are drawn as before, and with the same pos shape
    # (reg2_pe has 7 rows: other draws) every tensor in front of pos is the same
    plain = synthetic_weights("vit_test_patch16_32", classes=10, seed=1)
    assert _same(pe["patch_w"], plain["patch_w"]) and _same(pe["cls"], plain["cls"])
    assert w["reg"].unique().numel() == w["reg"].numel()


@pytest.mark.parametrize("name", ["vit_test_patch16_32_reg4", "vit_test_patch16_32_reg2_pe", "deit3_small_patch16_224_d2"])
def test_from_module_state_dict_and_container_give_the_same_flat_dictionary(name, tmp_path):
    from ssp2vit import export
    from ssp2vit.modules import EngineViT
    from ssp2vit.weights import count_params, from_module, from_state_dict, load_checkpoint, position_layout, token_layout
    w = _w(name)
    heads = {"num_attention_heads": int(w["heads"])}
    m = build_regtoken(w)
    regs = int(w["reg"].shape[1]) if "reg" in w else 0
    assert token_layout(m) == (1, 0) and position_layout(m) == (regs, bool(w.get("no_embed_class", False)))
    f = from_module(m)
    _check_flat(f, w)
    assert f["layout"] == "timm" and count_params(f) == sum(p.numel() for p in m.parameters())
    sd = dict(m.state_dict())
    assert ("reg_token" in sd) == bool(regs)
    cfg = dict(heads, img_size=int(w["img"])) if name != "deit3_small_patch16_224_d2" else heads      # 196 rows are unambiguous
    _check_flat(from_state_dict(sd, cfg), w)
    e = EngineViT(w)
    assert e.no_embed_class == bool(w.get("no_embed_class", False)) and e.num_prefix_tokens == 1 + regs and e.num_reg_tokens == regs
    assert e.global_pool == "token" and hasattr(e, "reg_token") == bool(regs)
    _check_flat(from_module(e), w)
    assert position_layout(e) == position_layout(m) and token_layout(e) == (1, 0)
    for saver in (lambda: export.save_pretrained_dir(e, str(tmp_path / "hf")), lambda: export.save_timm_state_dict(e, tmp_path, "timm")):
        back = load_checkpoint(saver())
        _check_flat(back, w)


def test_state_dict_inference_on_the_real_row_counts_and_the_ambiguity():
    """196 / 576 rows (DeiT-III at 224 / 384) and 256 / 1369 rows with four registers (DINOv2-reg at 224 / 518) read class-free; 197, 577,
    257 and 1370 rows with the prefix rows; 9 rows with four registers read both ways and need the config."""
    from ssp2vit.weights import _infer_no_embed_class, from_state_dict
    p16, p14 = torch.zeros(8, 3, 16, 16), torch.zeros(8, 3, 14, 14)
    reg4 = torch.zeros(1, 4, 8)

    def infer(rows, patch_w, reg=None, config=None, dist=False):
        w = {"pos": torch.zeros(1, rows, 8), "patch_w": patch_w}
        if reg is not None:
            w["reg"], w["prefix_tokens"] = reg, 1 + reg.shape[1]
        if dist:
            w["dist"], w["prefix_tokens"] = torch.zeros(1, 1, 8), 2
        return _infer_no_embed_class(w, dict(config or {}), {})
    for rows, pw, reg, want in ((196, p16, None, True), (576, p16, None, True), (197, p16, None, False), (577, p16, None, False),
                                (256, p14, reg4, True), (1369, p14, reg4, True), (257, p14, None, False), (1370, p14, None, False),
                                (261, p14, reg4, False), (1374, p14, reg4, False)):
        assert infer(rows, pw, reg) is want, rows
    assert infer(198, p16, dist=True) is False
    with pytest.raises(ValueError, match=r"pos_embed.*no_embed_class.*prefix"):
        infer(9, p16, reg4)
    with pytest.raises(ValueError, match="pos_embed"):
        infer(25, p16, torch.zeros(1, 8, 8))
    assert infer(9, p16, reg4, {"img_size": 48}) is True and infer(9, p16, reg4, {"image_size": 32}) is False
    assert infer(9, p16, reg4, {"no_embed_class": True}) is True and infer(9, p16, reg4, {"no_embed_class": False}) is False
    with pytest.raises(ValueError, match="pos_embed"):
        infer(9, p16, reg4, {"img_size": 64})
    with pytest.raises(ValueError, match="pos_embed"):
        infer(197, p16, None, {"no_embed_class": True})
    # through from_state_dict: the 9-token cut is the ambiguous one
    w = _w()
    sd = dict(build_regtoken(w).state_dict())
    # 4 rows with P = 5: only the class-free reading holds
    assert from_state_dict(sd, {"num_attention_heads": 4})["no_embed_class"] is True
    w9 = dict(w, img=48, pos=torch.zeros(1, 9, 64))
    sd9 = dict(build_regtoken(w9).state_dict())
    with pytest.raises(ValueError, match=r"pos_embed.*no_embed_class"):
        from_state_dict(sd9, {"num_attention_heads": 4})
    f = from_state_dict(sd9, {"num_attention_heads": 4, "img_size": 48})
    assert f["no_embed_class"] is True and f["img"] == 48
    g = from_state_dict(sd9, {"num_attention_heads": 4, "image_size": 32})
    assert "no_embed_class" not in g and g["img"] == 32 and g["prefix_tokens"] == 5


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_their_attribute():
    from deit_models import build_distilled
    from ssp2vit.weights import check_flat_layout, from_module, from_state_dict, synthetic_weights
    dw = synthetic_weights("deit_test_distilled_patch16_32", classes=10, seed=1)

    def distilled(**attrs):
        m = build_distilled(dw, "timm")
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    with pytest.raises(ValueError, match="reg_token"):                 # registers beside a dist_token
        from_module(distilled(reg_token=nn.Parameter(torch.zeros(1, 4, 64)), num_prefix_tokens=6))
    with pytest.raises(ValueError, match="no_embed_class"):            # class-free positions beside a dist_token
        from_module(distilled(no_embed_class=True))
    with pytest.raises(ValueError, match="reg_token"):                 # num_reg_tokens without the parameter
        from_module(distilled(num_reg_tokens=4))
    w = _w()
    m = build_regtoken(w)
    m.num_reg_tokens = 3
    with pytest.raises(ValueError, match="reg_token"):                 # ... or disagreeing with it
        from_module(m)
    m = build_regtoken(w)
    m.num_prefix_tokens = 1
    with pytest.raises(ValueError, match="num_prefix_tokens"):
        from_module(m)
    m = build_regtoken(w)
    m.pos_embed = nn.Parameter(torch.zeros(1, 5, 64))
    with pytest.raises(ValueError, match="no_embed_class"):            # class-free, but pos_embed is no square number of rows
        from_module(m)
    m = build_regtoken(_w("vit_test_patch16_32_reg2_pe"))
    m.pos_embed = nn.Parameter(torch.zeros(1, 6, 64))
    with pytest.raises(ValueError, match="pos_embed"):                 # rows fit neither reading
        from_module(m)
    m = build_regtoken(w)
    m.reg_token = nn.Parameter(torch.zeros(1, 9, 64)); m.num_reg_tokens = 9; m.num_prefix_tokens = 10
    with pytest.raises(ValueError, match="reg_token"):                 # more than 8 registers
        from_module(m)
    m = build_regtoken(w)
    m.reg_token = nn.Parameter(torch.zeros(1, 4, 32))
    with pytest.raises(ValueError, match="reg_token"):
        from_module(m)
    for attrs, word in ((dict(global_pool="avg"), "global_pool"), (dict(fc_norm=nn.LayerNorm(64)), "fc_norm")):      # pooled heads stay refused
        m = build_regtoken(w)
        for k, v in attrs.items():
            setattr(m, k, v)
        with pytest.raises(ValueError, match=word):
            from_module(m)
    # state dicts
    dsd = dict(build_distilled(dw, "timm").state_dict())
    with pytest.raises(ValueError, match="reg_token"):
        from_state_dict({**dsd, "reg_token": torch.zeros(1, 4, 64)}, {"num_attention_heads": 4})
    with pytest.raises(ValueError, match="pos_embed"):
        from_state_dict({**dsd, "pos_embed": torch.zeros(1, 4, 64)}, {"num_attention_heads": 4})
    sd = dict(build_regtoken(w).state_dict())
    with pytest.raises(ValueError, match="pos_embed"):
        from_state_dict({**sd, "pos_embed": torch.zeros(1, 7, 64)}, {"num_attention_heads": 4})
    with pytest.raises(ValueError, match="reg_token"):
        from_state_dict({**sd, "reg_token": torch.zeros(1, 9, 64)}, {"num_attention_heads": 4})
    with pytest.raises(ValueError, match="fc_norm"):
        from_state_dict({**sd, "fc_norm.weight": torch.ones(64), "fc_norm.bias": torch.zeros(64)}, {"num_attention_heads": 4})
    # HF register tokens stay refused
    hf = build_distilled(dw, "hf")
    hf.deit.embeddings.register_tokens = nn.Parameter(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError, match="register_tokens"):
        from_module(hf)
    # the flat dictionary's own validation
    with pytest.raises(ValueError, match="no_embed_class"):
        check_flat_layout(dict(w, no_embed_class=False))
    with pytest.raises(ValueError, match="prefix_tokens"):
        check_flat_layout(dict(w, prefix_tokens=4))
    with pytest.raises(ValueError, match="reg"):
        check_flat_layout(dict(w, reg=torch.zeros(1, 9, 64), prefix_tokens=10))
    with pytest.raises(ValueError, match="dist"):
        check_flat_layout(dict(w, dist=torch.zeros(1, 1, 64)))


def test_engine_reads_the_layout_from_the_dictionary_and_refuses_bad_shapes_by_name():
    from ssp2vit.engine import VitEngine
    assert VitEngine._position_layout_of(_w()) == (4, True)
    assert VitEngine._position_layout_of(_w("vit_test_patch16_32_reg2_pe")) == (2, False)
    assert VitEngine._position_layout_of(_w("vit_test_patch16_32")) == (0, False)
    with pytest.raises(ValueError, match="reg"):
        VitEngine._position_layout_of(dict(_w(), reg=torch.zeros(1, 4, 32)))


# ---------------------------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("tag", list(REG_GOLDEN_CASES))
def test_planner_and_parameter_counts_equal_the_reference(tag):
    """reg_token and the (shorter) pos_embed are in model.parameters() and in no attention count: the reference's planner,
    count_total_params and per-block counts on the duck module, on the rebuilt container and from the shapes equal the stored answers."""
    from ssp2vit import vit_pruning as vp
    from ssp2vit.modules import EngineViT
    from ssp2vit.planner import plan_from_stats, stats_from_shapes
    from ssp2vit.weights import count_params, n_tokens, reg_tokens_of
    w, _, z = load_golden(tag)
    min_rem = REG_GOLDEN_CASES[tag][4]
    duck = build_regtoken(w)
    assert int(z["total_params"]) == sum(p.numel() for p in duck.parameters())
    for model in (duck, EngineViT(w)):
        assert vp.count_total_params(model) == int(z["total_params"])
        st = vp._model_stats(model)
        assert st.attn_params == z["attn_params"].tolist() and st.ffn_params == z["ffn_params"].tolist()
        for s, (k, t, err) in zip(z["plan_targets"], z["plan_k_t_err"].tolist()):
            p = vp.plan_2ssp_allocation(model, float(s), min_rem)
            assert (p.blocks_to_prune, p.per_block_neurons_to_prune, p.est_error_params) == (k, t, err), (tag, s)
    assert count_params(w) == int(z["total_params"])
    st = stats_from_shapes(int(w["dim"]), int(w["depth"]), int(w["fc1_w.0"].shape[0]), 10, n_tokens(w), int(w["patch"]),
                           layer_scale=2 if "ls1.0" in w else 0, reg_tokens=reg_tokens_of(w), no_embed_class=bool(w.get("no_embed_class", False)))
    assert st.total_params == int(z["total_params"]) and st.attn_params == z["attn_params"].tolist()
    for s, (k, t, err) in zip(z["plan_targets"], z["plan_k_t_err"].tolist()):
        p = plan_from_stats(st, float(s), min_rem)
        assert (p.blocks_to_prune, p.per_block_neurons_to_prune, p.est_error_params) == (k, t, err), (tag, s)
    # the defaults leave the answers as they were
    assert stats_from_shapes(768, 12, 3072, 1000, 197, 16).total_params == stats_from_shapes(768, 12, 3072, 1000, 197, 16, reg_tokens=0, no_embed_class=False).total_params == 86567656


# -------------------------------------------------------------------------------------------------------------------- ABI
def _desc(L, img=32, patch=16, dim=64, heads=4, depth=1):
    arr = (C.c_int32 * depth)(*([128] * depth))
    return L.VitDesc(img, patch, dim, heads, depth, 10, 1e-6, 8, arr), arr


def test_new_entries_are_exported_and_the_abi_stays_7():
    L, lib = _lib()
    assert L.ABI_VERSION == 7 and lib.ssp2_abi_version() == 7
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "ssp2vit.h")).read()
    for name in ("ssp2_create_layout", "ssp2_set_reg_tokens"):
        assert name in L.SYMBOLS and hasattr(lib, name) and f"int {name}(" in hdr
    assert "#define SSP2_ABI_VERSION 7" in hdr
    assert "typedef struct {\n  int32_t prefix_tokens;\n  int32_t dist_head;\n  int32_t reg_tokens;\n  int32_t pos_prefix_rows;\n} ssp2_token_layout;" in hdr
    assert "typedef struct {\n  int32_t prefix_tokens;\n  int32_t dist_head;\n} ssp2_vit_ext;" in hdr
    assert L.T_KINDS[-3:] == ["dist", "head_dist_w", "head_dist_b"] and len(L.T_KINDS) == 23          # no new tensor kinds
    assert L.OPT_COUNT == 14 and L.EXT_OPTIONS == {"stream_fp8": 14} and L.OPT_END == 15             # no new options
    assert C.sizeof(L.TokenLayout) == 16 and C.sizeof(L.VitExt) == 8


def test_create_layout_refuses_bad_layouts_before_the_device_and_names_the_field():
    """SSP2_EINVAL (-1) with the field in the message for every refusal of the issue; a valid layout gets as far as the device
    (SSP2_EHIP = -2 without one; with one the engine is created and destroyed again).  ssp2_create_ext answers as before."""
    L, lib = _lib()
    desc, _keep = _desc(L)
    h = C.c_void_p()
    has_gpu = torch.cuda.is_available()

    def ok(rc):
        if has_gpu and rc == 0:
            return lib.ssp2_destroy(h) == 0
        return not has_gpu and rc == -2

    def create(prefix, dist_head, regs, pos_rows, d=desc):
        return lib.ssp2_create_layout(C.byref(d), None, C.byref(L.TokenLayout(prefix, dist_head, regs, pos_rows)), C.byref(h))
    bad = [((10, 0, 9, 0), "reg_tokens"), ((0, 0, -1, 1), "reg_tokens"), ((1, 0, 4, 0), "prefix_tokens"), ((6, 0, 4, 1), "prefix_tokens"),
           ((0, 0, 0, 1), "prefix_tokens"), ((3, 0, 0, 1), "prefix_tokens"), ((-1, 0, 0, 1), "prefix_tokens"), ((2, 1, 1, 1), "dist_head"),
           ((5, 1, 4, 0), "dist_head"), ((2, 1, 0, 0), "pos_prefix_rows"), ((2, 0, 0, 0), "pos_prefix_rows"), ((5, 0, 4, 2), "pos_prefix_rows"),
           ((5, 0, 4, -1), "pos_prefix_rows"), ((1, 2, 0, 1), "dist_head"), ((1, 1, 0, 1), "dist_head")]
    for args, word in bad:
        assert create(*args) == -1, args
        assert word in lib.ssp2_last_error().decode(), (args, lib.ssp2_last_error())
    assert lib.ssp2_create_layout(None, None, C.byref(L.TokenLayout(5, 0, 4, 0)), C.byref(h)) == -1
    # a token count without an attention kernel: the existing messages (d_h 16 takes up to 32 tokens; 36 + 5 = 41)
    big, _k2 = _desc(L, img=96)
    assert create(5, 0, 4, 0, big) == -1 and "no attention kernel for head dim 16 with 41 tokens" in lib.ssp2_last_error().decode()
    long_, _k3 = _desc(L, img=518, patch=14, dim=384, heads=6)
    assert create(5, 0, 4, 0, long_) == -1 and "SSP2_OPT_ATTN_STREAM = 1" in lib.ssp2_last_error().decode() and "1374 tokens" in lib.ssp2_last_error().decode()
    for args in ((5, 0, 4, 0), (9, 0, 8, 0), (3, 0, 2, 1), (1, 0, 0, 0), (1, 0, 0, 1), (2, 1, 0, 1), (2, 0, 0, 1), (2, 0, 1, 1), (2, 0, 1, 0)):
        assert ok(create(*args)), args                                  # valid: the only refusal left is "no HIP device"
    assert ok(lib.ssp2_create_layout(C.byref(desc), None, None, C.byref(h)))
    # ssp2_create_ext and its struct behave as before
    for prefix, dist_head in ((0, 0), (3, 0), (-1, 0), (1, 1), (2, 2), (2, -1), (1, 2)):
        assert lib.ssp2_create_ext(C.byref(desc), None, C.byref(L.VitExt(prefix, dist_head)), C.byref(h)) == -1, (prefix, dist_head)
    for ext in (None, L.VitExt(1, 0), L.VitExt(2, 0), L.VitExt(2, 1)):
        assert ok(lib.ssp2_create_ext(C.byref(desc), None, C.byref(ext) if ext is not None else None, C.byref(h)))


def test_set_reg_tokens_refuses_a_null_handle():
    """(The refusals that need a live handle — count, null pointer, ESTATE of ssp2_embed — are in tests/test_regtokens_gpu.py.)"""
    L, lib = _lib()
    assert lib.ssp2_set_reg_tokens(None, C.c_void_p(0x1000), 4, 0) == -1 and lib.ssp2_last_error()
