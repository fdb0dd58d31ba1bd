"""LayerScale (timm Block.ls1 / ls2), the parts that need no GPU: the CPU restatement of tests/layerscale_models.py against the real
reference's fixtures bit for bit, the loaders (live module, state dict, export round trip) and their refusals by name, the planner and
parameter counts against the reference's stored answers, the additive C ABI (new symbols, ABI still 7) and the argument refusals of
the new entries before the device is touched."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import PKG
from layerscale_models import LS_GOLDEN_CASES, LayerScale, bf16_from_bits, build_layerscale, load_golden


def _lib():
    from ssp2vit import _lib
    return _lib, _lib.load()


def _w(name="vit_test_patch16_32_ls", **kw):
    from ssp2vit.weights import synthetic_weights
    return synthetic_weights(name, classes=10, seed=1, **kw)


# ------------------------------------------------------------------------------------------------------------- arithmetic
def test_autocast_layerscale_is_a_product_and_a_sum_not_a_fused_multiply_add():
    """What the epilogue must reproduce: under CPU autocast the branch output is bf16, gamma fp32 — x + ls(y) equals x + y.float() * gamma
    bit for bit (two fp32 roundings), and the fused form (one rounding) gives other bits on some elements."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 320, generator=g)
    y = torch.randn(64, 320, generator=g).to(torch.bfloat16)
    ls = LayerScale(320)
    with torch.no_grad():
        ls.gamma.copy_(torch.randn(320, generator=g))
        with torch.autocast("cpu"):
            got = x + ls(y)
        assert got.dtype == torch.float32
        assert torch.equal(got, x + y.float() * ls.gamma)
        fused = (x.double() + y.double() * ls.gamma.double()).float()       # the product is exact in float64: one rounding, as an fma
        assert not torch.equal(got, fused)


# ------------------------------------------------------------------------------------- the reference's outputs (fixtures)
@pytest.fixture
def eight_threads():
    """The fixtures were captured with torch.set_num_threads(8) (make_golden_layerscale.py): the CPU GEMMs' reduction order, and so the
    last bits of the bf16 chain, depend on the thread count — other tests of the suite leave it at 1 or 2."""
    before = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(before)


@pytest.mark.parametrize("tag", list(LS_GOLDEN_CASES))
def test_cpu_restatement_reproduces_the_reference_fixtures_bit_for_bit(tag, eight_threads):
    """tests/golden/make_golden_layerscale.py ran the REAL reference on the LayerScale duck module; the CPU restatement (oracle/ref_cpu.py
    on the same module) reproduces its bf16 stage-1 scores, autocast logits, top-1, depth importances (with every bypassed model's
    logits), the masks at the stored plan and the K selection, bit for bit."""
    from oracle import ref_cpu
    w, batches, z = load_golden(tag)
    model = build_layerscale(w)
    depth = int(w["depth"])
    t, min_rem, K = LS_GOLDEN_CASES[tag][3:6]
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
    # the cut is decisive in every block (the fixtures' weak neurons): the reference's masks are exactly those neurons
    from layerscale_models import weak_neurons
    from ssp2vit.mask_parity import mask_parity_report
    rep = mask_parity_report([bf16_from_bits(z[f"s1_imp_bf16bits.{l}"]).float() for l in range(depth)], [t] * depth, min_rem, eps=2.0 ** -5)
    assert rep["blocks_guaranteed"] == depth, rep
    for l in range(depth):
        assert torch.equal(torch.nonzero(torch.as_tensor(masks[l])).view(-1), weak_neurons(tag, l)), l


def test_the_scales_matter_and_a_bypassed_block_returns_x_exactly():
    """The fixtures' gammas are far from 1: the same weights without them give other logits; a block whose attention is bypassed adds
    ls1(0) = 0, i.e. x comes through its attention half exactly."""
    from oracle import ref_cpu
    w, batches, z = load_golden("ls_test")
    px = batches[0]["pixel_values"]
    plain = {k: v for k, v in w.items() if not k.startswith(("ls1.", "ls2."))}
    assert not torch.equal(ref_cpu.logits_of(build_layerscale(plain), px), bf16_from_bits(z["logits_bf16bits.0"]))
    m = build_layerscale(w)
    blk = m.blocks[1]
    ref_cpu.bypass_attention_(m, 1)
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad(), torch.autocast("cpu"):
        half = x + blk.ls1(blk.attn(blk.norm1(x)))
    assert torch.equal(half, x)


# ---------------------------------------------------------------------------------------------------------------- loaders
def _same(a, b):
    return torch.equal(a.reshape(-1).cpu(), b.reshape(-1).cpu())


def test_model_table_and_synthetic_layer_scales():
    from ssp2vit.weights import LAYER_SCALE, VIT_CONFIGS, n_tokens, synthetic_weights
    for name, tok in (("vit_small_patch14_dinov2", 1370), ("vit_base_patch14_dinov2", 1370), ("vit_large_patch14_dinov2", 1370),
                      ("vit_small_patch14_dinov2_224", 257), ("vit_small_patch14_dinov2_d2", 1370), ("vit_small_patch16_224_ls_d2", 197),
                      ("vit_test_patch16_32_ls", 5)):
        assert name in VIT_CONFIGS and name in LAYER_SCALE
        img, patch = VIT_CONFIGS[name][:2]
        assert n_tokens(dict(img=img, patch=patch)) == tok, name
    assert "vit_base_patch16_224" not in LAYER_SCALE and "deit_base_distilled_patch16_224" not in LAYER_SCALE
    w = _w()
    plain = synthetic_weights("vit_test_patch16_32_ls", classes=10, seed=1, layer_scale=False)
    assert not any(k.startswith("ls") for k in plain)
    assert all(_same(w[k], v) for k, v in plain.items() if isinstance(v, torch.Tensor))          # the other tensors do not move
    assert any(k.startswith("ls1.") for k in synthetic_weights("vit_test_patch16_32", classes=10, seed=1, layer_scale=True))
    g = torch.cat([w[f"{k}.{i}"] for k in ("ls1", "ls2") for i in range(4)])
    assert g.numel() == 8 * 64 and float(g.abs().min()) >= 1e-3 and float(g.abs().max()) <= 2.0
    assert 0.15 <= float((g < 0).float().mean()) <= 0.35 and g.unique().numel() == g.numel()


def test_from_module_and_from_state_dict_round_trip_the_gammas():
    from ssp2vit.weights import count_params, from_module, from_state_dict, has_layer_scale
    w = _w()
    m = build_layerscale(w)
    f = from_module(m)
    g = from_state_dict(dict(m.state_dict()), {"num_attention_heads": 4})
    for flat in (f, g):
        for i in range(4):
            assert _same(flat[f"ls1.{i}"], w[f"ls1.{i}"]) and _same(flat[f"ls2.{i}"], w[f"ls2.{i}"]), i
            assert flat[f"ls1.{i}"].dtype == torch.float32 and _same(flat[f"fc1_w.{i}"], w[f"fc1_w.{i}"])
        assert flat["layout"] == "timm" and "prefix_tokens" not in flat
    assert has_layer_scale(m) == ((True, True),) * 4
    assert count_params(f) == sum(p.numel() for p in m.parameters())          # the gammas count, as in the reference's model.parameters()


def test_identity_and_mixed_branches():
    """nn.Identity (timm init_values=None) or an absent attribute means none: no ls* keys; a model with ls1 only keeps only those."""
    from oracle.vit_modules import build_from_flat
    from ssp2vit.weights import from_module, from_state_dict, has_layer_scale
    w = _w()
    plain = {k: v for k, v in w.items() if not k.startswith(("ls1.", "ls2."))}
    m = build_layerscale(plain)                                    # ls1 / ls2 = nn.Identity
    assert isinstance(m.blocks[0].ls1, nn.Identity)
    for flat in (from_module(m), from_state_dict(dict(m.state_dict()), {"num_attention_heads": 4}), from_module(build_from_flat(plain, "timm"))):
        assert not any(k.startswith(("ls1.", "ls2.")) for k in flat)
    assert has_layer_scale(m) == ((False, False),) * 4
    only1 = {k: v for k, v in w.items() if not k.startswith("ls2.") and k != "ls1.2"}
    f = from_module(build_layerscale(only1))
    assert sorted(k for k in f if k.startswith("ls")) == ["ls1.0", "ls1.1", "ls1.3"]


def test_refusals_name_their_attribute():
    from deit_models import build_distilled
    from oracle.vit_modules import build_from_flat
    from ssp2vit.weights import from_module, from_state_dict, synthetic_weights
    w = _w()
    m = build_layerscale(w)
    m.blocks[2].ls2.inplace = True                                  # x.mul_(gamma): the product is rounded to bf16
    with pytest.raises(ValueError, match=r"blocks\[2\]\.ls2\.inplace"):
        from_module(m)
    m = build_layerscale(w)
    m.blocks[1].ls1.gamma = nn.Parameter(torch.ones(32))
    with pytest.raises(ValueError, match=r"blocks\[1\]\.ls1\.gamma"):
        from_module(m)
    sd = dict(build_layerscale(w).state_dict())
    with pytest.raises(ValueError, match=r"blocks\.3\.ls1\.gamma"):
        from_state_dict({**sd, "blocks.3.ls1.gamma": torch.ones(65)}, {"num_attention_heads": 4})
    # HF DINOv2: layer_scale1.lambda1 / layer_scale2.lambda1, as keys and as modules
    plain = synthetic_weights("vit_test_patch16_32", classes=10, seed=1)
    hf = build_from_flat(plain, "hf")
    hsd = dict(hf.state_dict())
    key = next(k for k in hsd if k.endswith("layernorm_before.weight")).replace("layernorm_before.weight", "layer_scale1.lambda1")
    with pytest.raises(ValueError, match=r"layer_scale1\.lambda1"):
        from_state_dict({**hsd, key: torch.ones(64)}, {"num_attention_heads": 4})
    with pytest.raises(ValueError, match=r"layer_scale2\.lambda1"):
        from_state_dict({**hsd, key.replace("layer_scale1", "layer_scale2"): torch.ones(64)}, {"num_attention_heads": 4})

    class _HfLs(nn.Module):
        def __init__(self):
            super().__init__()
            self.lambda1 = nn.Parameter(torch.ones(64))
    enc = hf.vit.encoder.layer if hasattr(hf.vit, "encoder") else hf.vit.layers
    enc[1].layer_scale2 = _HfLs()
    with pytest.raises(ValueError, match=r"layer_scale2\.lambda1"):
        from_module(hf)
    m = build_layerscale(w)
    m.blocks[0].ls1 = _HfLs()
    with pytest.raises(ValueError, match=r"ls1\.lambda1"):
        from_module(m)
    # the unchanged refusals still come first on such models: register tokens, no_embed_class (timm DeiT-III), pooled heads
    for attrs, word in ((dict(no_embed_class=True), "no_embed_class"), (dict(num_reg_tokens=4), "reg_token"), (dict(global_pool="avg"), "global_pool")):
        m = build_layerscale(w)
        for k, v in attrs.items():
            setattr(m, k, v)
        with pytest.raises(ValueError, match=word):
            from_module(m)


def test_engine_vit_container_and_export_round_trip(tmp_path):
    """The rebuilt timm-layout module carries ls1 / ls2 (out of place), its state dict the gammas; an export of a width- and depth-pruned
    LayerScale module reloads through load_checkpoint to the same flat dictionary."""
    from ssp2vit import export, vit_pruning as vp
    from ssp2vit.modules import EngineViT
    from ssp2vit.weights import from_module, from_state_dict, load_checkpoint
    w = _w()
    m = EngineViT(w)
    assert m.blocks[0].ls1.inplace is False and "blocks.3.ls2.gamma" in m.state_dict()
    f = from_module(m)
    assert all(_same(f[f"{k}.{i}"], w[f"{k}.{i}"]) for k in ("ls1", "ls2") for i in range(4))
    plain = EngineViT({k: v for k, v in w.items() if not k.startswith(("ls1.", "ls2."))})
    assert not hasattr(plain.blocks[0], "ls1") and not any(".ls" in k for k in plain.state_dict())
    # prune on the host (no GPU: slice the module as the apply step does), export, reload
    keep = torch.arange(0, 128, 2)
    with torch.no_grad():
        for b in m.blocks:
            fc1, fc2 = b.mlp.fc1, b.mlp.fc2
            n1, n2 = nn.Linear(64, keep.numel()), nn.Linear(keep.numel(), 64)
            n1.weight.copy_(fc1.weight[keep]); n1.bias.copy_(fc1.bias[keep]); n2.weight.copy_(fc2.weight[:, keep]); n2.bias.copy_(fc2.bias)
            b.mlp.fc1, b.mlp.fc2 = n1, n2
    m.blocks[1].attn = vp.TimmAttentionBypass()
    want = from_module(m)
    d = export.save_pretrained_dir(m, str(tmp_path / "ls"))
    back = load_checkpoint(d)
    assert back.get("attn_absent.1") and int(back["fc1_w.0"].shape[0]) == 64
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert _same(back[k], v), k
    assert sorted(k for k in back if k.startswith("ls")) == sorted(k for k in want if k.startswith("ls")) and len([k for k in back if k.startswith("ls")]) == 8


# ---------------------------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("tag", list(LS_GOLDEN_CASES))
def test_planner_and_parameter_counts_equal_the_reference(tag):
    """The reference's planner counts model.parameters() (the gammas are in it) and takes its attention count from the attn module (they
    are not): plan_2ssp_allocation, count_total_params and the per-block counts on the LayerScale module, on the rebuilt container and
    from the shapes equal the stored answers."""
    from ssp2vit import vit_pruning as vp
    from ssp2vit.modules import EngineViT
    from ssp2vit.planner import plan_from_stats, stats_from_shapes
    from ssp2vit.weights import count_params, n_tokens
    w, _, z = load_golden(tag)
    min_rem = LS_GOLDEN_CASES[tag][4]
    for model in (build_layerscale(w), EngineViT(w)):
        assert vp.count_total_params(model) == int(z["total_params"])
        st = vp._model_stats(model)
        assert st.attn_params == z["attn_params"].tolist() and st.ffn_params == z["ffn_params"].tolist()
        for s, (k, t, err) in zip(z["plan_targets"], z["plan_k_t_err"].tolist()):
            p = vp.plan_2ssp_allocation(model, float(s), min_rem)
            assert (p.blocks_to_prune, p.per_block_neurons_to_prune, p.est_error_params) == (k, t, err), (tag, s)
    assert count_params(w) == int(z["total_params"])
    st = stats_from_shapes(int(w["dim"]), int(w["depth"]), int(w["fc1_w.0"].shape[0]), 10, n_tokens(w), int(w["patch"]), layer_scale=2)
    assert st.total_params == int(z["total_params"]) and st.attn_params == z["attn_params"].tolist()
    for s, (k, t, err) in zip(z["plan_targets"], z["plan_k_t_err"].tolist()):
        p = plan_from_stats(st, float(s), min_rem)
        assert (p.blocks_to_prune, p.per_block_neurons_to_prune, p.est_error_params) == (k, t, err), (tag, s)


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_new_entries_are_exported_and_the_abi_stays_7():
    L, lib = _lib()
    assert L.ABI_VERSION == 7 and lib.ssp2_abi_version() == 7
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "ssp2vit.h")).read()
    for name in ("ssp2_set_layer_scale", "ssp2_linear_ls_bf16", "ssp2_linear_ls_e4m3"):
        assert name in L.SYMBOLS and hasattr(lib, name) and f"int {name}(" in hdr
    assert "#define SSP2_ABI_VERSION 7" in hdr
    assert L.T_KINDS[-3:] == ["dist", "head_dist_w", "head_dist_b"] and len(L.T_KINDS) == 23          # no new tensor kinds
    assert L.OPT_COUNT == 14


def test_layerscale_kernels_have_no_scratch_and_leave_the_ten_forms_alone():
    """The LayerScale residual forms of the persistent GEMM run the body whose vector-memory operations are counted by hand
    (`s_waitcnt vmcnt(N)`): a register spill would be silently wrong data.  hipcc's resource remarks (a device-only compile, no GPU) must
    show exactly two gemm256_ls_kernel instantiations (bf16 and e4m3 operands) with zero scratch and zero spilled VGPRs, the 128 x 128
    form likewise, and still exactly the ten gemm256_bf16_kernel forms the product launched before."""
    import re
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc: the product cannot be built here")
    csrc = os.path.join(PKG, "csrc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-S",
                          os.path.join(csrc, "engine.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    name, res = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs): (\d+)", line)
        if m and name:
            res.setdefault(name, {})[m.group(1)] = int(m.group(2))
    ls = {k: v for k, v in res.items() if "gemm256_ls_kernel" in k}
    small = {k: v for k, v in res.items() if re.search(r"gemm_bf16_kernelILi5ELi0E", k)}          # gemm_bf16_kernel<EPI_RESID_LS>
    print({k: v for k, v in {**ls, **small}.items()})
    assert len(ls) == 2 and len(small) == 1, (sorted(ls), sorted(small))
    for k, v in {**ls, **small}.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 256, (k, v)
    assert sum(1 for k in res if "gemm256_bf16_kernel" in k) == 10


def test_set_layer_scale_refuses_a_null_handle():
    """(The refusals that need a live handle — layer, branch, null gamma — are in tests/test_layerscale_gpu.py.)"""
    L, lib = _lib()
    assert lib.ssp2_set_layer_scale(None, 0, 0, C.c_void_p(0x1000), 0) == -1 and lib.ssp2_last_error()


def test_layerscale_operators_refuse_bad_arguments_before_touching_the_device():
    """Every refusal is SSP2_EINVAL (-1) with fake pointers that are never dereferenced: it happens before the first HIP call."""
    L, lib = _lib()
    fake = C.c_void_p(0x1000)

    def bf(a=fake, lda=256, w=fake, ldw=256, bias=fake, gamma=fake, M=300, N=256, K=256, x=fake, xin=None, ldx=256, kernel=0, rev=0):
        return lib.ssp2_linear_ls_bf16(None, a, lda, w, ldw, bias, gamma, M, N, K, x, xin, ldx, kernel, rev)

    def f8(a=fake, lda=256, asc=None, ac=0.0, w=fake, ldw=256, ws=fake, bias=fake, gamma=fake, M=300, N=256, K=256, x=fake, xin=None, ldx=256, rev=0):
        return lib.ssp2_linear_ls_e4m3(None, a, lda, asc, ac, w, ldw, ws, bias, gamma, M, N, K, x, xin, ldx, rev)

    bad_bf = {"null a": dict(a=None), "null w": dict(w=None), "null bias": dict(bias=None), "null gamma": dict(gamma=None), "null x": dict(x=None),
              "gamma not 16-byte aligned": dict(gamma=C.c_void_p(0x1004)),
              "M 0": dict(M=0), "N not % 64": dict(N=200), "K not % 64": dict(K=200, lda=200, ldw=200), "lda < K": dict(lda=128),
              "ldw not % 8": dict(ldw=260), "ldx < N": dict(ldx=128), "ldx not % 4": dict(ldx=258), "kernel 3": dict(kernel=3),
              "kernel -1": dict(kernel=-1), "rev 2": dict(rev=2), "rev -1": dict(rev=-1)}
    for what, kw in bad_bf.items():
        assert bf(**kw) == -1, what
        assert lib.ssp2_last_error()
    bad_f8 = {"null a": dict(a=None), "null w": dict(w=None), "null bias": dict(bias=None), "null gamma": dict(gamma=None), "null x": dict(x=None),
              "gamma not 16-byte aligned": dict(gamma=C.c_void_p(0x1008)), "null wscale": dict(ws=None), "K not % 128": dict(K=192), "N not % 64": dict(N=200), "lda not % 16": dict(lda=264),
              "ldw < K": dict(ldw=128), "ascale_const < 0": dict(ac=-1.0), "ascale_const nan": dict(ac=float("nan")),
              "both scales": dict(asc=fake, ac=0.5), "ldx < N": dict(ldx=64), "rev 2": dict(rev=2), "M 0": dict(M=0)}
    for what, kw in bad_f8.items():
        assert f8(**kw) == -1, what
        assert lib.ssp2_last_error()


def test_engine_refuses_a_gamma_of_the_wrong_length_by_name():
    from ssp2vit.engine import VitEngine
    w = _w()
    w["ls2.1"] = torch.ones(32)
    with pytest.raises(ValueError, match=r"ls2\.1"):
        VitEngine._layer_scale_of(w, 4, 64)
    assert VitEngine._layer_scale_of(_w(), 4, 64) == ((True, True),) * 4
