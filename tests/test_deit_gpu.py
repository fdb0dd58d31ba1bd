"""Distilled DeiT on the MI355X: two prefix tokens (CLS + distillation token), the evaluation tail on both prefix rows and the
averaged two-head classifier.  Kernels on their own against float64 (embed rows, the prefix-query attention on the resident and the
key-streaming kernel), the tail bit for bit against the full last block, whole models against the CPU restatement of
tests/deit_models.py (the oracle's blocks with DeiT's embedding and heads, under CPU autocast), the apply step, fp8 at one cut, the
layout-free engine against ssp2_create, and the reference-named API / CLI end to end."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT
from deit_models import build_distilled
from test_operator_numerics_gpu import GUARD, PATTERNS, SENT, _attn_inputs, _attn_ref, _image_rows, _pack_qkv

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -7          # bf16 ulp at 1.0 (8 significant bits)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(gpu):
    """Any engine: the operator entries it wraps take their geometry from the call (the tiny d_h 16 model)."""
    from ssp2vit.engine import VitEngine
    e = VitEngine(_w("deit_test_distilled_patch16_32"), device=gpu, max_images=4)
    yield e
    e.close()


def _w(name, seed=3, **kw):
    from ssp2vit.weights import synthetic_weights
    kw.setdefault("std", 0.03)
    kw.setdefault("bias_std", 0.02)
    return synthetic_weights(name, classes=10, seed=seed, **kw)


def _px(n, img, seed=0):
    return torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(seed))


def _hf_flat(w):
    """The same weights as an HF-origin model: eps 1e-12 (the engine and the restatement both read w["eps"])."""
    return dict(w, eps=1e-12)


# ----------------------------------------------------------------------------------------------------------------- 1. embed
@pytest.mark.parametrize("name", ["deit_test_distilled_patch16_32", "deit_small_distilled_patch16_224_d2"])
def test_embed_rows_vs_float64_both_patch_paths(gpu, name):
    """Row 0 = cls + pos[0] and row 1 = dist + pos[1] exactly (one fp32 add); patch q at token 2 + q = float(bf16(conv + bias)) +
    pos[2 + q] against a float64 convolution of the bf16-rounded operands (bound: the bf16 rounding of the sum plus the fp32
    accumulation); SSP2_OPT_PATCH_LDS 0 and 1 give the same bits, in the contiguous and the slab layout."""
    from ssp2vit.engine import VitEngine
    w = _w(name)
    n, img, p, D = 5, int(w["img"]), int(w["patch"]), int(w["dim"])
    eng = VitEngine(w, max_images=n)
    assert eng.tokens == (img // p) ** 2 + 2 and eng.prefix_tokens == 2 and eng.dist_head == 1
    px = _px(n, img).to(gpu)
    outs = {}
    for lds in (1, 0):
        eng.set_option("patch_lds", lds)
        for group in (0, 2):
            outs[(lds, group)] = eng.embed(px, group=group).clone()
    torch.cuda.synchronize()
    assert torch.equal(outs[(1, 0)], outs[(0, 0)]) and torch.equal(outs[(1, 2)], outs[(0, 2)])
    x = outs[(1, 0)].view(n, eng.tokens, D).cpu()
    pos = w["pos"].reshape(-1, D)
    assert torch.equal(x[:, 0], (w["cls"].reshape(D) + pos[0]).expand(n, D))
    assert torch.equal(x[:, 1], (w["dist"].reshape(D) + pos[1]).expand(n, D))
    bf = lambda t: t.to(torch.bfloat16).double()
    conv = torch.nn.functional.conv2d(bf(px.cpu()), bf(w["patch_w"]), bf(w["patch_b"]), stride=p)     # [n, D, side, side]
    ref = conv.flatten(2).transpose(1, 2) + pos[2:].double()
    err = (x[:, 2:].double() - ref).abs()
    bound = 2.0 ** -8 * conv.flatten(2).transpose(1, 2).abs() + 2.0 ** -24 * (3 * p * p + 2) * \
        (bf(px.cpu()).abs().unfold(2, p, p).unfold(3, p, p).sum((-1, -2)).sum(1).flatten(1)[:, :, None].expand(-1, -1, D)
         * bf(w["patch_w"]).abs().amax()) + 2.0 ** -23 * ref.abs() + 1e-30
    print(f"[deit-embed] {name}: max err/bound {float((err / bound).max()):.3f}")
    assert float((err / bound).max()) <= 1.0
    # the slab layout puts the same rows at the slab offsets
    idx, _ = _image_rows(n, eng.tokens, 2, gpu)
    assert torch.equal(outs[(1, 2)][idx.reshape(-1)].view(n, eng.tokens, D).cpu(), x)
    eng.close()


# ------------------------------------------------------------------------------------------------- 2. prefix-query attention
@pytest.mark.parametrize("tokens,stream", [(198, 0), (6, 0), (578, 1), (198, 1)])
@pytest.mark.parametrize("n_prefix", [1, 2])
def test_prefix_attention_vs_float64(gpu, eng, tokens, stream, n_prefix):
    """ssp2_attention_prefix_bf16 on caller buffers: n_prefix queries per image (prefix-major q and out) against float64, on the resident
    CLS-only kernel (198 tokens at d_h 64, 6 at d_h 16) and the key-streaming one (578 and 198 tokens), with the peaked score patterns of
    test_operator_numerics_gpu and its element-wise bound.  qkv's q columns, slab pad rows and q rows past n_prefix * n are NaN; out
    rows / columns past the written ones keep a sentinel."""
    d_h = 16 if tokens == 6 else 64
    heads = 3
    n = len(PATTERNS)
    dim = heads * d_h
    g = torch.Generator().manual_seed(11 + tokens + n_prefix)
    q, k, v = _attn_inputs(n, tokens, heads, d_h, g, PATTERNS)
    for group in (3, 0):
        idx, rows = _image_rows(n, tokens, group, gpu)
        qkv = _pack_qkv(q, k, v, idx, rows, gpu)
        qkv[:, :dim] = float("nan")
        qp = torch.full((n_prefix * n + GUARD, dim), float("nan"), dtype=torch.bfloat16, device=gpu)
        for t in range(n_prefix):
            qp[t * n:(t + 1) * n] = q[:, :, t, :].reshape(n, dim).to(gpu, torch.bfloat16)
        out = torch.full((n_prefix * n + GUARD, dim + 8), SENT, dtype=torch.bfloat16, device=gpu)
        eng.attention_prefix(qkv, n, tokens, heads, d_h, qp, n_prefix, group=group, out=out, stream=bool(stream))
        torch.cuda.synchronize()
        o, core = _attn_ref(q.to(gpu), k.to(gpu), v.to(gpu), d_h)
        worst = 0.0
        for t in range(n_prefix):
            ot, ct = o[:, :, t, :].reshape(n, dim), core[:, :, t, :].reshape(n, dim)
            if stream:          # online softmax: each rescale adds a rounding of O and of the sum (attn_stream.hip.h)
                ct = ct + 2.0 ** -22 * (-(-tokens // 64)) * (o.abs()[:, :, t, :].reshape(n, dim) + ct)
            bound = 2.0 ** -8 * (ot.abs() + ct) + ct + 1e-30
            got = out[t * n:(t + 1) * n, :dim].double()
            assert not torch.isnan(got).any(), (tokens, stream, n_prefix, group, t)
            worst = max(worst, float(((got - ot).abs() / bound).max()))
        print(f"[deit-attn-prefix] T={tokens} stream={stream} P={n_prefix} group={group}: max err/bound {worst:.3f}")
        assert worst <= 1.0
        assert bool((out[:n_prefix * n, dim:].float() == SENT).all()) and bool((out[n_prefix * n:].float() == SENT).all())


def test_prefix_attention_p1_is_the_cls_only_form_bit_for_bit(gpu, eng):
    """n_prefix = 1 runs the instantiations of the CLS-only form: the same bits as ssp2_attention_bf16(q_cls) and
    ssp2_attention_stream_bf16(q_cls)."""
    for tokens, stream in ((197, False), (577, True)):
        n, heads, d_h = 8, 3, 64
        dim = heads * d_h
        g = torch.Generator().manual_seed(tokens)
        q, k, v = _attn_inputs(n, tokens, heads, d_h, g, PATTERNS)
        idx, rows = _image_rows(n, tokens, 0, gpu)
        qkv = _pack_qkv(q, k, v, idx, rows, gpu)
        q_cls = q[:, :, 0, :].reshape(n, dim).to(gpu, torch.bfloat16).contiguous()
        a = eng.attention(qkv, n, tokens, heads, d_h, q_cls=q_cls, stream=stream)
        b = eng.attention_prefix(qkv, n, tokens, heads, d_h, q_cls, 1, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(a[:n], b[:n]), (tokens, stream)


# ----------------------------------------------------------------------------------------------------- 3. the two-row tail
@pytest.mark.parametrize("name,dist_head", [("deit_small_distilled_patch16_224_d2", 1), ("deit_test_distilled_patch16_32", 1),
                                            ("deit_small_distilled_patch16_224_d2", 0)])
def test_prefix_tail_is_bit_identical_to_the_full_last_block(gpu, name, dist_head):
    """tail() carries rows 0 and 1 (only row 0 for a CLS head on two prefix tokens) through the last block: the logits, preds and
    counts equal layers(depth-1, depth) + head() bit for bit, in the contiguous layout, the slab layout and with slots."""
    from ssp2vit.engine import VitEngine
    w = _w(name)
    if not dist_head:
        w = {k: v for k, v in w.items() if not k.startswith("head_dist")}
    n, img = 12, int(w["img"])
    eng = VitEngine(w, max_images=3 * n)
    assert eng.dist_head == dist_head
    px = _px(n, img, seed=2).to(gpu)
    labels = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(1)).to(gpu)
    L = eng.depth
    for group in (0, 4):
        x = eng.embed(px, group=group)
        eng.layers(x, n, 0, L - 1, score_group=group)
        x_in = x.clone()
        lt, pt, ct = eng.tail(x, n, labels=labels, want_logits=True, want_pred=True, group=group)
        assert torch.equal(x, x_in)                                  # the tail leaves x alone
        eng.layers(x, n, L - 1, L, score_group=group)
        lf, pf, cf = eng.head(x, n, labels=labels, want_logits=True, want_pred=True, group=group)
        torch.cuda.synchronize()
        assert torch.equal(lt, lf) and torch.equal(pt, pf) and torch.equal(ct, cf), (name, group)
        assert torch.equal(pf.long(), lf.argmax(-1))
    # three slots side by side (the layer-major search's tail): slot s is counted in correct[s]
    x = eng.embed(px)
    eng.layers(x, n, 0, L - 1)
    x3 = torch.cat([x, x, x], 0).contiguous()
    l3, p3, c3 = eng.tail(x3, n, labels=labels, want_logits=True, want_pred=True, slots=3)
    l1, p1, c1 = eng.tail(x, n, labels=labels, want_logits=True, want_pred=True)
    torch.cuda.synchronize()
    assert torch.equal(l3, torch.cat([l1] * 3)) and torch.equal(c3, c1.expand(3))
    eng.close()


# ------------------------------------------------------------------------------------------- 4. whole models vs the restatement
def _check_logits(got, ref, tag):
    err = float((got.float() - ref.float()).abs().max())
    top = float(ref.float().abs().max())
    print(f"[deit-logits] {tag}: max |err| {err:.3e}, largest logit {top:.3e} ({err / (BF16_ULP * top):.2f} bf16 ulp of it)")
    assert err <= 2 * BF16_ULP * top, tag


@pytest.mark.parametrize("layout,teacher", [("timm", True), ("hf", True), ("hf", False)])
@pytest.mark.parametrize("name", ["deit_test_distilled_patch16_32", "deit_small_distilled_patch16_224_d2"])
def test_dense_logits_and_stage1_scores_vs_the_cpu_restatement(gpu, name, layout, teacher):
    """The engine built from the live CPU module (from_module) against the module itself under CPU autocast: logits within 2 bf16 ulp of
    the largest logit; stage-1 scores at the hook site of the anatomy — bf16 chain <= 2 ulp and >= 90 % identical, fp32 chain within
    rel 2e-3 (pre-GELU) / 5.9e-3 (post-GELU); top-1 counts equal where the restatement's margins decide them."""
    from oracle import ref_cpu
    from ssp2vit import vit_pruning as vp, weights as W
    from ssp2vit.engine import VitEngine
    w = _w(name, seed=5)
    if layout == "hf":
        w = _hf_flat(w)
    model = build_distilled(w, layout, teacher)
    flat = W.from_module(model)
    assert flat["prefix_tokens"] == 2 and ("head_dist_w" in flat) == teacher
    n, img = 16, int(w["img"])
    px = _px(n, img, seed=7)
    eng = VitEngine(flat, max_images=n)
    got = eng.forward_logits(px.to(gpu)).cpu()
    ref = ref_cpu.logits_of(model, px).float()
    _check_logits(got, ref, f"{name} {layout} teacher={teacher}")
    batches = [{"pixel_values": px[:8]}, {"pixel_values": px[8:]}]
    rtol = 2e-3 if W.score_site_for(layout) == "pre_gelu" else 5.9e-3
    for chain in ("bf16_ref", "fp32"):
        got_s = vp._compute_ffn_activation_importance(model, batches, device="cuda", score_chain=chain)      # the hook site of the anatomy
        ref_s = ref_cpu.ffn_activation_importance(model, batches, chain="autocast" if chain == "bf16_ref" else "fp32")
        for l, (a, r) in enumerate(zip(got_s, ref_s)):
            if chain == "bf16_ref":
                ulp = (a.cpu().view(torch.int16).int() - r.to(torch.bfloat16).view(torch.int16).int()).abs()
                assert int(ulp.max()) <= 2 and float((ulp == 0).float().mean()) >= 0.9, (name, layout, l, int(ulp.max()))
            else:
                assert torch.allclose(a.cpu(), r, rtol=rtol, atol=1e-4), (name, layout, l)
    vp.release_engines(free=True)
    labels = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(3))
    c_ref = (ref.argmax(-1) == labels)
    c_eng = (got.argmax(-1) == labels)
    top2 = ref.topk(2, -1).values
    decided = (top2[:, 0] - top2[:, 1]) > 4 * BF16_ULP * ref.abs().amax(-1)
    assert torch.equal(c_ref[decided], c_eng[decided])
    if (~decided).any():
        print(f"[deit-logits] {int((~decided).sum())} image(s) with an undecided top-1 margin: ref {c_ref[~decided].tolist()} eng {c_eng[~decided].tolist()}")
    eng.close()


@pytest.mark.parametrize("tag,layout", [(t, l) for t in ("deit_test", "deit_s16") for l in ("timm", "hf")])
def test_engine_vs_the_reference_goldens(gpu, tag, layout):
    """The engine on the live distilled module against the REAL reference's outputs (tests/golden/make_golden_deit.py): bf16 stage-1
    scores <= 2 ulp and >= 90 % identical; dense logits within 2 bf16 ulp of the largest logit; per image, top-1 correctness equal
    wherever the stored logits' margin decides it; each block's impact (Auto2SSPInterface copy mode) equal wherever the baseline's and
    that block's bypassed model's stored margins decide every image; the K selection equal when every impact is decided."""
    from deit_models import DEIT_GOLDEN_CASES, bf16_from_bits, load_golden
    from ssp2vit import vit_pruning as vp
    from ssp2vit.mask_conjunction import Auto2SSPInterface
    w, batches, z = load_golden(tag, layout)
    model = build_distilled(w, layout, teacher=True)
    depth, K = int(w["depth"]), DEIT_GOLDEN_CASES[tag][5]
    imps = vp._compute_ffn_activation_importance(model, batches, device="cuda", score_chain="bf16_ref")
    for l, a in enumerate(imps):
        ulp = (a.cpu().view(torch.int16).int() - bf16_from_bits(z[f"s1_imp_bf16bits.{l}"]).view(torch.int16).int()).abs()
        print(f"[deit-golden] {tag} {layout} block {l}: scores max {int(ulp.max())} ulp, {float((ulp == 0).float().mean()):.3f} identical")
        assert int(ulp.max()) <= 2 and float((ulp == 0).float().mean()) >= 0.9, (tag, layout, l)

    def decided(key_fmt):
        """per batch: images whose stored top-1 margin exceeds twice the logit bar (so the engine's argmax must agree)."""
        out = []
        for i in range(len(batches)):
            ref = bf16_from_bits(z[key_fmt.format(i=i)]).float()
            top2 = ref.topk(2, -1).values
            out.append(((top2[:, 0] - top2[:, 1]) > 2 * (2 * BF16_ULP * ref.abs().max()), ref))
        return out

    eng = vp.engine_for(model, "cuda", max_images=32)
    N = sum(int(b["labels"].numel()) for b in batches)

    def check_model(key_fmt, skip, tag_):
        """Per-image top-1 correctness equal on the decided images; returns the interval of accuracies the undecided ones allow."""
        lo = hi = 0
        for i, (b, (dec, ref)) in enumerate(zip(batches, decided(key_fmt))):
            got = eng.forward_logits(b["pixel_values"].to(gpu), attn_skip=skip).cpu()
            _check_logits(got, ref, f"{tag} {layout} {tag_} batch {i} vs the reference")
            ok_ref, ok_got = ref.argmax(-1) == b["labels"], got.argmax(-1) == b["labels"]
            assert torch.equal(ok_ref[dec], ok_got[dec]), (tag, layout, tag_, i)
            lo += int((ok_ref & dec).sum()); hi += int((ok_ref & dec).sum()) + int((~dec).sum())
        return lo / N, hi / N

    blo, bhi = check_model("logits_bf16bits.{i}", None, "dense")
    top1 = vp.evaluate_top1(model, batches, device="cuda", progress=False)
    print(f"[deit-golden] {tag} {layout}: top1 engine {top1} reference {float(z['top1'])}, decided interval [{blo}, {bhi}]")
    assert blo <= top1 <= bhi and blo <= float(z["top1"]) <= bhi
    att, _ = Auto2SSPInterface(model, batches, device="cuda", importance_mode="copy", batch_limit=5).fit()
    att = att.float().cpu()
    ref_att = torch.from_numpy(z["att_imp"])
    all_dec = True
    for blk in range(depth):
        plo, phi = check_model(f"bypass_logits_bf16bits.{blk}.{{i}}", [blk], f"attention {blk} bypassed")
        ilo, ihi = max(0.0, blo - phi), max(0.0, bhi - plo)        # impact = max(0, baseline - bypassed top-1)
        print(f"[deit-golden] {tag} {layout} block {blk}: impact engine {float(att[blk])} reference {float(ref_att[blk])}, "
              f"decided interval [{ilo}, {ihi}]")
        assert ilo - 1e-6 <= float(att[blk]) <= ihi + 1e-6, (tag, layout, blk)
        all_dec = all_dec and ilo == ihi
    sel = sorted(int(i) for i in torch.argsort(att)[:K])
    print(f"[deit-golden] {tag} {layout}: selection engine {sel} reference {z[f's2_selected_k{K}'].tolist()} (every impact decided: {all_dec})")
    if all_dec:
        assert sel == z[f"s2_selected_k{K}"].tolist()
    vp.release_engines(free=True)


def test_transformers_deit_teacher_and_cls_models_vs_their_own_forward(gpu):
    """The installed transformers' DeiTForImageClassificationWithTeacher and DeiTForImageClassification (the `deit.layers` anatomy): the
    engine's logits within 2 bf16 ulp of the model's own forward under CPU autocast."""
    transformers = pytest.importorskip("transformers")
    from ssp2vit import vit_pruning as vp
    cfg = transformers.DeiTConfig(image_size=32, patch_size=16, hidden_size=64, num_hidden_layers=3, num_attention_heads=4,
                                  intermediate_size=128, num_labels=10)
    px = _px(8, 32, seed=9)
    for cls in (transformers.DeiTForImageClassificationWithTeacher, transformers.DeiTForImageClassification):
        torch.manual_seed(0)
        m = cls(cfg).eval()
        with torch.no_grad():
            for p_ in m.parameters():
                p_.add_(0.02 * torch.randn_like(p_))
            with torch.autocast(device_type="cpu", enabled=True):
                ref = m(pixel_values=px).logits.float()
        got = vp.engine_for(m, "cuda", max_images=8).forward_logits(px.to(gpu)).cpu()
        _check_logits(got, ref, cls.__name__)
    vp.release_engines(free=True)


# ------------------------------------------------------------------------------------------------------- 5. apply and export
def test_apply_into_twin_equals_an_engine_of_the_host_sliced_weights_and_the_export_reloads(gpu, tmp_path):
    """Width masks + dropped attention applied into a pruned twin (device gathers) give the same logits, bit for bit, as an engine built
    from weights sliced on the host; the reference-named API's pruned module exports and reloads (dist_token, head_dist) to the same
    logits."""
    from ssp2vit import export, vit_pruning as vp, weights as W
    from ssp2vit.engine import VitEngine
    from ssp2vit.modules import EngineViT
    w = _w("deit_small_distilled_patch16_224_d2", seed=6)
    depth, d_int = int(w["depth"]), int(w["fc1_w.0"].shape[0])
    g = torch.Generator().manual_seed(2)
    masks = []
    for l in range(depth):
        m = torch.zeros(d_int, dtype=torch.int64)
        m[torch.randperm(d_int, generator=g)[:d_int // 4]] = 1
        masks.append(m)
    n, px = 8, _px(8, 224, seed=4).to(gpu)
    dense = VitEngine(w, max_images=n)
    twin = dense.pruned_twin([d_int - d_int // 4] * depth, max_images=n)
    dense.apply_into(twin, masks, [1])
    sliced = dict(w)
    for l, m in enumerate(masks):
        keep = torch.nonzero(m == 0).view(-1)
        sliced[f"fc1_w.{l}"] = w[f"fc1_w.{l}"][keep]; sliced[f"fc1_b.{l}"] = w[f"fc1_b.{l}"][keep]
        sliced[f"fc2_w.{l}"] = w[f"fc2_w.{l}"][:, keep]
    sliced["attn_absent.1"] = True
    host = VitEngine(sliced, max_images=n)
    a, b = twin.forward_logits(px), host.forward_logits(px)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    # the API on the timm-layout container, then export -> load_checkpoint -> same logits
    model = EngineViT(w).to(gpu)
    res = vp.prune_vit_mlp_width(model, n_to_prune_per_block=[d_int // 4] * depth, min_remaining=64, strategy="l1",
                                 collect_masks=True, precomputed_importance=[torch.rand(d_int, generator=g) for _ in range(depth)])
    out = vp.prune_vit_attention_blocks(res["model"], sparsity=0.5, dataloader=None, device=gpu, num_to_prune=1, show_progress=False,
                                        selected_indices=[1])
    pm = out["model"]
    assert hasattr(pm, "dist_token") and hasattr(pm, "head_dist")
    l_api = pm(px).cpu()
    d = export.save_pretrained_dir(pm, str(tmp_path / "deit"))
    back = W.load_checkpoint(d)
    assert back["prefix_tokens"] == 2 and "head_dist_w" in back and back.get("attn_absent.1")
    l_back = VitEngine(back, max_images=n).forward_logits(px).cpu()
    assert torch.equal(l_api, l_back)
    vp.release_engines(free=True)


# ------------------------------------------------------------------------------------------------------- 6. 578 tokens
def test_384_pixel_distilled_model_on_the_streaming_attention_vs_the_restatement(gpu):
    """deit_base_distilled_patch16_384 cut to two blocks: 578 tokens on the key-streaming kernels (attn_stream=1), logits and fp32-chain
    stage-1 scores against the CPU restatement."""
    from oracle import ref_cpu
    from ssp2vit.engine import VitEngine
    w = _w("deit_base_distilled_patch16_384_d2", seed=12, std=0.02)
    model = build_distilled(w, "timm")
    n, px = 4, _px(4, 384, seed=13)
    with pytest.raises(Exception, match="SSP2_OPT_ATTN_STREAM"):
        VitEngine(w, max_images=n, attn_stream=0)
    eng = VitEngine(w, max_images=n, attn_stream=1)
    assert eng.tokens == 578
    got = eng.forward_logits(px.to(gpu)).cpu()
    _check_logits(got, ref_cpu.logits_of(model, px).float(), "deit_base_distilled_patch16_384_d2 stream")
    sc = eng.forward_scores(px.to(gpu), "pre_gelu", "fp32")[0].cpu() / n       # sums over the images; the reference averages
    for l, r in enumerate(ref_cpu.ffn_activation_importance(model, [{"pixel_values": px}], chain="fp32")):
        rel = (sc[l, :r.numel()] - r).abs() / r.abs().clamp_min(1e-3)            # the bars of test_long_sequence_gpu at 577 tokens
        assert float(rel.max()) <= 5e-3 and float(rel.mean()) <= 5e-4, (l, float(rel.max()), float(rel.mean()))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7. fp8
def test_fp8_distilled_cut_tracks_the_bf16_engine(gpu):
    """A distilled engine in fp8 mode (attention and the tail stay bf16, nothing of the fp8 path depends on the prefix count): the bars of
    test_fp8_engine_tracks_the_bf16_engine_within_the_e4m3_tolerance — logits rel L2 <= 0.15 and correlation >= 0.98, stage-1 scores
    mean rel <= 2 %, max <= 10 % — and the fp8 kernels really ran."""
    from ssp2vit.engine import VitEngine
    w = _w("deit_small_distilled_patch16_224_d2", seed=8, spread=4.0)
    d_int = int(w["fc1_w.0"].shape[0])
    ref = VitEngine(w, max_images=64)
    f8 = VitEngine(w, max_images=64, precision="fp8")
    px = _px(64, 224, seed=4).to(gpu)
    lr, l8 = ref.forward_logits(px).cpu(), f8.forward_logits(px).cpu()
    rel = float((l8 - lr).norm() / lr.norm())
    corr = float(torch.corrcoef(torch.stack([l8.flatten(), lr.flatten()]))[0, 1])
    sr, s8 = ref.forward_scores(px, "pre_gelu")[0].cpu(), f8.forward_scores(px, "pre_gelu")[0].cpu()
    e = (s8[:, :d_int] - sr[:, :d_int]).abs() / sr[:, :d_int].abs().clamp_min(1e-6)
    print(f"[deit-fp8] logits rel {rel:.4f} corr {corr:.5f}; scores rel mean {float(e.mean()):.4f} max {float(e.max()):.4f}")
    assert not torch.equal(l8, lr)
    assert rel <= 0.15 and corr >= 0.98
    assert float(e.mean()) <= 0.02 and float(e.max()) <= 0.10
    ref.close(); f8.close()


# ----------------------------------------------------------------------------------------------- 8. the layout-free engine
@pytest.mark.parametrize("name", ["vit_small_patch16_224_d2", "vit_test_patch16_32"])
def test_create_ext_with_one_prefix_token_equals_create(gpu, name):
    """ssp2_create / ssp2_create_opts now forward to ssp2_create_ext with ext = NULL; this checks that an explicit one-token layout
    ext = {1, 0} builds the same engine (embed, scores, tail logits bit for bit).  That one-prefix models compute what they computed
    before this layout existed is shown by the whole GPU suite and by bench.py --dump-outputs against the previous build."""
    from ssp2vit import _lib
    from ssp2vit.engine import VitEngine
    w = _w(name)
    a = VitEngine(w, max_images=8)
    b = VitEngine(w, max_images=8)
    old = b.h
    arr = (C.c_int32 * b.depth)(*b.d_int)
    desc = _lib.VitDesc(b.img, b.patch, b.dim, b.heads, b.depth, b.classes, float(b.eps), b.max_images, arr)
    h = C.c_void_p()
    ext = _lib.VitExt(1, 0)
    opts = (C.c_int32 * _lib.OPT_COUNT)(*([-1] * _lib.OPT_COUNT))
    b._check(b.lib.ssp2_create_ext(C.byref(desc), opts, C.byref(ext), C.byref(h)))
    b.h = h
    b._load(w)
    b.lib.ssp2_destroy(old)
    px = _px(8, int(w["img"]), seed=1).to(gpu)
    assert torch.equal(a.embed(px), b.embed(px))
    assert torch.equal(a.forward_scores(px, "pre_gelu"), b.forward_scores(px, "pre_gelu"))
    assert torch.equal(a.forward_logits(px), b.forward_logits(px))
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------- 9. API and CLI end to end
def test_reference_api_on_a_live_hf_teacher_module(gpu):
    """evaluate_top1, the Auto2SSPInterface importances, prune_vit_mlp_width and prune_vit_attention_blocks on a live (old-anatomy) HF
    DeiT teacher module: the engine reads its distillation token and both heads, the module is sliced and bypassed in place, and the
    pruned module's logits are the engine's for the sliced weights."""
    from oracle import ref_cpu
    from ssp2vit import vit_pruning as vp, weights as W
    from ssp2vit.mask_conjunction import Auto2SSPInterface
    from ssp2vit.engine import VitEngine
    w = _hf_flat(_w("deit_test_distilled_patch16_32", seed=21))
    model = build_distilled(w, "hf", teacher=True)
    px = _px(32, 32, seed=22)
    labels = ref_cpu.logits_of(model, px).argmax(-1)
    loader = [{"pixel_values": px[i:i + 8], "labels": labels[i:i + 8]} for i in range(0, 32, 8)]
    acc = vp.evaluate_top1(model, loader, device="cuda", progress=False)
    assert acc >= 0.9, acc                                          # teacher labels: the engine agrees with the module
    iface = Auto2SSPInterface(model, loader, device="cuda", batch_limit=2, min_remaining=32)
    att, mlp = iface.fit()
    assert att.numel() == int(w["depth"]) and len(mlp) == int(w["depth"])
    res = vp.prune_vit_mlp_width(model, n_to_prune_per_block=[32] * int(w["depth"]), min_remaining=32, strategy="l1",
                                 collect_masks=True, precomputed_importance=[m.float() for m in mlp])
    out = vp.prune_vit_attention_blocks(res["model"], sparsity=0.25, dataloader=None, device="cuda", num_to_prune=1, show_progress=False,
                                        selected_indices=[int(torch.argsort(att)[0])])
    pm = out["model"]
    assert pm.deit.encoder.layer[0].intermediate.dense.out_features == 96
    flat = W.from_module(pm)
    assert flat["prefix_tokens"] == 2 and "head_dist_w" in flat and sum(bool(flat.get(f"attn_absent.{i}")) for i in range(4)) == 1
    e = VitEngine(flat, max_images=32)
    assert torch.equal(vp.engine_for(pm, "cuda", max_images=32).forward_logits(px.to(gpu)), e.forward_logits(px.to(gpu)))
    e.close()
    vp.release_engines(free=True)


def test_cli_distilled_model_end_to_end(gpu, tmp_path):
    """auto_2ssp.py --model deit_test_distilled_patch16_32 (synthetic weights) prunes and writes its report; --weights reads the timm
    checkpoint of a distilled module back."""
    from ssp2vit.weights import synthetic_weights
    from deit_models import build_distilled
    cli = os.path.join(PKG, "auto_2ssp.py")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    out = tmp_path / "out"
    common = ["--sparsity_rate", "0.25", "--min-remaining", "32", "--synthetic-calib", "64", "--eval-batches", "2", "--batch-size", "16",
              "--num-classes", "10"]
    r = subprocess.run([sys.executable, cli, "--model", "deit_test_distilled_patch16_32", "--output-dir", str(out), *common],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert list(out.rglob("report-*.json")), "no report written"
    w = synthetic_weights("deit_test_distilled_patch16_32", classes=10, seed=4)
    m = build_distilled(w, "timm")
    ck = tmp_path / "deit.pth"
    torch.save(m.state_dict(), ck)
    r = subprocess.run([sys.executable, cli, "--weights", str(ck), "--heads", "4", "--output-dir", str(tmp_path / "o2"), *common],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
