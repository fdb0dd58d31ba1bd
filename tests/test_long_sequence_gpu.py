"""Long sequences on the key-streaming attention (csrc/attn_stream.hip.h; SSP2_OPT_ATTN_STREAM): the operator against float64, whole
models against the CPU oracle at 577 and 785 tokens, stage 2 and the apply step at 577 tokens, the all-streaming mode against the
resident kernels, the CLI switch, and the fp8 refusal.

Bound of the online softmax (ssp2_attention_stream_bf16), derived from the resident kernels' bound (tests/test_operator_numerics_gpu.py,
module docstring: symbols u, A, smax, c2, S1, NT there) by adding the terms of the stage-wise rescale.  NS = stages (128 keys per stage
for the full form, 64 per chunk for the CLS-only form).  A key of stage j enters the output with the numerator
exp2(fma(s, c2, -m_j c2)) times the rescale factors a_i = exp2(fma(m_(i-1), c2, -m_i c2)) of every later stage i; the product
telescopes to exp2((s - M) c2) exactly, so the new errors are:
  * -m_i c2 is rounded once per stage (u smax c2 in the log2 domain); only the LAST stage's rounding is common to every key and cancels in
    the normalisation: (NS - 1) u smax c2;
  * the exponent of each a_i is an fma rounded once, |m_(i-1) - m_i| c2 <= 2 smax c2: (NS - 1) 2 u smax c2;
    => delta = c2 ((d_h + 2) u A + (17 + 3 (NS - 1)) u smax);
  * each a_i: v_exp_f32 (<= 2 ulp, 4u) and one multiply of O (or one fma of the running sum), u: eta += 5 (NS - 1) u;
  * the running sum: per stage the two interleaved partial sums of the resident kernel, plus one add of the two partials and one fma
    with the rescale: sigma = (8 NT + 2 NS + 20) u;
  * P V accumulation unchanged: acc = (32 NT + 16) u (the rescale multiplies are in eta).
The CLS-only form keeps P in fp32 (no bf16 rounding of P: the 2^-8 term of e_num is an over-estimate there), sums its 64-term dot
products sequentially ((d_h + 2) u A covers d_h fmas) and accumulates P V over at most 32 NT keys sequentially (acc covers it).
No slack factor is applied.
"""
import copy
import importlib.util
import math
import os

import pytest
import torch

from conftest import PKG
from test_operator_numerics_gpu import GUARD, LN2, PATTERNS, SENT, U, _attn_inputs, _bf, _image_rows, _pack_qkv, _to_rows

pytestmark = pytest.mark.gpu

STREAM_PATTERNS = PATTERNS + ("ramp",)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(gpu):
    from conftest import load_tiny_golden
    from ssp2vit.engine import VitEngine
    w, _, _ = load_tiny_golden("timm")
    e = VitEngine(w, device="cuda:0", max_images=4)
    yield e
    e.close()


def _inputs(n, tokens, heads, g):
    """The existing score patterns plus `ramp`: scores rise with the key index, so the running maximum grows in every stage and the
    global maximum sits in the last key tile (a rescale on every stage, the last one late)."""
    d_h = 64
    q, k, v = _attn_inputs(n, tokens, heads, d_h, g, STREAM_PATTERNS)
    sc = 1.0 / math.sqrt(d_h)
    for i in range(n):
        if STREAM_PATTERNS[i % len(STREAM_PATTERNS)] != "ramp":
            continue
        for h in range(heads):
            lam = (40.0 if h % 2 == 0 else 6.0) / (sc * d_h)
            r = torch.randint(0, 2, (d_h,), generator=g).float() * 2 - 1
            ramp = torch.linspace(-1.0, 1.0, tokens)[:, None]
            q[i, h] = _bf(r[None, :] + 0.05 * torch.randn(tokens, d_h, generator=g))
            k[i, h] = _bf(lam * ramp * r[None, :] + 0.3 * torch.randn(tokens, d_h, generator=g))
    return q, k, v


def _stream_ref(q, k, v, stage):
    """float64 reference and the online-softmax bound of the module docstring"""
    q, k, v = q.double(), k.double(), v.double()
    d_h, tokens = q.shape[-1], q.shape[2]
    NT, NS = (tokens + 31) // 32, (tokens + stage - 1) // stage
    scale = 1.0 / math.sqrt(d_h)
    raw = q @ k.transpose(-1, -2)
    p = torch.softmax(raw * scale, dim=-1)
    o = p @ v
    S1 = p @ v.abs()
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    smax = raw.abs().amax(-1, keepdim=True)
    del raw, p
    c2 = scale / LN2
    delta = c2 * ((d_h + 2) * U * A + (17 + 3 * (NS - 1)) * U * smax)
    eta = LN2 * delta + 4 * U + 5 * (NS - 1) * U
    sig = (8 * NT + 2 * NS + 20) * U
    acc = (32 * NT + 16) * U
    e_num = eta + 2.0 ** -8 * (1 + eta) + acc * (1 + 2.0 ** -8)
    e_den = eta + sig
    core = (e_num * S1 + e_den * o.abs()) / (1 - e_den) + 3 * U * (o.abs() + S1)
    return o, 2.0 ** -8 * (o.abs() + core) + core + 1e-30


STREAM_TOKENS = (5, 33, 197, 257, 288, 289, 320, 385, 577, 785, 1025, 2049)


@pytest.mark.parametrize("tokens", STREAM_TOKENS)
def test_stream_operator_vs_float64(eng, gpu, tokens):
    """Every pattern (one per image), slab and dense layouts with NaN pad / guard rows, a sentinel-filled output wider than dim."""
    g = torch.Generator().manual_seed(4242 + tokens)
    heads, n, d_h = 2, len(STREAM_PATTERNS), 64
    dim = heads * d_h
    q, k, v = _inputs(n, tokens, heads, g)
    o, bound = _stream_ref(q.to(gpu), k.to(gpu), v.to(gpu), 128)
    worst = {}
    for group, pad in ((3, 8), (0, 0), (0, 16)):
        idx, rows = _image_rows(n, tokens, group, gpu)
        qkv = _pack_qkv(q, k, v, idx, rows, gpu)
        out = torch.full((rows + GUARD, dim + pad), SENT, dtype=torch.bfloat16, device=gpu)
        eng.attention(qkv, n, tokens, heads, d_h, group=group, out=out, stream=True)
        torch.cuda.synchronize()
        got = out[idx.reshape(-1), :dim].double()
        assert not torch.isnan(got).any(), f"T={tokens} group={group}: NaN in the output"
        written = torch.zeros(rows + GUARD, dim + pad, dtype=torch.bool, device=gpu)
        written[idx.reshape(-1), :dim] = True
        assert bool((out[~written].float() == SENT).all()), f"T={tokens} group={group}: a write outside the image rows / columns"
        ratio = ((got - _to_rows(o)).abs() / _to_rows(bound)).reshape(n, tokens, dim).amax(dim=(1, 2)).cpu()
        for i in range(n):
            pat = STREAM_PATTERNS[i % len(STREAM_PATTERNS)]
            worst[pat] = max(worst.get(pat, 0.0), float(ratio[i]))
    print(f"\n[stream-vs-f64] T={tokens}: max err/bound " + ", ".join(f"{p} {r:.3f}" for p, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("tokens", (197, 577, 1025))
def test_stream_cls_only_vs_float64(eng, gpu, tokens):
    g = torch.Generator().manual_seed(99 + tokens)
    heads, n, d_h = 3, len(STREAM_PATTERNS), 64
    dim = heads * d_h
    q, k, v = _inputs(n, tokens, heads, g)
    o, bound = _stream_ref(q[:, :, :1].to(gpu), k.to(gpu), v.to(gpu), 64)
    o0, b0 = o[:, :, 0, :].reshape(n, dim), bound[:, :, 0, :].reshape(n, dim)
    for group in (3, 0):
        idx, rows = _image_rows(n, tokens, group, gpu)
        qkv = _pack_qkv(q, k, v, idx, rows, gpu)
        qkv[:, :dim] = float("nan")                                          # the CLS form reads q from its compact buffer only
        q_cls = q[:, :, 0, :].reshape(n, dim).to(gpu, torch.bfloat16).contiguous()
        out = torch.full((n + GUARD, dim + 8), SENT, dtype=torch.bfloat16, device=gpu)
        eng.attention(qkv, n, tokens, heads, d_h, group=group, out=out, q_cls=q_cls, stream=True)
        torch.cuda.synchronize()
        got = out[:n, :dim].double()
        assert not torch.isnan(got).any()
        r = float(((got - o0).abs() / b0).max())
        print(f"\n[stream-cls] T={tokens} group={group}: max err/bound {r:.3f}")
        assert r <= 1.0
        assert bool((out[:n, dim:].float() == SENT).all()) and bool((out[n:].float() == SENT).all())


def _logit_tol(ref):
    return 2.0 ** -6 * float(ref.abs().max())


@pytest.mark.parametrize("cfg,layout", [("vit_base_patch16_384_d2", "timm"), ("vit_small_patch8_224_d2", "hf")])
def test_long_sequence_models_vs_oracle(gpu, cfg, layout):
    """The bars of test_gpu_parity.py::test_other_geometries_vs_oracle at 577 / 785 tokens with attn_stream = 1."""
    from oracle import ref_cpu
    from oracle.vit_modules import build_from_flat
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    w = synthetic_weights(cfg, classes=10, seed=8, std=0.03, eps=1e-6 if layout == "timm" else 1e-12, bias_std=0.02)
    model = build_from_flat(w, layout)
    px = torch.randn(3, 3, int(w["img"]), int(w["img"]), generator=torch.Generator().manual_seed(4))
    eng = VitEngine(w, max_images=3, attn_stream=1)
    assert eng.attn_stream == 1 and eng.tokens > 288
    ref = ref_cpu.logits_of(model, px).float()
    got = eng.forward_logits(px.to(gpu)).cpu()
    print(f"\n[long-oracle] {cfg}: logits max|err| {float((got - ref).abs().max()):.4f} (bar {_logit_tol(ref):.4f})")
    assert (got - ref).abs().max() <= _logit_tol(ref)
    refs = ref_cpu.ffn_activation_importance(model, [{"pixel_values": px}], chain="fp32")
    sc = eng.forward_scores(px.to(gpu), "pre_gelu" if layout == "timm" else "post_gelu", "fp32")[0].cpu() / 3
    for l, r in enumerate(refs):
        rel = (sc[l, : r.numel()] - r).abs() / r.abs().clamp_min(1e-3)
        assert float(rel.max()) <= 5e-3 and float(rel.mean()) <= 5e-4, (l, float(rel.max()), float(rel.mean()))
    skip = eng.forward_logits(px.to(gpu), attn_skip=[1]).cpu()
    m2 = copy.deepcopy(model); ref_cpu.bypass_attention_(m2, 1)
    r2 = ref_cpu.logits_of(m2, px).float()
    assert (skip - r2).abs().max() <= _logit_tol(r2)
    eng.close()


def test_stage2_and_apply_at_577_tokens(gpu):
    """One-pass prune (stage-1 scores + depth-search counts) on a 577-token model against the oracle's per-candidate correctness, then
    FFN masks and one dropped attention applied into the pruned twin (which must inherit attn_stream) against the oracle's pruned module."""
    from oracle import ref_cpu
    from oracle.vit_modules import build_from_flat
    from ssp2vit import core, vit_pruning as vp
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    name, depth, d_int, n = "vit_small_patch16_384_d3", 3, 1536, 8
    w = synthetic_weights(name, classes=10, seed=5, std=0.03, eps=1e-6, bias_std=0.02)
    model = build_from_flat(w, "timm")
    px = torch.randn(n, 3, 384, 384, generator=torch.Generator().manual_seed(6))
    ref = ref_cpu.logits_of(model, px).float()
    labels = ref.argmax(-1)
    eng = VitEngine(w, max_images=core.lm_capacity_images(577, depth, n, n), attn_stream=1)
    batches = [{"pixel_values": px, "labels": labels}]
    scores, (base, cand, total) = core.prune_pass(eng, batches, [d_int] * depth, "pre_gelu", depth, score_limit=5, search_limit=5,
                                                  eval_chunk_images=n)
    assert total == n
    refs = ref_cpu.ffn_activation_importance(model, [{"pixel_values": px}], chain="fp32")
    for l, r in enumerate(refs):
        rel = (torch.as_tensor(scores[l]).float().cpu()[: r.numel()] - r).abs() / r.abs().clamp_min(1e-3)
        assert float(rel.max()) <= 5e-3 and float(rel.mean()) <= 5e-4, (l, float(rel.max()), float(rel.mean()))

    def decisive_compare(tag, ref_logits, got_logits, got_count):
        err = float((got_logits - ref_logits).abs().max())
        top2 = ref_logits.topk(2, dim=-1).values
        dec = (top2[:, 0] - top2[:, 1]) > 4 * err
        ok_ref = ref_logits.argmax(-1) == labels
        ok_got = got_logits.argmax(-1) == labels
        assert torch.equal(ok_ref[dec], ok_got[dec]), tag
        assert int(ok_got.sum()) == got_count, (tag, int(ok_got.sum()), got_count)        # the search's count is the forward's
        und = [(int(i), float(top2[i, 0] - top2[i, 1])) for i in torch.nonzero(~dec).flatten()]
        print(f"[577 stage 2] {tag}: correct oracle {int(ok_ref.sum())} engine {got_count}; logit err {err:.4f}; undecided {und}")

    dense = eng.forward_logits(px.to(gpu)).cpu()
    decisive_compare("dense", ref, dense, base)
    for b in range(depth):
        m2 = copy.deepcopy(model); ref_cpu.bypass_attention_(m2, b)
        decisive_compare(f"skip {b}", ref_cpu.logits_of(m2, px).float(), eng.forward_logits(px.to(gpu), attn_skip=[b]).cpu(), cand[b])

    k = 512
    imps = [torch.as_tensor(scores[l]).float().cpu()[:d_int] for l in range(depth)]
    pruned = build_from_flat(w, "timm")
    res = vp.prune_vit_mlp_width(pruned, n_to_prune_per_block=[k] * depth, min_remaining=256, collect_masks=True, precomputed_importance=imps)
    vp._apply_bypass(pruned, 1)
    twin = eng.pruned_twin([d_int - k] * depth, max_images=n)
    assert twin.attn_stream == 1
    eng.apply_into(twin, res["ffn_prune_masks"], [1])
    rp = ref_cpu.logits_of(pruned, px).float()
    got = twin.forward_logits(px.to(gpu)).cpu()
    print(f"[577 apply] pruned twin logits max|err| {float((got - rp).abs().max()):.4f} (bar {_logit_tol(rp):.4f})")
    assert (got - rp).abs().max() <= _logit_tol(rp)
    twin.close(); eng.close()


def test_mode2_against_the_resident_kernels_and_mode1_bit_identical(gpu):
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    w = synthetic_weights("vit_base_patch16_224_d3", classes=10, seed=2, std=0.03, eps=1e-6, bias_std=0.02)
    px = torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(gpu)
    e0 = VitEngine(w, max_images=6, attn_stream=0)
    ref = e0.forward_logits(px).cpu()
    skip0 = e0.forward_logits(px, attn_skip=[2]).cpu()
    e1 = VitEngine(w, max_images=6, attn_stream=1)
    assert torch.equal(e1.forward_logits(px).cpu(), ref)                         # 197 tokens: mode 1 keeps the resident kernels
    e2 = VitEngine(w, max_images=6, attn_stream=2)
    for tag, a, b in (("dense", ref, e2.forward_logits(px).cpu()), ("skip last", skip0, e2.forward_logits(px, attn_skip=[2]).cpu())):
        err = float((a - b).abs().max())
        print(f"\n[mode 2] {tag}: logits max|diff| vs resident {err:.5f} (bar {_logit_tol(a):.4f})")
        assert err <= _logit_tol(a)
        top2 = a.topk(2, dim=-1).values
        dec = (top2[:, 0] - top2[:, 1]) > 2 * _logit_tol(a)
        assert torch.equal(a.argmax(-1)[dec], b.argmax(-1)[dec])
    for e in (e0, e1, e2):
        e.close()


def test_cli_end_to_end_with_long_sequences(gpu, tmp_path, monkeypatch):
    import json
    from ssp2vit._lib import Ssp2Error
    monkeypatch.delenv("SSP2_ATTN_STREAM", raising=False)
    spec = importlib.util.spec_from_file_location("auto_2ssp_amd_long", os.path.join(PKG, "auto_2ssp.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    out = tmp_path / "run"
    args = ["--model", "vit_tiny_patch16_384", "--target", "0.3", "--eval-batches", "2", "--batch-size", "16", "--synthetic-calib", "32",
            "--num-classes", "10", "--min-remaining", "256", "--output-dir", str(out), "--fw-export-prefix", str(out / "fw")]
    rep = cli.main(args + ["--long-sequences"])[0]
    m = rep["metrics"]
    assert {"params_before_stage1", "params_after_stage2", "latency_baseline_ms", "acc_baseline", "acc_stage1", "acc_stage2",
            "total_reduction_percent", "acc_total_drop_percent"} <= set(m)
    plan = rep["plan"]
    assert len(rep["artifacts"]["pruned_block_indices"]) == plan["blocks_to_prune"]
    masks = json.load(open(rep["artifacts"]["ffn_prune_masks_path"]))["ffn_masks"]
    assert len(masks) == 12 and all(sum(r) == plan["per_block_neurons_to_prune"] and len(r) == 768 for r in masks)
    assert any(f.startswith("report-") and f.endswith(".md") for f in os.listdir(out / "reports"))
    from ssp2vit import vit_pruning as vp
    vp.release_engines(free=True)
    with pytest.raises(Ssp2Error, match="--long-sequences") as ei:
        cli.main(args)
    assert "577 tokens" in str(ei.value)
    vp.release_engines(free=True)


def test_fp8_is_refused_on_a_streaming_engine(gpu):
    """fp8 and the key-streaming attention do not combine (the kernel writes no e4m3): set_precision / precision="fp8" refuse it, and
    so does switching a 577-token engine back to the resident kernels."""
    from ssp2vit._lib import Ssp2Error
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    w = synthetic_weights("vit_base_patch16_384_d2", classes=10, seed=1)
    with pytest.raises(Ssp2Error, match="key-streaming"):
        VitEngine(w, max_images=2, precision="fp8", attn_stream=1)
    e = VitEngine(w, max_images=2, attn_stream=1)
    with pytest.raises(Ssp2Error):
        e.set_option("attn_stream", 0)
    with pytest.raises(Ssp2Error, match="key-streaming"):
        e._check(e.lib.ssp2_set_precision(e.h, 1))
    assert e.get_option("attn_stream") == 1
    e.close()
    w2 = synthetic_weights("vit_base_patch16_224_d3", classes=10, seed=1)
    e8 = VitEngine(w2, max_images=2, precision="fp8")
    with pytest.raises(Ssp2Error):
        e8.set_option("attn_stream", 2)
    e8.close()
