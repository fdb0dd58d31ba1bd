#!/usr/bin/env python3
"""Fixture generator — runs ONLY in the build container (needs /root/reference, which never travels).

Imports the real reference (`/root/reference/src/vit_pruning.py`,
`/root/reference/adaptation-for-Pures-framework/mask_conjunction.py`), drives it with the build-owned
duck-typed modules of `oracle/vit_modules.py` on seeded inputs and writes DATA ONLY (inputs + the
reference's outputs) to `tests/golden/*.npz|*.json`.  No reference source text is stored.

    python tests/golden/make_golden.py
    python tests/golden/make_golden.py --properties     # properties_reference.json + ref_head_*.pt of tests/test_properties_cpu.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "2ssp-x-vit_amd"))

REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "adaptation-for-Pures-framework"))  # mask_conjunction + its src/
import mask_conjunction as ref_mc  # noqa: E402
from src import vit_pruning as ref_vp  # noqa: E402

from oracle.vit_modules import build_from_flat, TimmLayoutViT  # noqa: E402
from ssp2vit.weights import synthetic_weights, VIT_CONFIGS  # noqa: E402

torch.set_num_threads(8)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def make_batches(n_batches, bs, img, seed, model=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_batches):
        px = torch.randn(bs, 3, img, img, generator=g)
        out.append({"pixel_values": px})
    if model is not None:  # teacher labels: the dense model's own argmax under the reference's autocast
        for b in out:
            with torch.no_grad(), torch.autocast("cpu", enabled=True):
                o = model(pixel_values=b["pixel_values"]) if hasattr(model, "vit") else model(b["pixel_values"])
            logits = o.logits if hasattr(o, "logits") else o
            b["labels"] = logits.argmax(-1)
    return out


def bits(t: torch.Tensor) -> np.ndarray:
    """bf16 tensors are stored as their raw uint16 bit patterns; fp32 as is."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().astype(np.int16).view(np.uint16)
    return t.numpy()


def tiny_case(layout: str, std: float):
    """Reference smoke-test config (test_stage2_attention_only.py:44-53): img 32, patch 16, d 64, 4 heads,
    d_int 128, 4 layers, 10 labels; 2 batches x 8 images N(0,1)."""
    w = synthetic_weights("vit_test_patch16_32", classes=10, seed=0, std=std, bias_std=0.02,
                          eps=1e-6 if layout == "timm" else 1e-12)
    model = build_from_flat(w, layout)
    batches = make_batches(2, 8, 32, seed=1, model=model)
    # perturb a few teacher labels so the baseline is < 1 and clamping max(0, .) is exercised
    batches[1]["labels"] = batches[1]["labels"].clone()
    batches[1]["labels"][:2] = (batches[1]["labels"][:2] + 1) % 10

    rec = {}
    for k, v in w.items():
        rec["w." + k] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    for i, b in enumerate(batches):
        rec[f"px.{i}"] = b["pixel_values"].numpy()
        rec[f"labels.{i}"] = b["labels"].numpy()

    imps = ref_vp._compute_ffn_activation_importance(model, batches, device="cpu", batch_limit=None)
    assert all(t.dtype == torch.bfloat16 for t in imps)
    for i, t in enumerate(imps):
        rec[f"s1_imp_bf16bits.{i}"] = bits(t)
    imps1 = ref_vp._compute_ffn_activation_importance(model, batches, device="cpu", batch_limit=1)
    for i, t in enumerate(imps1):
        rec[f"s1_imp_limit1_bf16bits.{i}"] = bits(t)

    rec["top1"] = np.float64(ref_vp.evaluate_top1(model, batches, device="cpu"))
    rec["top1_limit1"] = np.float64(ref_vp.evaluate_top1(model, batches, device="cpu", max_batches=1))

    iface = ref_mc.Auto2SSPInterface(model, batches, device="cpu", importance_mode="copy", batch_limit=5)
    rec["att_imp"] = quiet(iface._compute_att_depth_importance).numpy()
    mlp_imp = quiet(iface._compute_mlp_importance)
    for i, t in enumerate(mlp_imp):
        assert torch.equal(t, imps[i])

    # mask step on the CLI's fp32 cast of the scores (auto_2ssp.py:809), two prune counts
    import copy
    for tag, n_prune, min_rem in (("t40", 40, 16), ("t100_clamped", 100, 64)):
        res = quiet(ref_vp.prune_vit_mlp_width, copy.deepcopy(model), n_to_prune_per_block=[n_prune] * 4,
                    min_remaining=min_rem, collect_masks=True,
                    precomputed_importance=[x.to(torch.float32) for x in imps])
        rec[f"mask.{tag}"] = np.asarray(res["ffn_prune_masks"], dtype=np.int16)
        rec[f"pruned_idx.{tag}"] = np.asarray(res["ffn_pruned_indices"], dtype=np.int64)
        pm = res["model"]
        rec[f"top1_after.{tag}"] = np.float64(ref_vp.evaluate_top1(pm, batches, device="cpu"))

    # stage-2 through the function API: copy mode (search) and selected_indices (apply only)
    res = quiet(ref_vp.prune_vit_attention_blocks, copy.deepcopy(model), sparsity=0.5, dataloader=batches,
                device="cpu", batch_limit=5, importance_mode="copy", show_progress=False, num_to_prune=2)
    rec["s2_copy.pruned"] = np.asarray(res["pruned_indices"], dtype=np.int64)
    rec["s2_copy.orig"] = np.float64(res["original_metrics"])
    rec["s2_copy.final"] = np.float64(res["final_metrics"])
    res = quiet(ref_vp.prune_vit_attention_blocks, copy.deepcopy(model), sparsity=0.5, dataloader=None,
                device="cpu", importance_mode="heuristic", show_progress=False, num_to_prune=2)
    rec["s2_heur.pruned"] = np.asarray(res["pruned_indices"], dtype=np.int64)
    sel = [int(i) for i in torch.argsort(torch.from_numpy(rec["att_imp"]))[:2]]
    res = quiet(ref_vp.prune_vit_attention_blocks, copy.deepcopy(model), sparsity=0.5, dataloader=batches,
                device="cpu", batch_limit=5, num_to_prune=2, selected_indices=sel, show_progress=False)
    rec["s2_sel.pruned"] = np.asarray(res["pruned_indices"], dtype=np.int64)
    rec["s2_sel.final"] = np.float64(res["final_metrics"])

    np.savez_compressed(os.path.join(HERE, f"tiny_{layout}.npz"), **rec)
    print(f"[golden] tiny_{layout}: top1={rec['top1']:.4f} att_imp={rec['att_imp'].tolist()} "
          f"s2_copy={rec['s2_copy.pruned'].tolist()} distinct_labels={len(set(torch.cat([b['labels'] for b in batches]).tolist()))}")


def vit_tiny_case():
    """BASELINE.json configs[0]: ViT-Tiny/16, 32 calibration images, stage-1 scoring only, CPU.
    Weights/pixels are regenerated from seeds (22 MB of fp32 is too large to commit)."""
    w = synthetic_weights("vit_tiny_patch16_224", classes=10, seed=0, std=0.02, eps=1e-6)
    model = build_from_flat(w, "timm")
    batches = make_batches(2, 16, 224, seed=1)
    imps = ref_vp._compute_ffn_activation_importance(model, batches, device="cpu")
    rec = {f"s1_imp_bf16bits.{i}": bits(t) for i, t in enumerate(imps)}
    rec["weights_checksum"] = np.float64(sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor)))
    rec["pixels_checksum"] = np.float64(sum(float(b["pixel_values"].double().sum()) for b in batches))
    np.savez_compressed(os.path.join(HERE, "vit_tiny16_stage1.npz"), **rec)
    print("[golden] vit_tiny16_stage1 written; distinct values in block 0:",
          len(set(imps[0].float().tolist())))


def vit_b16_case():
    """BASELINE.json configs[1] geometry at a size the REAL reference finishes in about two minutes on 8 cores:
    ViT-B/16, 1000 classes, fc1 rows spread x[1/4, 4] (the bench's weights), 2 x 32 images.  Stored: the reference's
    bf16 stage-1 scores, the masks its mask step makes of them at the planner's t = 1120 (on the CLI's fp32 cast,
    auto_2ssp.py:809), the teacher labels (dense-model argmax under the reference's autocast), the dense top-1 and the
    depth-importance vector over those 64 images — plus the oracle's fp32-chain scores, so that the GPU test needs no
    CPU forward at this size.  Weights and pixels are regenerated from seeds (346 MB of fp32 is not a fixture)."""
    import copy
    from oracle import ref_cpu
    w = synthetic_weights("vit_base_patch16_224", classes=1000, seed=0, std=0.02, eps=1e-6, spread=4.0)
    model = build_from_flat(w, "timm")
    batches = make_batches(2, 32, 224, seed=1, model=model)
    rec = {"weights_checksum": np.float64(sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor))),
           "pixels_checksum": np.float64(sum(float(b["pixel_values"].double().sum()) for b in batches))}
    for i, b in enumerate(batches):
        rec[f"labels.{i}"] = b["labels"].numpy()
    imps = ref_vp._compute_ffn_activation_importance(model, batches, device="cpu")
    assert all(t.dtype == torch.bfloat16 for t in imps)
    for i, t in enumerate(imps):
        rec[f"s1_imp_bf16bits.{i}"] = bits(t)
    res = quiet(ref_vp.prune_vit_mlp_width, copy.deepcopy(model), n_to_prune_per_block=[1120] * 12, min_remaining=512,
                collect_masks=True, precomputed_importance=[x.to(torch.float32) for x in imps])
    rec["mask.t1120"] = np.packbits(np.asarray(res["ffn_prune_masks"], dtype=np.uint8), axis=1)
    # BASELINE configs[2] sweeps 25 / 37.5 / 50 % from ONE stage-1 pass and ONE search (main.py:152-157 convention): the
    # planner's other two answers for this model are (K, t) = (4, 661) and (7, 1450); same scores, the reference's own mask step
    for t in (661, 1450):
        r2 = quiet(ref_vp.prune_vit_mlp_width, copy.deepcopy(model), n_to_prune_per_block=[t] * 12, min_remaining=512,
                   collect_masks=True, precomputed_importance=[x.to(torch.float32) for x in imps])
        rec[f"mask.t{t}"] = np.packbits(np.asarray(r2["ffn_prune_masks"], dtype=np.uint8), axis=1)
    rec["top1"] = np.float64(ref_vp.evaluate_top1(model, batches, device="cpu"))
    iface = ref_mc.Auto2SSPInterface(model, batches, device="cpu", importance_mode="copy", batch_limit=5)
    rec["att_imp"] = quiet(iface._compute_att_depth_importance).numpy()
    sel = [int(i) for i in torch.argsort(torch.from_numpy(rec["att_imp"]))[:5]]          # auto_2ssp.py:857, K = 5
    rec["s2_selected_k5"] = np.asarray(sorted(sel), dtype=np.int64)
    for K in (4, 7):                                                                     # the sweep's other two depth targets
        rec[f"s2_selected_k{K}"] = np.asarray(sorted(int(i) for i in torch.argsort(torch.from_numpy(rec["att_imp"]))[:K]), dtype=np.int64)
    o32 = ref_cpu.ffn_activation_importance(model, batches, chain="fp32")
    for i, t in enumerate(o32):
        rec[f"oracle_fp32.{i}"] = t.numpy()
    ob = ref_cpu.ffn_activation_importance(model, batches)
    assert all(torch.equal(a, b) for a, b in zip(ob, imps)), "oracle != reference at ViT-B/16"
    np.savez_compressed(os.path.join(HERE, "vit_b16_2x32.npz"), **rec)
    print(f"[golden] vit_b16_2x32: top1={rec['top1']:.4f} att_imp={rec['att_imp'].tolist()} selected={sorted(sel)} "
          f"distinct bf16 scores in block 0: {len(set(imps[0].float().tolist()))}")


def vit_deep_case(name, tag, n_per_batch, targets, layout="timm"):
    """BASELINE.json configs[3] / configs[4] geometries at FULL depth against the REAL reference:
    ViT-L/16 (24 blocks) and ViT-H/14 (32 blocks, patch 14, 257 tokens), 1000 classes, the bench's weights (fc1 rows
    spread x[1/4, 4]), 2 batches of `n_per_batch` images — sized so that ONE stage-1 launch of the two 256-row-aligned
    slabs has >= 4096 rows: the persistent 256 x 256 kernel at K = 1024 / 1280 is then what the GPU test compares, not the
    128 x 128 one.  Stored (data only): the reference's bf16 stage-1 scores, its masks at the planner's t for each target
    (on the CLI's fp32 cast, auto_2ssp.py:809), teacher labels, dense top-1, the depth-importance vector over the
    teacher-labelled images, the argsort selections (auto_2ssp.py:857) — plus the oracle's fp32-chain scores and the
    oracle's dense bf16 logits of the first batch.  Weights / pixels are regenerated from seeds."""
    import copy
    import time
    from oracle import ref_cpu
    from ssp2vit.planner import plan_from_stats, stats_from_shapes
    img, patch, dim, heads, inter, depth = VIT_CONFIGS[name]
    t0 = time.time()
    w = synthetic_weights(name, classes=1000, seed=0, std=0.02, eps=1e-6 if layout == "timm" else 1e-12, spread=4.0)
    model = build_from_flat(w, layout)
    batches = make_batches(2, n_per_batch, img, seed=1, model=model)
    rec = {"weights_checksum": np.float64(sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor))),
           "pixels_checksum": np.float64(sum(float(b["pixel_values"].double().sum()) for b in batches)),
           "n_per_batch": np.int64(n_per_batch), "layout": np.asarray(layout)}
    for i, b in enumerate(batches):
        rec[f"labels.{i}"] = b["labels"].numpy()
    imps = ref_vp._compute_ffn_activation_importance(model, batches, device="cpu")
    assert all(t.dtype == torch.bfloat16 for t in imps)
    for i, t in enumerate(imps):
        rec[f"s1_imp_bf16bits.{i}"] = bits(t)
    print(f"[golden] {tag}: stage 1 done after {time.time() - t0:.0f} s", flush=True)
    n_tok = (img // patch) ** 2 + 1
    plans = [plan_from_stats(stats_from_shapes(dim, depth, inter, 1000, n_tok, patch), s, 512) for s in targets]
    # the reference's own planner on an architecture-shaped module agrees (planner.json pins it; asserted here again)
    with torch.device("meta"):
        meta = TimmLayoutViT(img=img, patch=patch, dim=dim, heads=heads, inter=inter, depth=depth, classes=1000)
    for s, p in zip(targets, plans):
        rp = quiet(ref_vp.plan_2ssp_allocation, meta, s, min_remaining=512)
        assert (rp.blocks_to_prune, rp.per_block_neurons_to_prune) == (p.blocks_to_prune, p.per_block_neurons_to_prune)
    rec["targets"] = np.asarray(targets, dtype=np.float64)
    rec["plan_K"] = np.asarray([p.blocks_to_prune for p in plans], dtype=np.int64)
    rec["plan_t"] = np.asarray([p.per_block_neurons_to_prune for p in plans], dtype=np.int64)
    for p in plans:
        t = p.per_block_neurons_to_prune
        # only the mask step is wanted: hand the reference a one-parameter-per-matrix stand-in?  No — it slices real weights
        # (src/vit_pruning.py:297-311), so it gets a real copy; 1.2 / 2.5 GB each, one at a time
        r = quiet(ref_vp.prune_vit_mlp_width, copy.deepcopy(model), n_to_prune_per_block=[t] * depth, min_remaining=512,
                  collect_masks=True, precomputed_importance=[x.to(torch.float32) for x in imps])
        rec[f"mask.t{t}"] = np.packbits(np.asarray(r["ffn_prune_masks"], dtype=np.uint8), axis=1)
        del r
    rec["top1"] = np.float64(ref_vp.evaluate_top1(model, batches, device="cpu"))
    iface = ref_mc.Auto2SSPInterface(model, batches, device="cpu", importance_mode="copy", batch_limit=5)
    rec["att_imp"] = quiet(iface._compute_att_depth_importance).numpy()
    print(f"[golden] {tag}: depth importance done after {time.time() - t0:.0f} s", flush=True)
    for p in plans:
        K = p.blocks_to_prune
        rec[f"s2_selected_k{K}"] = np.asarray(sorted(int(i) for i in torch.argsort(torch.from_numpy(rec["att_imp"]))[:K]), dtype=np.int64)
    o32 = ref_cpu.ffn_activation_importance(model, batches, chain="fp32")
    for i, t in enumerate(o32):
        rec[f"oracle_fp32.{i}"] = t.numpy()
    ob = ref_cpu.ffn_activation_importance(model, batches)
    assert all(torch.equal(a, b) for a, b in zip(ob, imps)), f"oracle != reference at {name}"
    for i, b in enumerate(batches):          # the oracle's dense logits of every image: the GPU test derives from them which images sit on a near-tie
        rec[f"oracle_logits_bf16bits.{i}"] = bits(ref_cpu.logits_of(model, b["pixel_values"]).to(torch.bfloat16))
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **rec)
    print(f"[golden] {tag}: top1={rec['top1']:.4f} att_imp(images)={[round(float(v) * 2 * n_per_batch) for v in rec['att_imp']]} "
          f"plans={[(int(k), int(t)) for k, t in zip(rec['plan_K'], rec['plan_t'])]} "
          f"distinct bf16 scores in block 0: {len(set(imps[0].float().tolist()))}; {time.time() - t0:.0f} s", flush=True)


# ----------------------------------------------------------------------------------------------------------------------------
# DECISIVE stage-2 fixtures.  With a random classifier head over 1000 classes a random-init ViT's logits are
# flat (max |logit| ~ 2.4, top-2 gaps of a few hundredths): a third of the images sit on a near-tie that ANY implementation's rounding
# decides, so counts could only be compared within a band.  Scaling the head does not help (margins and errors scale alike).  What
# helps is a head DESIGNED on the model's own features, which the reference then runs as it would run any head:
#   * label class of image i (class i):    w = a * unit(f_i - mean f),  bias cancels the mean  -> own logit a |d_i| ~ 3, others ~ +-0.3
#   * distractor class of image i (n + i): the label row + b * v_i, where v_i is the minimum-norm direction with
#         v_i . (f_i under bypass c  -  f_i dense) = 1 for the candidates c that shall flip image i, 0 for the others,
#         v_i . (f_j - f_i) = 0 for the other images j (and, where the dimension allows, v_i . (their bypass shifts) = 0),
#     and a bias that puts it b / 2 BELOW the label on the dense model: under candidate c it ends b / 2 above (flip) or b / 2 below (keep).
#   * every other class: zero row, bias -5.
# The bypass shifts |f_c - f| are 2 .. 19 against a bf16-vs-fp32 feature discrepancy of 0.26 (ViT-L/16), the system is well conditioned
# (|v| ~ 1), so every (pass, image) pair gets a top-2 margin of ~ b / 2 = 1 at |logit| ~ 3-5: 30-60 x the implementations' logit
# differences.  The flip pattern gives every candidate its own count, a few of them equal (the argsort tie rule stays exercised).
# The features come from the ORACLE (test infrastructure) — they only shape the head; every stored expectation is the REAL reference's.
def _head_of(model, layout):
    return model.classifier if layout == "hf" else model.head


def _cls_features(model, layout, px):
    """fp32 copy of what the classifier head receives (the CLS row behind the final LayerNorm) under the reference's autocast."""
    from oracle import ref_cpu
    got = {}
    h = _head_of(model, layout).register_forward_pre_hook(lambda m, inp: got.__setitem__("f", inp[0].detach().float().clone()))
    try:
        with torch.no_grad(), torch.autocast("cpu", enabled=True):
            ref_cpu._call(model, px)
    finally:
        h.remove()
    return got["f"]


def design_decisive_head(model, layout, px, flips, a=0.2, b=2.0):
    """-> (rows f32 [2n, d], bias f32 [2n], report).  flips[c] = the images candidate c shall flip."""
    import copy
    from oracle import ref_cpu
    depth = len(ref_cpu._blocks_of(model))
    F0 = _cls_features(model, layout, px).double()
    n, d = F0.shape
    D = []
    for c in range(depth):
        m = copy.deepcopy(model)
        ref_cpu.bypass_attention_(m, c)
        D.append(_cls_features(m, layout, px).double() - F0)
        del m
    D = torch.stack(D)                                           # [depth, n, d]
    mu = F0.mean(0)
    dd = F0 - mu
    rows = torch.zeros(2 * n, d, dtype=torch.float64); bias = torch.zeros(2 * n, dtype=torch.float64)
    vnorm = []
    cross = False      # "other images' bypass shifts project to zero too" (depth x (n - 1) more equations) was tried: |v| 1 -> 9, and the
                       # implementations' feature differences grow with it (ViT-L/16: logit discrepancy 0.34, margins down to 0.02) — off
    for i in range(n):
        u = dd[i] / dd[i].norm()
        rows[i] = a * u; bias[i] = -a * float(u @ mu)
        A, t = [D[c, i] for c in range(depth)], [1.0 if i in flips[c] else 0.0 for c in range(depth)]
        for j in range(n):
            if j != i:
                A.append(F0[j] - F0[i]); t.append(0.0)
                if cross:
                    for c in range(depth):
                        A.append(D[c, j]); t.append(0.0)
        v = torch.linalg.pinv(torch.stack(A)) @ torch.tensor(t, dtype=torch.float64)
        vnorm.append(float(v.norm()))
        rows[n + i] = rows[i] + b * v
        bias[n + i] = bias[i] - b * float(v @ F0[i]) - b / 2
    return rows.float(), bias.float(), {"v_norm_max": max(vnorm), "bypass_shift_min": float(D.norm(dim=2).min()),
                                        "bypass_shift_max": float(D.norm(dim=2).max()), "cross_constraints": cross}


def install_head(model, layout, rows, bias, classes):
    head = _head_of(model, layout)
    with torch.no_grad():
        head.weight.zero_(); head.bias.fill_(-5.0)
        head.weight[: rows.shape[0]].copy_(rows); head.bias[: bias.shape[0]].copy_(bias)
    assert head.weight.shape[0] == classes


def flip_pattern(depth, n):
    """Candidate c flips k_c images: counts 0 .. ~n/3 in a fixed irregular order, some equal; images dealt with stride 5."""
    ks = [(c * 7 + 3) % (n // 3 + 1) for c in range(depth)]
    return [set(((c * 3 + m * 5) % n) for m in range(ks[c])) for c in range(depth)], ks


def decisive_stage2_case(name, tag, n_per_batch, layout, targets=(0.25, 0.375, 0.5), with_stage1=False):
    """Stage 2 at FULL depth against the REAL reference on a fixture where every (pass, image) pair is decided by a wide margin
    (see the block comment above): the dense top-1, the depth-importance vector and the argsort selections can then be compared
    EXACTLY.  Body weights and pixels as in vit_deep_case / vit_b16_case (regenerated from the seeds, checksummed); stored: the
    designed head rows, labels (= the dense argmax under the reference's autocast = the image's own class), the reference's top-1,
    att_imp and selections, the oracle's per-pair margins and the fp32-vs-bf16 oracle logit discrepancy.  `with_stage1`: also the
    reference's bf16 stage-1 scores and masks + the oracle's fp32-chain scores (a geometry that has no stage-1 fixture yet)."""
    import copy
    import time
    from oracle import ref_cpu
    from ssp2vit.planner import plan_from_stats, stats_from_shapes
    img, patch, dim, heads, inter, depth = VIT_CONFIGS[name]
    t0 = time.time()
    w = synthetic_weights(name, classes=1000, seed=0, std=0.02, eps=1e-6 if layout == "timm" else 1e-12, spread=4.0)
    model = build_from_flat(w, layout).eval()
    g = torch.Generator().manual_seed(1)
    pxs = [torch.randn(n_per_batch, 3, img, img, generator=g) for _ in range(2)]
    px = torch.cat(pxs)
    n = px.shape[0]
    flips, ks = flip_pattern(depth, n)
    rows, bias, rep = design_decisive_head(model, layout, px, flips)
    install_head(model, layout, rows, bias, 1000)
    print(f"[golden] {tag}: head designed after {time.time() - t0:.0f} s: {rep}", flush=True)
    # the oracle's view of every pass: label margin per (pass, image); pass 0 = dense
    def margins(m):
        lg = ref_cpu.logits_of(m, px).float()
        lab = lg[torch.arange(n), torch.arange(n)]
        oth = lg.clone(); oth[torch.arange(n), torch.arange(n)] = -1e9
        return lab - oth.max(1).values, lg
    mg0, lg0 = margins(model)
    with torch.no_grad():
        lg32 = ref_cpu._call(model, px).float()
    disc = float((lg32 - lg0).abs().max())
    mg = [mg0]
    for c in range(depth):
        m = copy.deepcopy(model); ref_cpu.bypass_attention_(m, c)
        mg.append(margins(m)[0]); del m
    mg = torch.stack(mg)                                          # [depth + 1, n]
    min_abs = float(mg.abs().min())
    print(f"[golden] {tag}: smallest |label margin| over {depth + 1} x {n} pairs = {min_abs:.3f}; fp32-vs-bf16 oracle logit discrepancy {disc:.4f}; "
          f"max |logit| {float(lg0.abs().max()):.2f}", flush=True)
    assert bool((mg[0] > 0).all()), "the dense model must take every image's own class"
    assert min_abs >= 0.5 and min_abs >= 8 * disc, "fixture not decisive: adjust a / b"      # VERDICT r04 asked for 4 x the measured logit error
    batches = [{"pixel_values": pxs[i], "labels": torch.arange(i * n_per_batch, (i + 1) * n_per_batch)} for i in range(2)]
    rec = {"weights_checksum": np.float64(sum(float(v.double().sum()) for k, v in w.items() if isinstance(v, torch.Tensor) and not k.startswith("head_"))),
           "pixels_checksum": np.float64(float(px.double().sum())), "n_per_batch": np.int64(n_per_batch), "layout": np.asarray(layout),
           "head_rows": rows.numpy(), "head_bias": bias.numpy(), "rest_bias": np.float32(-5.0),
           "oracle_margins": mg.numpy(), "oracle_fp32_vs_bf16_logit_disc": np.float64(disc), "designed_flips_per_candidate": np.asarray(ks, dtype=np.int64)}
    for i, bt in enumerate(batches):
        rec[f"labels.{i}"] = bt["labels"].numpy()
    # ---- the REAL reference on this model
    rec["top1"] = np.float64(ref_vp.evaluate_top1(model, batches, device="cpu"))
    iface = ref_mc.Auto2SSPInterface(model, batches, device="cpu", importance_mode="copy", batch_limit=5)
    rec["att_imp"] = quiet(iface._compute_att_depth_importance).numpy()
    n_tok = (img // patch) ** 2 + 1
    plans = [plan_from_stats(stats_from_shapes(dim, depth, inter, 1000, n_tok, patch), s_, 512) for s_ in targets]
    rec["plan_K"] = np.asarray([p.blocks_to_prune for p in plans], dtype=np.int64)
    rec["plan_t"] = np.asarray([p.per_block_neurons_to_prune for p in plans], dtype=np.int64)
    for p in plans:
        K = p.blocks_to_prune
        rec[f"s2_selected_k{K}"] = np.asarray(sorted(int(i) for i in torch.argsort(torch.from_numpy(rec["att_imp"]))[:K]), dtype=np.int64)
    assert rec["top1"] == 1.0
    want = np.asarray([float(np.float32(max(0.0, 1.0 - (n - int((mg[c + 1] <= 0).sum())) / n))) for c in range(depth)])
    assert np.allclose(rec["att_imp"], want, atol=1e-7), "the reference's impacts are the oracle margins' flips"
    print(f"[golden] {tag}: reference top1={rec['top1']:.3f} impacts(images)={[int(round(float(v) * n)) for v in rec['att_imp']]} after {time.time() - t0:.0f} s", flush=True)
    if with_stage1:
        imps = ref_vp._compute_ffn_activation_importance(model, batches, device="cpu")
        assert all(t.dtype == torch.bfloat16 for t in imps)
        for i, t in enumerate(imps):
            rec[f"s1_imp_bf16bits.{i}"] = bits(t)
        for p in plans:
            t = p.per_block_neurons_to_prune
            r = quiet(ref_vp.prune_vit_mlp_width, copy.deepcopy(model), n_to_prune_per_block=[t] * depth, min_remaining=512,
                      collect_masks=True, precomputed_importance=[x.to(torch.float32) for x in imps])
            rec[f"mask.t{t}"] = np.packbits(np.asarray(r["ffn_prune_masks"], dtype=np.uint8), axis=1)
            del r
        o32 = ref_cpu.ffn_activation_importance(model, batches, chain="fp32")
        for i, t in enumerate(o32):
            rec[f"oracle_fp32.{i}"] = t.numpy()
        ob = ref_cpu.ffn_activation_importance(model, batches)
        assert all(torch.equal(x, y) for x, y in zip(ob, imps)), f"oracle != reference at {name} ({layout})"
        print(f"[golden] {tag}: stage 1 done after {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **rec)
    print(f"[golden] {tag}: written; {time.time() - t0:.0f} s", flush=True)


def deep_logits_patch(name, tag, layout):
    """Adds the oracle's dense logits of EVERY batch to an existing full-depth fixture (round 4 stored batch 0 only at first)
    without re-running the reference's 25 / 33 passes: weights and pixels are regenerated from the seeds and checked against the
    fixture's checksums, everything else in the file is left as the reference produced it."""
    import math
    from oracle import ref_cpu
    path = os.path.join(HERE, f"{tag}.npz")
    z = dict(np.load(path))
    img = VIT_CONFIGS[name][0]
    nb = int(z["n_per_batch"])
    w = synthetic_weights(name, classes=1000, seed=0, std=0.02, eps=1e-6 if layout == "timm" else 1e-12, spread=4.0)
    assert math.isclose(sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor)), float(z["weights_checksum"]), rel_tol=1e-12)
    model = build_from_flat(w, layout)
    g = torch.Generator().manual_seed(1)
    for i in range(2):
        px = torch.randn(nb, 3, img, img, generator=g)
        lg = ref_cpu.logits_of(model, px).to(torch.bfloat16)
        if i == 0:
            assert np.array_equal(bits(lg), z["oracle_logits_bf16bits.0"]), "regenerated logits differ from the stored ones"
        assert torch.equal(lg.float().argmax(-1), torch.from_numpy(z[f"labels.{i}"])), "teacher labels are the oracle's argmax"
        z[f"oracle_logits_bf16bits.{i}"] = bits(lg)
    np.savez_compressed(path, **z)
    print(f"[golden] {tag}: oracle logits of both batches stored")


def planner_cases():
    """plan_2ssp_allocation known answers on architecture-shaped modules (meta device: only numel is read)."""
    out = []
    cases = []
    for name in ("vit_tiny_patch16_224", "vit_base_patch16_224", "vit_large_patch16_224", "vit_huge_patch14_224"):
        for s in (0.25, 0.375, 0.5):
            cases.append((name, 1000, s, 256 if "tiny" in name else 512, None))
    for s, fb in ((0.1, None), (0.2, None), (0.3, None), (0.4, None), (0.3, 2), (0.05, None), (0.9, None), (0.3, 0)):
        cases.append(("vit_base_patch16_224", 10, s, 512, fb))
    cases.append(("vit_test_patch16_32", 10, 0.3, 16, None))
    cases.append(("vit_test_patch16_32", 10, 0.02, 16, None))
    for name, classes, s, min_rem, fb in cases:
        img, patch, dim, heads, inter, depth = VIT_CONFIGS[name]
        with torch.device("meta"):
            m = TimmLayoutViT(img=img, patch=patch, dim=dim, heads=heads, inter=inter, depth=depth, classes=classes)
        plan = quiet(ref_vp.plan_2ssp_allocation, m, s, min_remaining=min_rem, forced_blocks=fb)
        out.append(dict(model=name, classes=classes, target=s, min_remaining=min_rem, forced_blocks=fb,
                        total_params=int(ref_vp.count_total_params(m)),
                        plan=dict(target_sparsity=plan.target_sparsity, num_blocks_total=plan.num_blocks_total,
                                  blocks_to_prune=plan.blocks_to_prune,
                                  per_block_neurons_to_prune=plan.per_block_neurons_to_prune,
                                  stage2_fraction=plan.stage2_fraction,
                                  estimated_total_removed_params=plan.estimated_total_removed_params,
                                  est_error_params=plan.est_error_params)))
        print(f"[golden] plan {name} C={classes} s={s} fb={fb}: K={plan.blocks_to_prune} "
              f"t={plan.per_block_neurons_to_prune} err={plan.est_error_params}")
    with open(os.path.join(HERE, "planner.json"), "w") as f:
        json.dump(out, f, indent=1)


def heuristic_and_exports():
    out = {}
    for B in (4, 12, 24, 32):
        with torch.device("meta"):
            m = TimmLayoutViT(img=32, patch=16, dim=64, heads=4, inter=128, depth=B, classes=10)
        iface = ref_mc.Auto2SSPInterface(m, None, device="cpu", importance_mode="heuristic")
        out[str(B)] = iface._compute_att_depth_importance().tolist()
    with open(os.path.join(HERE, "heuristic_depth.json"), "w") as f:
        json.dump(out, f)

    # framework export schema (auto_2ssp.py:71-185) on a 2-block toy — written by the reference's own exporter
    sys.path.insert(0, os.path.join(REF, "adaptation-for-Pures-framework"))
    try:
        import importlib
        a2 = importlib.import_module("auto_2ssp")
    except Exception as e:  # transformers/timm/datasets imports at module top may fail: ordinary error, skip
        print("[golden] auto_2ssp import failed (ordinary error, exports fixture skipped):", repr(e)[:200])
        return
    import tempfile
    from types import SimpleNamespace
    with torch.device("cpu"):
        m = build_from_flat(synthetic_weights("vit_test_patch16_32", classes=10, seed=3, std=0.2), "hf")
    m.vit.encoder.layer = m.vit.encoder.layer[:2]
    m.config = SimpleNamespace(hidden_size=4, num_attention_heads=2)
    mlp_imp = [torch.tensor([0.5, 1.5, 0.25]), torch.tensor([2.0, 0.0, 1.0])]
    att_imp = torch.tensor([0.125, 0.0])
    masks = [[0, 0, 1], [0, 1, 0]]
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "fw")
        quiet(a2.build_framework_exports, prefix, m, mlp_imp, att_imp, masks, [1])
        exp = {"inputs": {"mlp_imp": [t.tolist() for t in mlp_imp], "att_imp": att_imp.tolist(),
                          "ffn_masks": masks, "pruned_blocks": [1], "hidden": 4, "heads": 2},
               "scores": json.load(open(prefix + "_scores.json")),
               "masks": json.load(open(prefix + "_masks.json"))}
    with open(os.path.join(HERE, "framework_export.json"), "w") as f:
        json.dump(exp, f, indent=1)
    print("[golden] framework_export.json written")


def artifact_tool_cases():
    """Score/mask JSON tooling: run the reference's stdlib-only scripts on small random leaves."""
    import importlib.util
    import random

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    me = os.path.join(REF, "manual-experiments")
    norm = load(os.path.join(me, "normalize_scores.py"), "ref_normalize")
    agg = load(os.path.join(me, "aggregate_and_mask-summation.py"), "ref_aggregate")
    cons = load(os.path.join(me, "consensus_mask.py"), "ref_consensus")
    rnd = random.Random(5)
    files = []
    for f in range(3):
        leaf = {}
        for b in range(3):
            for j in range(20 if b < 2 else 17):                     # ragged last block
                leaf[f"{b}:{j}"] = round(rnd.random() * (f + 1), 3) if rnd.random() > 0.15 else 0.5   # ties
        files.append(leaf)
    out = {"files": files, "cases": []}
    tree = {"ffn": files[0], "meta": {"name": "x", "vals": [1, 2.5, True, None]}}
    lo, hi = norm.scan_min_max_raw(tree)
    out["normalize"] = {"input": tree, "output": norm.normalize_structure(tree, lo, hi)}
    out["normalize_const"] = {"input": {"a": [2, 2]}, "output": norm.normalize_structure({"a": [2, 2]}, 2.0, 2.0)}
    summed = {}
    for leaf in files:
        for k, v in leaf.items():
            summed[k] = summed.get(k, 0.0) + v
    for frac, rounding, pbk in ((0.25, "round", None), (0.5, "floor", None), (0.3, "ceil", None), (0.3, "round", 4), (0.0, "round", None)):
        m = quiet(agg.make_mask_for_leaf, summed, frac, rounding, pbk)
        out["cases"].append({"kind": "bottom_k", "fraction": frac, "rounding": rounding, "per_block_k": pbk, "mask": m})
    for frac, rounding in ((0.25, "round"), (0.4, "floor"), (0.1, "ceil")):
        m = quiet(cons.consensus_for_path, files, frac, rounding, False)
        out["cases"].append({"kind": "consensus", "fraction": frac, "rounding": rounding, "mask": m})
    try:
        amp = load(os.path.join(REF, "experiments", "vit_pruning", "apply_mask_prune.py"), "ref_apply_mask")
        print("[golden] apply_mask_prune imported")
    except Exception as e:
        print("[golden] apply_mask_prune import failed (ordinary error; load_mask restated from source only):", repr(e)[:120])
    with open(os.path.join(HERE, "artifact_tools.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("[golden] artifact_tools.json written:", len(out["cases"]), "cases")


def preprocess_cases():
    """Input pipeline.  torchvision is not installed; its Resize on PIL images IS `Image.resize`
    (third-party Pillow, importable here), so the resized uint8 images are captured from Pillow itself."""
    from PIL import Image
    rng = np.random.default_rng(21)
    rec = {}
    for tag, (h, w), n in (("cifar", (32, 32), 2), ("nonsquare", (40, 48), 1), ("down", (256, 300), 1)):
        imgs = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
        imgs[0, :4, :4] = 255; imgs[0, -4:, -4:] = 0                  # saturated corners: exercises the 8-bit clip
        out = np.stack([np.asarray(Image.fromarray(im, "RGB").resize((224, 224), Image.BICUBIC)) for im in imgs])
        rec[f"{tag}.in"] = imgs
        rec[f"{tag}.out"] = out
    import PIL
    rec["pillow_version"] = np.asarray(PIL.__version__)
    np.savez_compressed(os.path.join(HERE, "preprocess_pil.npz"), **rec)
    print("[golden] preprocess_pil.npz written (Pillow", PIL.__version__, ")")


def preprocess_axis_cases():
    """Pillow's resampler one axis at a time -> preprocess_pil_axes.npz (tests/preprocess_cases.py holds the lists).  The result along an
    axis depends on that axis's (in, out) alone, so thin strips record it: a 6-line strip resized to (out, 6) runs the horizontal pass
    only, its transpose resized to (6, out) the vertical pass only.  Lines 0-1 uniform bytes, 2-3 noise of 0 / 255 (both clips), 4 all 0,
    5 all 255.  Four small whole images beside them, whose result depends on the 8-bit image between the passes: per geometry one
    uniform, one noise, one with the upper rows 0 and the lower 255."""
    import PIL
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import preprocess_cases as PC
    rng = np.random.default_rng(22)
    rec = {}
    for n_in, n_out in PC.AXIS_PAIRS:
        strip = np.empty((6, n_in, 3), dtype=np.uint8)
        strip[0:2] = rng.integers(0, 256, size=(2, n_in, 3), dtype=np.uint8)
        strip[2:4] = rng.integers(0, 2, size=(2, n_in, 3), dtype=np.uint8) * 255
        strip[4], strip[5] = 0, 255
        rec[f"axis.{n_in}.{n_out}.in"] = strip
        rec[f"axis.{n_in}.{n_out}.h"] = np.asarray(Image.fromarray(strip).resize((n_out, 6), Image.BICUBIC))
        rec[f"axis.{n_in}.{n_out}.v"] = np.asarray(Image.fromarray(np.ascontiguousarray(strip.transpose(1, 0, 2))).resize((6, n_out), Image.BICUBIC))
    for h, w, s in PC.FULL_CASES:
        imgs = np.empty((3, h, w, 3), dtype=np.uint8)
        imgs[0] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        imgs[1] = rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255
        imgs[2, :h // 2], imgs[2, h // 2:] = 0, 255
        rec[f"full.{h}.{w}.{s}.in"] = imgs
        rec[f"full.{h}.{w}.{s}.out"] = np.stack([np.asarray(Image.fromarray(im).resize((s, s), Image.BICUBIC)) for im in imgs])
    rec["pillow_version"] = np.asarray(PIL.__version__)
    path = os.path.join(HERE, "preprocess_pil_axes.npz")
    np.savez_compressed(path, **rec)
    print(f"[golden] preprocess_pil_axes.npz written ({os.path.getsize(path)} bytes, Pillow {PIL.__version__})")


def property_cases(n_planner=60, n_masks=60, n_oracle=25):
    """The reference's outputs on fixed seeded cases of tests/test_properties_cpu.py -> properties_reference.json + ref_head_<kind>.pt.
    The test module builds every case's inputs (imported from there, so both sides build the same ones) and runs the cases as explicit
    examples; tensors are stored as the test's digests of dtype, shape and bits, inputs included (a torch whose module init differs is
    caught instead of compared)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_properties_cpu as P
    rng = np.random.default_rng(20261015)

    def geometry(head_dims):
        return dict(layout=str(rng.choice(["timm", "hf"])), heads=int(rng.choice([1, 2, 4])), head_dim=int(rng.choice(head_dims)))

    out = {"made_by": "the reference's plan_2ssp_allocation, prune_vit_mlp_width, _compute_ffn_activation_importance, evaluate_top1, "
                      "Auto2SSPInterface._compute_att_depth_importance and save_cifar_adapter (tests/golden/make_golden.py --properties)",
           "planner": [], "mask_step": [], "oracle": []}
    for i in range(n_planner):
        a = dict(geometry([4, 8]), inter=int(rng.integers(6, 97)), depth=int(rng.integers(2, 10)), classes=int(rng.choice([3, 10])),
                 target=round(float(rng.uniform(0.02, 0.95)), 4), min_remaining=int(rng.choice([0, 4, 16, 64])),
                 forced=None if i % 2 else int(rng.integers(0, 11)))
        m = P.tiny_model(a["layout"], a["heads"], a["head_dim"], a["inter"], a["depth"], a["classes"], 0)
        plan = quiet(ref_vp.plan_2ssp_allocation, m, a["target"], min_remaining=a["min_remaining"], forced_blocks=a["forced"])
        out["planner"].append({"args": a, "want": dict(plan.__dict__)})
    for i in range(n_masks):
        a = dict(geometry([4, 8]), inter=int(rng.integers(6, 97)), depth=int(rng.integers(2, 10)), classes=int(rng.choice([3, 10])),
                 t=0 if i == 1 else int(rng.integers(0, 201)), min_remaining=int(rng.choice([1, 4, 16])),
                 levels=1 if i == 0 else int(rng.integers(1, 41)), seed=int(rng.integers(0, 10 ** 6)))
        m, imps, ts = P.mask_case(a["layout"], a["heads"], a["head_dim"], a["inter"], a["depth"], a["classes"], a["t"], a["levels"], a["seed"])
        inputs = P.sha(*m.parameters(), *imps)
        res = quiet(ref_vp.prune_vit_mlp_width, m, n_to_prune_per_block=list(ts), min_remaining=a["min_remaining"],
                    precomputed_importance=[x.clone() for x in imps], collect_masks=True, device="cpu")
        out["mask_step"].append({"args": a, "want": {"inputs": inputs, "masks": [list(map(int, x)) for x in res["ffn_prune_masks"]],
                                                     "indices": [list(map(int, x)) for x in res["ffn_pruned_indices"]],
                                                     "params": P.params_sha(res["model"])}})
    torch.set_num_threads(2)                                # the thread count the test runs these forwards with
    for i in range(n_oracle):
        a = dict(geometry([8, 16]), inter=int(rng.integers(8, 81)), depth=1 if i == 2 else int(rng.integers(1, 6)),
                 sizes=[int(x) for x in rng.integers(1, 8, size=int(rng.integers(1, 5)))],
                 limit=0 if i == 0 else None if i % 3 == 1 else int(rng.integers(0, 6)), seed=int(rng.integers(0, 10 ** 6)))
        m, batches = P.oracle_case(a["layout"], a["heads"], a["head_dim"], a["inter"], a["depth"], a["sizes"], a["seed"])
        inputs = P.sha(*m.parameters(), *(t for b in batches for t in (b["pixel_values"], b["labels"])))
        scores = quiet(ref_vp._compute_ffn_activation_importance, m, batches, device="cpu", batch_limit=a["limit"])
        top1 = quiet(ref_vp.evaluate_top1, m, batches, device="cpu", max_batches=a["limit"])
        att = None
        if a["depth"] >= 2:
            iface = ref_mc.Auto2SSPInterface(m, batches, device="cpu", importance_mode="copy", batch_limit=a["limit"] if a["limit"] is not None else 5)
            att = P.sha(quiet(iface._compute_att_depth_importance))
        out["oracle"].append({"args": a, "want": {"inputs": inputs, "scores": [P.sha(s) for s in scores], "top1": float(top1), "att": att}})
    with open(os.path.join(HERE, "properties_reference.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    for kind in ("linear", "adapter"):
        ref_vp.save_cifar_adapter(P.head_source(kind), HERE, f"ref_head_{kind}.pt", extra={"note": 1})
    print(f"[golden] properties_reference.json: {n_planner} planner, {n_masks} mask-step, {n_oracle} oracle cases; ref_head_{{linear,adapter}}.pt")


if __name__ == "__main__":
    if "--properties" in sys.argv:
        property_cases()
        sys.exit(0)
    if "--preprocess-only" in sys.argv:
        preprocess_cases()
        preprocess_axis_cases()
        sys.exit(0)
    if "--b16-only" in sys.argv:
        vit_b16_case()
        sys.exit(0)
    if "--deep-logits-only" in sys.argv:
        deep_logits_patch("vit_large_patch16_224", "vit_l16_2x12", "hf")
        deep_logits_patch("vit_huge_patch14_224", "vit_h14_2x8", "timm")
        sys.exit(0)
    if "--l16" in sys.argv or "--h14" in sys.argv:
        # 12 x 197 = 2364 -> 2560-row slabs, two of them 5120 rows; 8 x 257 = 2056 -> 2304-row slabs, two of them 4608 rows
        if "--l16" in sys.argv:
            vit_deep_case("vit_large_patch16_224", "vit_l16_2x12", 12, (0.25, 0.375, 0.5), layout="hf")
        if "--h14" in sys.argv:
            vit_deep_case("vit_huge_patch14_224", "vit_h14_2x8", 8, (0.25, 0.375, 0.5))
        sys.exit(0)
    if "--decisive" in sys.argv:
        # decisive stage-2 fixtures (designed head): `--decisive b16hf l16 h14` or any subset
        if "b16hf" in sys.argv:     # the reference CLI's default anatomy (HF google/vit-base-patch16-224: post-GELU hook, eps 1e-12) at the headline geometry
            decisive_stage2_case("vit_base_patch16_224", "vit_b16_hf_2x32", 32, "hf", with_stage1=True)
        if "l16" in sys.argv:
            decisive_stage2_case("vit_large_patch16_224", "vit_l16_2x12_s2", 12, "hf")
        if "h14" in sys.argv:
            decisive_stage2_case("vit_huge_patch14_224", "vit_h14_2x8_s2", 8, "timm")
        sys.exit(0)
    if "--artifacts-only" in sys.argv:
        artifact_tool_cases()
        sys.exit(0)
    tiny_case("timm", std=0.25)
    tiny_case("hf", std=0.25)
    vit_tiny_case()
    vit_b16_case()
    planner_cases()
    heuristic_and_exports()
    artifact_tool_cases()
    preprocess_cases()
    preprocess_axis_cases()
