"""Property tests (hypothesis; SURVEY.md §4 test plan item 3) of the host-side rows of §8: planner (f3), mask step (a7 / a8),
stage-2 selection (a9), the dealing of batches over ranks (e).

The REAL reference's outputs on fixed seeded cases — random geometries, scores with ties, clamps, forced block counts and loaders
that the other known-answer fixtures do not reach — are stored in tests/golden/properties_reference.json (written by
`tests/golden/make_golden.py --properties`, the only code that imports the reference).  Every stored case runs as an explicit
example of its test on every box, and there the results must EQUAL the reference's; the generated cases check the invariants.
Derandomised: the same cases on every run; no example database is written.
"""
import hashlib
import json
import os

import pytest
import torch

from conftest import GOLDEN

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import example, given, settings, strategies as st  # noqa: E402

REF_CASES_PATH = os.path.join(GOLDEN, "properties_reference.json")
# absent only while make_golden.py --properties imports this module to write it (test_the_reference_is_really_compared_where_it_exists)
REF_CASES = json.load(open(REF_CASES_PATH)) if os.path.exists(REF_CASES_PATH) else {}
_REF_INDEX = {name: {json.dumps(c["args"], sort_keys=True): c["want"] for c in cases}
              for name, cases in REF_CASES.items() if isinstance(cases, list)}


def reference_cases(name):
    """Decorator: every stored case of `name` as an explicit example of the hypothesis test."""
    def deco(fn):
        for case in REF_CASES.get(name, []):
            fn = example(**case["args"])(fn)
        return fn
    return deco


def reference_output(name, **args):
    """The reference's stored output for this case, or None for a generated case the fixture does not hold."""
    return _REF_INDEX.get(name, {}).get(json.dumps(args, sort_keys=True))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def params_sha(model):
    """One digest of every parameter's name, dtype, shape and bits, in module order (the reference's pruned weights)."""
    h = hashlib.sha256()
    for n, p in model.named_parameters():
        h.update(n.encode() + sha(p).encode())
    return h.hexdigest()


def quiet(fn, *a, **k):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def tiny_model(layout, heads, head_dim, inter, depth, classes, seed):
    from oracle.vit_modules import HFLayoutViT, TimmLayoutViT
    torch.manual_seed(seed)
    cls = TimmLayoutViT if layout == "timm" else HFLayoutViT
    return cls(img=32, patch=16, dim=heads * head_dim, heads=heads, inter=inter, depth=depth, classes=classes).eval()


CFG = settings(max_examples=60, deadline=None, database=None, derandomize=True)
geometry = dict(layout=st.sampled_from(["timm", "hf"]), heads=st.sampled_from([1, 2, 4]), head_dim=st.sampled_from([4, 8]),
                inter=st.integers(6, 96), depth=st.integers(2, 9), classes=st.sampled_from([3, 10]))


@CFG
@given(target=st.floats(0.02, 0.95), min_remaining=st.sampled_from([0, 4, 16, 64]), forced=st.one_of(st.none(), st.integers(0, 10)), **geometry)
@reference_cases("planner")
def test_planner_invariants_and_equality_with_the_reference(layout, heads, head_dim, inter, depth, classes, target, min_remaining, forced):
    """`plan_2ssp_allocation` (reference src/vit_pruning.py:585-769): K stays below the depth, t respects the `min_remaining` clamp, the
    bookkeeping fields are consistent — and on a stored case every field equals the reference's on the same module."""
    from ssp2vit import vit_pruning as vp
    m = tiny_model(layout, heads, head_dim, inter, depth, classes, 0)
    plan = vp.plan_2ssp_allocation(m, target, min_remaining=min_remaining, forced_blocks=forced)
    total = sum(p.numel() for p in m.parameters())
    dim = heads * head_dim
    assert plan.num_blocks_total == depth and 0 <= plan.blocks_to_prune <= depth - 1
    assert 0 <= plan.per_block_neurons_to_prune <= max(0, inter - min_remaining)
    if forced is not None:
        assert plan.blocks_to_prune == max(0, min(depth - 1, forced))
    attn = 4 * dim * dim + 4 * dim
    removed = plan.blocks_to_prune * attn + depth * plan.per_block_neurons_to_prune * (2 * dim + 1)
    assert plan.estimated_total_removed_params == removed
    assert plan.est_error_params == abs(int(round(total * target)) - removed)
    assert plan.stage2_fraction == plan.blocks_to_prune / depth
    want = reference_output("planner", layout=layout, heads=heads, head_dim=head_dim, inter=inter, depth=depth, classes=classes,
                            target=target, min_remaining=min_remaining, forced=forced)
    if want is not None:
        assert plan.__dict__ == want


def mask_case(layout, heads, head_dim, inter, depth, classes, t, levels, seed):
    """(module, importances, per-block prune counts) of one mask-step case."""
    m = tiny_model(layout, heads, head_dim, inter, depth, classes, seed % 7)
    g = torch.Generator().manual_seed(seed)
    imps = [torch.randint(0, levels, (inter,), generator=g).float() for _ in range(depth)]
    ts = [(t + 5 * b) % (inter + 20) for b in range(depth)]          # a different count per block, some beyond the clamp
    return m, imps, ts


@CFG
@given(t=st.integers(0, 200), min_remaining=st.sampled_from([1, 4, 16]), levels=st.integers(1, 40), seed=st.integers(0, 10 ** 6), **geometry)
@reference_cases("mask_step")
def test_mask_step_with_ties_equals_the_reference(layout, heads, head_dim, inter, depth, classes, t, min_remaining, levels, seed):
    """a7 / a8 (reference :256-311) on importances drawn from `levels` distinct values — TIES at the cut are the rule, not the exception —
    with a different count per block, some beyond the `min_remaining` clamp, some zero: exactly n_prune ones per mask, no pruned score
    above a kept one, the compacted fc1 is the kept rows in ascending order, an untouched block has no mask entry — and on a stored
    case masks, index lists and every weight tensor equal the reference's on the same module."""
    from ssp2vit import vit_pruning as vp
    m, imps, ts = mask_case(layout, heads, head_dim, inter, depth, classes, t, levels, seed)
    inputs = sha(*m.parameters(), *imps)
    fc1_before = [p.detach().clone() for n, p in m.named_parameters() if n.endswith(("fc1.weight", "intermediate.dense.weight"))]
    out = quiet(vp.prune_vit_mlp_width, m, n_to_prune_per_block=list(ts), min_remaining=min_remaining, precomputed_importance=[i.clone() for i in imps],
                collect_masks=True, device="cpu")
    drops = [max(0, min(ts[b], inter - min_remaining)) for b in range(depth)]
    pruned_blocks = [b for b in range(depth) if drops[b] > 0]          # a block that loses nothing gets NO mask entry (reference :282-283)
    assert len(out["ffn_prune_masks"]) == len(out["ffn_pruned_indices"]) == len(pruned_blocks)
    fc1_after = [p for n, p in out["model"].named_parameters() if n.endswith(("fc1.weight", "intermediate.dense.weight"))]
    for b in range(depth):
        if drops[b] == 0:
            assert torch.equal(fc1_after[b], fc1_before[b])
    for b, mask, idx in zip(pruned_blocks, out["ffn_prune_masks"], out["ffn_pruned_indices"]):
        mask_t = torch.as_tensor(mask)
        assert int(mask_t.sum()) == drops[b] == len(idx) and sorted(idx) == list(idx)
        assert torch.nonzero(mask_t).flatten().tolist() == list(idx)
        if drops[b] < inter:
            assert float(imps[b][mask_t.bool()].max()) <= float(imps[b][~mask_t.bool()].min())
        assert torch.equal(fc1_after[b], fc1_before[b][~mask_t.bool()])
    want = reference_output("mask_step", layout=layout, heads=heads, head_dim=head_dim, inter=inter, depth=depth, classes=classes, t=t,
                            min_remaining=min_remaining, levels=levels, seed=seed)
    if want is not None:
        assert inputs == want["inputs"], "this torch builds other modules / importances than the one that made the fixture"
        assert want["masks"] == [list(map(int, a)) for a in out["ffn_prune_masks"]]
        assert want["indices"] == [list(map(int, a)) for a in out["ffn_pruned_indices"]]
        assert want["params"] == params_sha(out["model"])


@CFG
@given(depth=st.integers(2, 32), k=st.integers(0, 31), levels=st.integers(1, 6), seed=st.integers(0, 10 ** 6))
def test_stage2_selection_is_the_references_argsort_prefix(depth, k, levels, seed):
    """a9 (reference auto_2ssp.py:857 `torch.argsort(att_imp)[:K]`, applied sorted): with impacts full of ties the selection is what
    `core.select_for_targets` returns for a plan with K blocks — the K lowest impacts, no selected impact above an unselected one."""
    from ssp2vit import core
    from ssp2vit.planner import TwoSSPPlan
    g = torch.Generator().manual_seed(seed)
    impact = (torch.randint(0, levels, (depth,), generator=g).float() / 64.0)
    k = min(k, depth - 1)
    imps = [torch.rand(8, generator=g) for _ in range(depth)]
    plan = TwoSSPPlan(0.3, depth, k, 2, k / depth, 0, 0)
    (sel,) = core.select_for_targets(imps, impact, [plan], min_remaining=1)
    chosen = sel["blocks"]
    want = sorted(int(i) for i in torch.argsort(impact)[:k])
    assert chosen == want and len(set(chosen)) == k
    if 0 < k < depth:
        rest = [i for i in range(depth) if i not in chosen]
        assert float(impact[chosen].max()) <= float(impact[rest].min())
    assert len(sel["masks"]) == depth and all(int(m.sum()) == 2 for m in sel["masks"])


@CFG
@given(n=st.integers(0, 500), batch=st.integers(1, 70), world=st.integers(1, 9), limit=st.one_of(st.none(), st.integers(0, 12)))
def test_batches_are_dealt_to_ranks_without_loss_or_overlap(n, batch, world, limit):
    """§8(e): batch b -> rank b % P.  Over all ranks every item of the first `limit` batches appears exactly once, a rank's batches keep
    the global order, batch b is owned by rank b % P, and only the globally last batch may be ragged."""
    from ssp2vit import dist as D
    per_rank = [D.rank_batch_indices(n, batch, r, world, limit) for r in range(world)]
    n_batches = (n + batch - 1) // batch
    if limit is not None:
        n_batches = min(n_batches, limit)
    flat = sorted(i for rb in per_rank for b in rb for i in b)
    assert flat == list(range(min(n, n_batches * batch)))
    for r, rb in enumerate(per_rank):
        starts = [b[0] for b in rb]
        assert starts == sorted(starts)
        for b in rb:
            gb = b[0] // batch
            assert gb % world == r and D.owns(gb, r, world) and list(b) == list(range(b[0], b[0] + len(b)))
            assert len(b) == batch or gb == (n + batch - 1) // batch - 1
        assert len(rb) == len(range(r, n_batches, world))


def test_the_reference_is_really_compared_where_it_exists():
    """The equality halves above must not vanish silently: the stored reference outputs are there, each test has its cases, and every
    case names exactly the arguments of its test."""
    import inspect
    assert os.path.exists(REF_CASES_PATH)
    for name, fn in (("planner", test_planner_invariants_and_equality_with_the_reference),
                     ("mask_step", test_mask_step_with_ties_equals_the_reference),
                     ("oracle", test_the_oracle_equals_the_reference_on_random_tiny_models)):
        params = set(inspect.signature(fn.hypothesis.inner_test).parameters)
        assert len(REF_CASES[name]) >= 25 and all(set(c["args"]) == params for c in REF_CASES[name]), name
        assert len(_REF_INDEX[name]) == len(REF_CASES[name]), f"{name}: two stored cases with the same arguments"


ORACLE_CFG = settings(max_examples=25, deadline=None, database=None, derandomize=True)


def oracle_case(layout, heads, head_dim, inter, depth, sizes, seed):
    """(module, batches) of one oracle-vs-reference case."""
    m = tiny_model(layout, heads, head_dim, inter, depth, 10, seed % 5)
    g = torch.Generator().manual_seed(seed)
    batches = [{"pixel_values": torch.randn(n, 3, 32, 32, generator=g), "labels": torch.randint(0, 10, (n,), generator=g)} for n in sizes]
    return m, batches


@ORACLE_CFG
@given(layout=st.sampled_from(["timm", "hf"]), heads=st.sampled_from([1, 2, 4]), head_dim=st.sampled_from([8, 16]), inter=st.integers(8, 80),
       depth=st.integers(1, 5), sizes=st.lists(st.integers(1, 7), min_size=1, max_size=4), limit=st.one_of(st.none(), st.integers(0, 5)),
       seed=st.integers(0, 10 ** 6))
@reference_cases("oracle")
def test_the_oracle_equals_the_reference_on_random_tiny_models(layout, heads, head_dim, inter, depth, sizes, limit, seed):
    """§8(c): the oracle (oracle/ref_cpu.py — the checker of every GPU parity test) against the reference ITSELF on geometries and
    loaders the committed fixtures do not hold: both anatomies, 1-5 blocks, ragged batches of 1-7 images, batch limits from 0 (no batch
    at all) upwards.  On a stored case the stage-1 scores in the reference's bf16 chain must be the same BITS and dtype, top-1 the same
    float, the depth-importance vector the same tensor.  On every case the oracle's own consistency is checked: a limit beyond the
    loader changes nothing, a limit of 0 gives zeros."""
    from oracle import ref_cpu
    torch.set_num_threads(2)
    m, batches = oracle_case(layout, heads, head_dim, inter, depth, sizes, seed)
    inputs = sha(*m.parameters(), *(t for b in batches for t in (b["pixel_values"], b["labels"])))
    imps = ref_cpu.ffn_activation_importance(m, batches, batch_limit=limit)
    acc = ref_cpu.evaluate_top1(m, batches, limit)
    assert len(imps) == depth and all(t.shape == (inter,) for t in imps)
    if limit == 0:
        assert all(float(t.abs().sum()) == 0.0 for t in imps) and acc == 0.0
    if limit is not None and limit >= len(sizes):
        again = ref_cpu.ffn_activation_importance(m, batches, batch_limit=None)
        assert all(torch.equal(a, b) for a, b in zip(imps, again))
    want = reference_output("oracle", layout=layout, heads=heads, head_dim=head_dim, inter=inter, depth=depth, sizes=sizes, limit=limit,
                            seed=seed)
    if want is not None:
        assert inputs == want["inputs"], "this torch builds other modules / images than the one that made the fixture"
        assert [sha(t) for t in imps] == want["scores"]                 # digest of dtype, shape and bits
        assert acc == want["top1"]
        if depth >= 2:
            got = ref_cpu.att_depth_importance(m, batches, batch_limit=limit if limit is not None else 5)
            assert sha(got) == want["att"]


def test_the_reference_interface_is_really_compared_where_it_exists():
    """The reference's Auto2SSPInterface made the stored depth-importance vectors: every stored oracle case of two or more blocks has one."""
    cases = REF_CASES["oracle"]
    assert sum(c["args"]["depth"] >= 2 for c in cases) >= 10
    assert all((c["want"]["att"] is not None) == (c["args"]["depth"] >= 2) for c in cases)


def head_source(kind):
    """The HF-layout model whose classifier head the head-file test saves: a Linear head, or the bottleneck adapter."""
    import torch.nn as nn
    src = tiny_model("hf", 2, 8, 24, 2, 10, seed=3)
    if kind == "adapter":
        torch.manual_seed(4)
        src.classifier = nn.Sequential(nn.Linear(16, 5, bias=False), nn.GELU(), nn.Linear(5, 7, bias=True))
        src.config.num_labels = 7
    return src


@pytest.mark.parametrize("kind", ["linear", "adapter"])
def test_classifier_head_files_round_trip_and_are_the_references(kind, tmp_path):
    """save_cifar_adapter / load_cifar_adapter (reference src/vit_pruning.py:774-875, in its `__all__`): the head of an HF-layout model — a
    Linear classifier or the bottleneck adapter Sequential(Linear(bias=False), GELU, Linear) — goes to one file and comes back onto another
    model with the same logits; the file's keys are the reference's; metadata missing from the file is read off the tensors; the three
    RuntimeErrors.  The file the REAL reference wrote for the same head (tests/golden/ref_head_<kind>.pt, make_golden.py --properties)
    holds the same keys, metadata and tensors as THIS build's — what the reference's loader reads — and this loader reads it back."""
    from ssp2vit import vit_pruning as vp
    src = head_source(kind)
    path = vp.save_cifar_adapter(src, str(tmp_path), "head.pt", extra={"note": 1})
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(blob) == sorted(["state_dict", "classifier_type", "num_labels", "hidden_size", "timestamp", "extra"])
    assert blob["classifier_type"] == ("Linear" if kind == "linear" else "Sequential") and blob["extra"] == {"note": 1}
    assert blob["num_labels"] == (10 if kind == "linear" else 7) and blob["hidden_size"] == 16
    dst = tiny_model("hf", 2, 8, 24, 2, 3, seed=9)
    assert vp.load_cifar_adapter(path, dst) is dst and dst.config.num_labels == blob["num_labels"]
    feats = torch.randn(5, 16, generator=torch.Generator().manual_seed(1))
    assert torch.equal(dst.classifier(feats), src.classifier(feats))
    # metadata missing: shapes come from the tensors
    bare = {"state_dict": blob["state_dict"], "classifier_type": blob["classifier_type"]}
    torch.save(bare, tmp_path / "bare.pt")
    again = tiny_model("hf", 2, 8, 24, 2, 3, seed=10)
    vp.load_cifar_adapter(str(tmp_path / "bare.pt"), again)
    assert torch.equal(again.classifier(feats), src.classifier(feats)) and again.config.num_labels == blob["num_labels"]
    # the reference's failures
    torch.save({"state_dict": {}, "classifier_type": "Linear"}, tmp_path / "empty.pt")
    nohid = tiny_model("hf", 2, 8, 24, 2, 3, seed=11); nohid.config.hidden_size = None
    with pytest.raises(RuntimeError, match="hidden size"):
        vp.load_cifar_adapter(str(tmp_path / "empty.pt"), nohid)
    with pytest.raises(RuntimeError, match="num_labels is None"):
        vp.load_cifar_adapter(str(tmp_path / "empty.pt"), tiny_model("hf", 2, 8, 24, 2, 3, seed=12))
    torch.save({"state_dict": {}, "classifier_type": "Sequential"}, tmp_path / "empty_seq.pt")
    with pytest.raises(RuntimeError, match="reconstruct adapter"):
        vp.load_cifar_adapter(str(tmp_path / "empty_seq.pt"), tiny_model("hf", 2, 8, 24, 2, 3, seed=13))
    rpath = os.path.join(GOLDEN, f"ref_head_{kind}.pt")                 # the reference's file of the same head
    rblob = torch.load(rpath, map_location="cpu", weights_only=True)
    assert sorted(rblob) == sorted(blob) and sorted(rblob["state_dict"]) == sorted(blob["state_dict"])
    assert all(torch.equal(rblob["state_dict"][k], blob["state_dict"][k]) for k in blob["state_dict"])
    assert {k: rblob[k] for k in ("classifier_type", "num_labels", "hidden_size", "extra")} == {k: blob[k] for k in ("classifier_type", "num_labels", "hidden_size", "extra")}
    ours = tiny_model("hf", 2, 8, 24, 2, 3, seed=15)
    vp.load_cifar_adapter(rpath, ours)                                      # this build reads the reference's
    assert torch.equal(ours.classifier(feats), src.classifier(feats)) and ours.config.num_labels == blob["num_labels"]
