"""Register tokens and class-free positions on the MI355X: the embedding (cls_row_kernel and both patch-embed epilogues) bit for bit
against the statement of timm's _pos_embed evaluated on the host, with planted defects; engines built through ssp2_create_layout against
engines built through ssp2_create_ext where the layouts coincide; the evaluation tail, the prefix-cached search, the attention skip and
the one-pass prune on the 9- and the 261-token cuts; whole models against the real reference's fixtures (tests/golden/reg_*.npz) and
the CPU restatement of tests/regtoken_models.py; the 1374-token geometry on the key-streaming attention; one fp8 leg; the pruned twin;
the CLI end to end."""
import copy
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import embed_head_cases as EH
from conftest import PKG, ROOT
from regtoken_models import REG_GOLDEN_CASES, bf16_from_bits, build_regtoken, embed_tokens, load_golden

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -7
SENT = -77.0
GUARD = 5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    return torch.device("cuda:0")


def _w(name, seed=3, **kw):
    from ssp2vit.weights import synthetic_weights
    kw.setdefault("std", 0.03)
    kw.setdefault("bias_std", 0.02)
    return synthetic_weights(name, classes=10, seed=seed, **kw)


def _px(n, img, seed=0):
    return torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(seed))


def _layout_engine(w, n, layout, **kw):
    """An engine for `w` whose handle comes from ssp2_create_layout(layout) whatever entry VitEngine itself would have picked."""
    from ssp2vit import _lib
    from ssp2vit.engine import VitEngine
    e = VitEngine(w, max_images=n, **kw)
    old = e.h
    arr = (C.c_int32 * e.depth)(*e.d_int)
    desc = _lib.VitDesc(e.img, e.patch, e.dim, e.heads, e.depth, e.classes, float(e.eps), e.max_images, arr)
    h = C.c_void_p()
    opts = (C.c_int32 * _lib.OPT_COUNT)(*([-1] * _lib.OPT_COUNT))
    e._check(e.lib.ssp2_create_layout(C.byref(desc), opts, C.byref(_lib.TokenLayout(*layout)), C.byref(h)))
    e.h = h
    e._load(w)
    e.lib.ssp2_destroy(old)
    return e


# ------------------------------------------------------------------------------------------------------------ 1. the embedding
def _embed_weights(img, patch, dim, regs, nec, seed=0):
    """A depth-1 flat dictionary of exact-arithmetic operands (tests/embed_head_cases.py: patch weights and pixels in eighths) whose
    prefix parameters and position rows are eighths too and differ from each other by more than 1 everywhere: position row r holds
    2 r + k / 8, register j 100 + 2 j + k / 8, cls -50 + k / 8 (|k| <= 3).  A position row read at another offset or a register written
    to another row then moves a result by far more than an ulp."""
    w = EH.flat_vit(img, patch, dim, EH.heads_of(dim), 10, seed=seed)
    g = torch.Generator().manual_seed(17 + regs + 100 * int(nec) + dim)
    jit = lambda *shape: torch.randint(-3, 4, shape, generator=g).float() / 8.0  # noqa: E731
    patches = (img // patch) ** 2
    P = 1 + regs
    rows = patches if nec else patches + P
    w["pos"] = (2.0 * torch.arange(rows).float()[:, None] + jit(rows, dim)).view(1, rows, dim)
    w["cls"] = (-50.0 + jit(dim)).view(1, 1, dim)
    if regs:
        w["reg"] = (100.0 + 2.0 * torch.arange(regs).float()[:, None] + jit(regs, dim)).view(1, regs, dim)
        w["prefix_tokens"] = P
    if nec:
        w["no_embed_class"] = True
    return w


def _embed_both_paths(eng, px, n, group, what):
    rows = eng.rows(n, group)
    bufs = []
    for lds in (1, 0):
        eng.set_option("patch_lds", lds)
        x = torch.full((rows + GUARD, eng.dim), SENT, dtype=torch.float32, device="cuda")
        assert eng.embed(px, x=x, group=group) is x
        bufs.append(x.cpu())
    eng.set_option("patch_lds", 1)
    assert torch.equal(bufs[0].view(torch.int32), bufs[1].view(torch.int32)), f"{what}: the LDS-staged and the im2col path differ"
    return bufs[0]


def _expected_buffer(stmt, n, tokens, group):
    total, first, pad = EH.embed_layout(n, tokens, group)
    want = torch.full((total + GUARD, stmt.shape[-1]), SENT)
    want[pad] = 0.0
    for t in range(tokens):
        want[first + t] = stmt[:, t]
    return want


def _check_embedding(w, img, patch, ns, what):
    from ssp2vit.engine import VitEngine
    regs = int(w["reg"].shape[1]) if "reg" in w else 0
    nec = bool(w.get("no_embed_class", False))
    P, patches = 1 + regs, (img // patch) ** 2
    eng = VitEngine(w, max_images=max(ns))
    try:
        assert (eng.tokens, eng.prefix_tokens, eng.reg_tokens, eng.no_embed_class) == (patches + P, P, regs, nec)
        for n in ns:
            px = EH.exact_pixels(n, img, seed=patch + n)
            y = EH.embed_y(px, w)
            stmt = embed_tokens(w, y)
            if not regs and not nec:
                assert torch.equal(stmt, EH.embed_statement(px, w))        # today's arithmetic
            pxd = px.cuda()
            for group in (0, (n + 1) // 2):                                 # contiguous; two slabs (the second one shorter when n is odd)
                tag = f"{what} n {n} group {group}"
                want = _expected_buffer(stmt, n, eng.tokens, group)
                assert eng.rows(n, group) + GUARD == want.shape[0], tag
                got = _embed_both_paths(eng, pxd, n, group, tag)
                bad = got.view(torch.int32) != want.view(torch.int32)
                assert not bool(bad.any()), f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[:4].tolist()}"
                # planted defects on the host side: each must miss
                if nec:       # the position row read at prefix + q on a class-free model
                    pos = w["pos"].view(patches, -1)
                    off = stmt.clone()
                    off[:, P:] = y + pos[(torch.arange(patches) + P) % patches]
                    miss = _expected_buffer(off, n, eng.tokens, group) != got
                    assert int(miss.sum()) >= n * patches * eng.dim // 2, tag
                if regs >= 2:  # the register rows in reversed order
                    rev = embed_tokens(dict(w, reg=w["reg"].flip(1)), y)
                    miss = _expected_buffer(rev, n, eng.tokens, group) != got
                    assert int(miss.sum()) >= n * (regs - regs % 2) * eng.dim // 2, tag
    finally:
        eng.close()


@pytest.mark.parametrize("nec", [False, True])
@pytest.mark.parametrize("regs", [0, 1, 2, 4, 8])
def test_embedding_bit_for_bit_vs_the_host_statement(gpu, regs, nec):
    """patch 16 at 32 pixels, dim 64, 32 and 33 images (128 patch rows: one row tile; 132: one row past it), both position forms, both
    patch paths, contiguous and two slabs: the whole buffer — prefix rows, patch rows, zero pad rows, sentinels behind the last row —
    equals the statement of the semantics (tests/regtoken_models.py embed_tokens on the host's bf16 patch embedding), torch.equal."""
    w = _embed_weights(32, 16, 64, regs, nec)
    _check_embedding(w, 32, 16, (32, 33), f"R {regs} class-free {nec}")


def test_embedding_patch14_dim192_bit_for_bit(gpu):
    """patch 14 at 42 pixels (the element-wise pixel gather, 10 K-tiles), dim 192, four registers, class-free: 15 images = 135 patch rows."""
    w = _embed_weights(42, 14, 192, 4, True)
    _check_embedding(w, 42, 14, (15,), "p14 R 4 class-free")


@pytest.mark.parametrize("kind", ["plain", "distilled", "distilled_cls_head"])
def test_layouts_of_create_ext_give_the_same_bits_through_create_layout(gpu, kind):
    """R = 0 with positions for every token, and the distilled layout (row 1 from `dist`): an engine whose handle comes from
    ssp2_create_layout equals one built through ssp2_create_ext / ssp2_create_opts bit for bit — embedding on both patch paths, stage-1
    scores, tail logits."""
    from ssp2vit.engine import VitEngine
    name = "vit_test_patch16_32" if kind == "plain" else "deit_test_distilled_patch16_32"
    w = _w(name)
    if kind == "distilled_cls_head":
        w = {k: v for k, v in w.items() if not k.startswith("head_dist")}
    layout = {"plain": (1, 0, 0, 1), "distilled": (2, 1, 0, 1), "distilled_cls_head": (2, 0, 0, 1)}[kind]
    a, b = VitEngine(w, max_images=33), _layout_engine(w, 33, layout)
    px = _px(33, 32, seed=1).to(gpu)
    for group in (0, 17):
        xa, xb = _embed_both_paths(a, px, 33, group, kind), _embed_both_paths(b, px, 33, group, kind)
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), (kind, group)
    assert torch.equal(a.forward_scores(px, "pre_gelu"), b.forward_scores(px, "pre_gelu"))
    assert torch.equal(a.forward_logits(px), b.forward_logits(px))
    a.close(); b.close()


def test_set_reg_tokens_and_tensor_counts_are_checked_on_a_live_handle(gpu):
    """ssp2_set_reg_tokens refuses a count other than the engine's R and a null pointer (SSP2_EINVAL, nothing dereferenced); an engine
    without registers refuses every count; SSP2_T_POS takes patches * dim floats on a class-free engine and tokens * dim otherwise;
    SSP2_T_DIST is refused on a register engine; ssp2_embed answers SSP2_ESTATE while the registers were never set."""
    from ssp2vit import _lib
    from ssp2vit.engine import VitEngine
    w = _w("vit_test_patch16_32_reg4")
    e = VitEngine(w, max_images=4)
    px = _px(4, 32).to(gpu)
    before = e.embed(px).clone()
    fake = C.c_void_p(0x1000)
    for count, ptr in ((3, fake), (5, fake), (0, fake), (-1, fake), (4, None)):
        assert e.lib.ssp2_set_reg_tokens(e.h, ptr, count, 1) == -1, count
        assert e.lib.ssp2_last_error()
    pos_kind, dist_kind = _lib.T_KINDS.index("pos"), _lib.T_KINDS.index("dist")
    buf = torch.zeros(9 * 64)
    fp = C.cast(buf.data_ptr(), C.POINTER(C.c_float))
    assert e.lib.ssp2_load_tensor(e.h, pos_kind, 0, fp, 9 * 64) == -1           # class-free: 4 rows, not 9
    assert e.lib.ssp2_load_tensor(e.h, dist_kind, 0, fp, 64) == -1
    assert torch.equal(e.embed(px), before)
    plain = VitEngine(_w("vit_test_patch16_32"), max_images=4)
    assert plain.lib.ssp2_set_reg_tokens(plain.h, fake, 4, 1) == -1 and plain.lib.ssp2_set_reg_tokens(plain.h, fake, 0, 1) == -1
    assert plain.lib.ssp2_load_tensor(plain.h, pos_kind, 0, fp, 4 * 64) == -1   # positions for every token: 5 rows, not 4
    plain.close()
    # never set: ESTATE
    arr = (C.c_int32 * e.depth)(*e.d_int)
    desc = _lib.VitDesc(e.img, e.patch, e.dim, e.heads, e.depth, e.classes, float(e.eps), 4, arr)
    h = C.c_void_p()
    e._check(e.lib.ssp2_create_layout(C.byref(desc), None, C.byref(_lib.TokenLayout(5, 0, 4, 0)), C.byref(h)))
    keep = []
    for k in ("patch_w", "patch_b", "cls", "pos"):
        t = w[k].contiguous().float(); keep.append(t)
        e._check(e.lib.ssp2_load_tensor(h, _lib.T_KINDS.index(k), 0, C.cast(t.data_ptr(), C.POINTER(C.c_float)), t.numel()))
    x = e.new_x(4)
    assert e.lib.ssp2_embed(h, C.c_void_p(px.data_ptr()), 4, C.c_void_p(x.data_ptr()), 0) == -4
    assert b"register tokens" in e.lib.ssp2_last_error()
    e.lib.ssp2_destroy(h)
    e.close()


# ------------------------------------------------------------------------------------------------------- 2. tail and search
CUTS = ["vit_test_patch16_32_reg4", "vit_test_patch16_32_reg2_pe", "vit_small_patch14_reg4_dinov2_224_d2"]


@pytest.mark.parametrize("name", CUTS)
def test_tail_is_bit_identical_to_the_full_last_block(gpu, name):
    """The evaluation tail carries ONE row per image however many registers there are (the head reads row 0) and equals the full last
    block followed by head(), bit for bit: contiguous and slab layout, with and without the last attention."""
    from ssp2vit.engine import VitEngine
    w = _w(name)
    n, img = 12, int(w["img"])
    e = VitEngine(w, max_images=3 * n)
    px = _px(n, img, seed=2).to(gpu)
    labels = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(1)).to(gpu)
    L = e.depth
    for group in (0, 4):
        for skip in (None, [L - 1]):
            x = e.embed(px, group=group)
            e.layers(x, n, 0, L - 1, score_group=group)
            x_in = x.clone()
            lt, pt, ct = e.tail(x, n, attn_skip=skip, labels=labels, want_logits=True, want_pred=True, group=group)
            assert torch.equal(x, x_in)
            e.layers(x, n, L - 1, L, attn_skip=skip, score_group=group)
            lf, pf, cf = e.head(x, n, labels=labels, want_logits=True, want_pred=True, group=group)
            torch.cuda.synchronize()
            assert torch.equal(lt, lf) and torch.equal(pt, pf) and torch.equal(ct, cf), (name, group, skip)
    e.close()


@pytest.mark.parametrize("name", ["vit_test_patch16_32_reg4", "vit_small_patch14_reg4_dinov2_224_d2"])
def test_search_equals_full_reruns_and_one_pass_equals_two(gpu, name):
    """As integers and score bits: the prefix-cached search (core.depth_search_counts) equals one full forward per candidate; an attention
    skip equals an engine whose out-projection of that block is zero (x + ls1 * 0 = x); core.prune_pass equals core.stage1_scores +
    core.depth_search_counts for both score chains."""
    from ssp2vit import core
    from ssp2vit.engine import VitEngine
    w = _w(name, seed=4, std=0.04, spread=4.0)
    depth, d_int, img = int(w["depth"]), int(w["fc1_w.0"].shape[0]), int(w["img"])
    bsz = 8
    T = (img // int(w["patch"])) ** 2 + int(w["prefix_tokens"])
    eng = VitEngine(w, max_images=core.lm_capacity_images(T, depth, 2 * bsz, bsz))
    assert eng.tokens == T
    g = torch.Generator().manual_seed(31)
    batches = []
    for n in (bsz, bsz, bsz - 3):
        px = torch.randn(n, 3, img, img, generator=g)
        x = eng.embed(px.cuda()); eng.layers(x, n)
        lb = eng.head(x, n, want_pred=True)[1].long().cpu()
        lb[::3] = (lb[::3] + 1) % 10
        batches.append({"pixel_values": px, "labels": lb})
    base, cand, total = core.depth_search_counts(eng, batches, depth, batch_limit=None, chunk_images=2 * bsz)
    assert total == 3 * bsz - 3 and 0 < base < total

    def count(e, skip):
        c = 0
        for b in batches:
            n = int(b["labels"].numel())
            x = e.embed(b["pixel_values"].cuda()); e.layers(x, n, attn_skip=skip)
            c += int(e.head(x, n, labels=b["labels"])[2].item())
        return c
    assert count(eng, None) == base
    for blk in range(depth):
        assert count(eng, [blk]) == cand[blk], (name, blk)
        wz = dict(w)
        wz[f"proj_w.{blk}"] = torch.zeros_like(w[f"proj_w.{blk}"]); wz[f"proj_b.{blk}"] = torch.zeros_like(w[f"proj_b.{blk}"])
        z = VitEngine(wz, max_images=bsz)
        px = batches[0]["pixel_values"].cuda()
        assert torch.equal(z.forward_logits(px), eng.forward_logits(px, attn_skip=[blk])), (name, blk)
        z.close()
    same = lambda a, b: len(a) == len(b) and all(p.dtype == q.dtype and torch.equal(p, q) for p, q in zip(a, b))  # noqa: E731
    d_ints = [d_int] * depth
    for chain in ("fp32", "bf16_ref"):
        for s_lim, q_lim, chunk in ((None, None, 2 * bsz), (2, 3, bsz)):
            ref_s = core.stage1_scores(eng, batches, d_ints, "pre_gelu", batch_limit=s_lim, score_chain=chain, chunk_images=2 * bsz)
            ref_c = core.depth_search_counts(eng, batches, depth, batch_limit=q_lim, chunk_images=chunk)
            got_s, got_c = core.prune_pass(eng, batches, d_ints, "pre_gelu", depth, score_limit=s_lim, search_limit=q_lim,
                                           score_chain=chain, chunk_images=2 * bsz, eval_chunk_images=chunk)
            assert same(got_s, ref_s), (name, chain, s_lim, q_lim)
            assert got_c == ref_c, (name, chain, s_lim, q_lim, got_c, ref_c)
    eng.close()


# ------------------------------------------------------------------------------ 3. the reference's fixtures and the restatement
def _check_logits(got, ref, tag):
    err = float((got.float() - ref.float()).abs().max())
    top = float(ref.float().abs().max())
    print(f"[reg-logits] {tag}: max |err| {err:.3e}, largest logit {top:.3e} ({err / (BF16_ULP * top):.2f} bf16 ulp of it)")
    assert err <= 2 * BF16_ULP * top, tag


@pytest.mark.parametrize("name", CUTS + ["deit3_small_patch16_224_d2"])
def test_dense_logits_and_stage1_scores_vs_the_cpu_restatement(gpu, name):
    """The engine built from the live CPU module against the module under CPU autocast: logits within 2 bf16 ulp of the largest logit;
    stage-1 scores (summed over all tokens, registers included), bf16 chain <= 2 ulp and >= 90 % identical, fp32 chain within
    rel 2e-3 + 1e-4."""
    from oracle import ref_cpu
    from ssp2vit import vit_pruning as vp, weights as W
    from ssp2vit.engine import VitEngine
    w = _w(name, seed=5)
    model = build_regtoken(w)
    flat = W.from_module(model)
    assert W.reg_tokens_of(flat) == W.REG_TOKENS.get(name, 0) and bool(flat.get("no_embed_class", False)) == (name in W.NO_EMBED_CLASS)
    n, img = 16, int(w["img"])
    px = _px(n, img, seed=7)
    e = VitEngine(flat, max_images=n)
    got = e.forward_logits(px.to(gpu)).cpu()
    ref = ref_cpu.logits_of(model, px).float()
    _check_logits(got, ref, name)
    batches = [{"pixel_values": px[:8]}, {"pixel_values": px[8:]}]
    for chain in ("bf16_ref", "fp32"):
        got_s = vp._compute_ffn_activation_importance(model, batches, device="cuda", score_chain=chain)
        ref_s = ref_cpu.ffn_activation_importance(model, batches, chain="autocast" if chain == "bf16_ref" else "fp32")
        for l, (a, r) in enumerate(zip(got_s, ref_s)):
            if chain == "bf16_ref":
                ulp = (a.cpu().view(torch.int16).int() - r.to(torch.bfloat16).view(torch.int16).int()).abs()
                print(f"[reg-scores] {name} block {l}: max {int(ulp.max())} ulp, {float((ulp == 0).float().mean()):.3f} identical")
                assert int(ulp.max()) <= 2 and float((ulp == 0).float().mean()) >= 0.9, (name, l, int(ulp.max()))
            else:
                rel = float(((a.cpu() - r).abs() / (2e-3 * r.abs() + 1e-4)).max())
                print(f"[reg-scores] {name} block {l}: fp32 chain, largest error {rel:.3f} of the bar rel 2e-3 + 1e-4")
                assert torch.allclose(a.cpu(), r, rtol=2e-3, atol=1e-4), (name, l)
    vp.release_engines(free=True)
    e.close()


@pytest.mark.parametrize("tag", list(REG_GOLDEN_CASES))
def test_engine_vs_the_reference_fixtures(gpu, tag):
    """The engine on the live duck module against the REAL reference's outputs (tests/golden/make_golden_regtokens.py): bf16 stage-1
    scores <= 2 ulp and >= 90 % identical; dense logits within 2 bf16 ulp of the largest logit; per image, top-1 correctness equal
    wherever the stored logits' margin decides it; each block's impact equal wherever the stored margins decide every image; the K
    selection equal when every impact is decided; the masks at the stored plan identical in every block whose cut the stored scores
    guarantee (ssp2vit.mask_parity) — every block of every fixture (weak_neurons)."""
    import numpy as np
    from ssp2vit import vit_pruning as vp
    from ssp2vit.mask_conjunction import Auto2SSPInterface
    from ssp2vit.mask_parity import mask_parity_report
    w, batches, z = load_golden(tag)
    model = build_regtoken(w)
    depth = int(w["depth"])
    t, min_rem, K = REG_GOLDEN_CASES[tag][3:6]
    imps = vp._compute_ffn_activation_importance(model, batches, device="cuda", score_chain="bf16_ref")
    ref_masks = np.unpackbits(z[f"mask.t{t}"], axis=1)
    res = vp.prune_vit_mlp_width(build_regtoken(w), n_to_prune_per_block=[t] * depth, min_remaining=min_rem, collect_masks=True,
                                 precomputed_importance=[a.float().cpu() for a in imps])
    report = mask_parity_report([bf16_from_bits(z[f"s1_imp_bf16bits.{l}"]).float() for l in range(depth)], [t] * depth, min_rem, eps=2.0 ** -5)
    for l, a in enumerate(imps):
        r = bf16_from_bits(z[f"s1_imp_bf16bits.{l}"])
        ulp = (a.cpu().view(torch.int16).int() - r.view(torch.int16).int()).abs()
        print(f"[reg-golden] {tag} block {l}: scores max {int(ulp.max())} ulp, {float((ulp == 0).float().mean()):.3f} identical")
        assert int(ulp.max()) <= 2 and float((ulp == 0).float().mean()) >= 0.9, (tag, l)
        same = np.array_equal(np.asarray(res["ffn_prune_masks"][l], dtype=np.uint8), ref_masks[l, :r.numel()])
        print(f"[reg-golden] {tag} block {l}: mask identical {same} (guaranteed: {report['blocks'][l]['guaranteed']}, "
              f"cut margin {report['blocks'][l]['cut_margin']:.3f})")
        if report["blocks"][l]["guaranteed"]:
            assert same, (tag, l)
    assert report["blocks_guaranteed"] == depth, report

    def decided(key_fmt):
        out = []
        for i in range(len(batches)):
            ref = bf16_from_bits(z[key_fmt.format(i=i)]).float()
            top2 = ref.topk(2, -1).values
            out.append(((top2[:, 0] - top2[:, 1]) > 2 * (2 * BF16_ULP * ref.abs().max()), ref))
        return out

    e = vp.engine_for(model, "cuda", max_images=32)
    assert e.reg_tokens == (int(w["reg"].shape[1]) if "reg" in w else 0) and e.no_embed_class == bool(w.get("no_embed_class", False))
    N = sum(int(b["labels"].numel()) for b in batches)

    def check_model(key_fmt, skip, tag_):
        lo = 0; und = 0
        for i, (b, (dec, ref)) in enumerate(zip(batches, decided(key_fmt))):
            got = e.forward_logits(b["pixel_values"].to(gpu), attn_skip=skip).cpu()
            _check_logits(got, ref, f"{tag} {tag_} batch {i} vs the reference")
            ok_ref, ok_got = ref.argmax(-1) == b["labels"], got.argmax(-1) == b["labels"]
            assert torch.equal(ok_ref[dec], ok_got[dec]), (tag, tag_, i)
            lo += int((ok_ref & dec).sum()); und += int((~dec).sum())
        return lo / N, (lo + und) / N

    blo, bhi = check_model("logits_bf16bits.{i}", None, "dense")
    top1 = vp.evaluate_top1(model, batches, device="cuda", progress=False)
    print(f"[reg-golden] {tag}: top1 engine {top1} reference {float(z['top1'])}, decided interval [{blo}, {bhi}]")
    assert blo <= top1 <= bhi and blo <= float(z["top1"]) <= bhi
    att, _ = Auto2SSPInterface(model, batches, device="cuda", importance_mode="copy", batch_limit=5).fit()
    att = att.float().cpu()
    ref_att = torch.from_numpy(z["att_imp"])
    all_dec = True
    for blk in range(depth):
        plo, phi = check_model(f"bypass_logits_bf16bits.{blk}.{{i}}", [blk], f"attention {blk} bypassed")
        ilo, ihi = max(0.0, blo - phi), max(0.0, bhi - plo)
        print(f"[reg-golden] {tag} block {blk}: impact engine {float(att[blk])} reference {float(ref_att[blk])}, decided interval [{ilo}, {ihi}]")
        assert ilo - 1e-6 <= float(att[blk]) <= ihi + 1e-6, (tag, blk)
        all_dec = all_dec and ilo == ihi
    sel = sorted(int(i) for i in torch.argsort(att)[:K])
    print(f"[reg-golden] {tag}: selection engine {sel} reference {z[f's2_selected_k{K}'].tolist()} (every impact decided: {all_dec})")
    srt = ref_att.sort().values
    if all_dec and float(srt[K - 1]) < float(srt[K]):               # (a tie across the cut would leave the selection to the sort's order)
        assert sel == z[f"s2_selected_k{K}"].tolist()
    vp.release_engines(free=True)


# ------------------------------------------------------------------------------------------------------- 4. 1374 tokens
def test_1374_tokens_on_the_streaming_attention_vs_the_restatement(gpu):
    """vit_small_patch14_reg4_dinov2 cut to two blocks at 518 pixels: 1374 tokens on the key-streaming kernels (attn_stream=1, refused
    by name without it), 2 images; logits (through the streaming tail) and the logits with one attention bypassed within the
    long-sequence bar of tests/test_long_sequence_gpu.py (2^-6 of the largest logit), fp32-chain scores rel max 5e-3 / mean 5e-4."""
    from oracle import ref_cpu
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch14_reg4_dinov2_d2", seed=12, std=0.02)
    model = build_regtoken(w)
    n, px = 2, _px(2, 518, seed=13)
    with pytest.raises(Exception, match="SSP2_OPT_ATTN_STREAM"):
        VitEngine(w, max_images=n, attn_stream=0)
    e = VitEngine(w, max_images=n, attn_stream=1)
    assert e.tokens == 1374 and e.reg_tokens == 4 and e.no_embed_class
    for skip in (None, [1]):
        m = model
        if skip:
            m = copy.deepcopy(model); ref_cpu.bypass_attention_(m, 1)
        ref = ref_cpu.logits_of(m, px).float()
        got = e.forward_logits(px.to(gpu), attn_skip=skip).cpu()
        err, bar = float((got - ref).abs().max()), 2.0 ** -6 * float(ref.abs().max())
        print(f"[reg-long] skip {skip}: logits max |err| {err:.4f} (bar {bar:.4f})")
        assert err <= bar, skip
    sc = e.forward_scores(px.to(gpu), "pre_gelu", "fp32")[0].cpu() / n
    for l, r in enumerate(ref_cpu.ffn_activation_importance(model, [{"pixel_values": px}], chain="fp32")):
        rel = (sc[l, :r.numel()] - r).abs() / r.abs().clamp_min(1e-3)
        print(f"[reg-long] block {l}: scores rel max {float(rel.max()):.2e} mean {float(rel.mean()):.2e}")
        assert float(rel.max()) <= 5e-3 and float(rel.mean()) <= 5e-4, (l, float(rel.max()), float(rel.mean()))
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 5. fp8
def test_fp8_register_cut_tracks_the_bf16_engine(gpu):
    """The 261-token cut in fp8 mode within the existing fp8 bars: logits rel L2 <= 0.15, stage-1 scores mean rel <= 2 % / max <= 10 %,
    masks >= 95 % identical at a quarter pruned."""
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch14_reg4_dinov2_224_d2", seed=8, spread=4.0)
    d_int = int(w["fc1_w.0"].shape[0])
    n = 32                                                          # 8352 token rows: the e4m3 projections
    ref = VitEngine(w, max_images=n)
    f8 = VitEngine(w, max_images=n, precision="fp8")
    px = _px(n, 224, seed=4).to(gpu)
    lr, l8 = ref.forward_logits(px).cpu(), f8.forward_logits(px).cpu()
    rel = float((l8 - lr).norm() / lr.norm())
    sr, s8 = ref.forward_scores(px, "pre_gelu")[0].cpu(), f8.forward_scores(px, "pre_gelu")[0].cpu()
    err = (s8[:, :d_int] - sr[:, :d_int]).abs() / sr[:, :d_int].abs().clamp_min(1e-6)
    t = d_int // 4

    def cut(sc):
        m = torch.zeros(d_int, dtype=torch.bool)
        m[sc.argsort()[:t]] = True
        return m
    same = min(float((cut(sr[l, :d_int]) == cut(s8[l, :d_int])).float().mean()) for l in range(2))
    print(f"[reg-fp8] logits rel {rel:.4f}; scores rel mean {float(err.mean()):.4f} max {float(err.max()):.4f}; masks identical {same:.4f}")
    assert not torch.equal(l8, lr)
    assert rel <= 0.15 and float(err.mean()) <= 0.02 and float(err.max()) <= 0.10 and same >= 0.95
    ref.close(); f8.close()


# ---------------------------------------------------------------------------------------------------------- 6. pruned twin
@pytest.mark.parametrize("name", ["vit_test_patch16_32_reg4", "vit_small_patch14_reg4_dinov2_224_d2"])
def test_apply_into_twin_equals_an_engine_of_the_host_sliced_weights(gpu, name):
    """Width masks + a dropped attention applied into a pruned twin (which inherits the layout and gets the registers by the clone) give
    the logits, bit for bit, of an engine built from weights sliced on the host; cloning into a plain engine of the same geometry, or
    one that differs in the position form only, is refused."""
    from ssp2vit.engine import VitEngine
    w = _w(name, seed=6)
    depth, d_int, img = int(w["depth"]), int(w["fc1_w.0"].shape[0]), int(w["img"])
    g = torch.Generator().manual_seed(2)
    masks = []
    for l in range(depth):
        m = torch.zeros(d_int, dtype=torch.int64)
        m[torch.randperm(d_int, generator=g)[:d_int // 4]] = 1
        masks.append(m)
    n, px = 8, _px(8, img, seed=4).to(gpu)
    dense = VitEngine(w, max_images=n)
    twin = dense.pruned_twin([d_int - d_int // 4] * depth, max_images=n)
    assert (twin.reg_tokens, twin.no_embed_class, twin.prefix_tokens, twin.tokens) == (4, True, 5, dense.tokens)
    assert twin.layer_scale == dense.layer_scale and twin.geometry_key()[-2:] == (4, True)
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
    assert not torch.equal(a, dense.forward_logits(px))
    # the clone refuses engines whose layouts differ: registers against none (other token counts are another architecture already at
    # the Python level, so the plain engine here is given the same image size), and class-free against positions for every token
    plain = {k: v for k, v in w.items() if k not in ("reg", "prefix_tokens", "no_embed_class")}
    plain["pos"] = torch.zeros(1, (img // int(w["patch"])) ** 2 + 1, int(w["dim"]))
    p = VitEngine(plain, max_images=n)
    assert dense.lib.ssp2_clone_weights(p.h, dense.h) == -1 and b"token layouts differ" in dense.lib.ssp2_last_error()
    pe = dict(w, pos=torch.zeros(1, dense.tokens, int(w["dim"])))
    del pe["no_embed_class"]
    q = VitEngine(pe, max_images=n)
    assert dense.lib.ssp2_clone_weights(q.h, dense.h) == -1 and b"pos_prefix_rows" in dense.lib.ssp2_last_error()
    with pytest.raises(Exception, match="token layouts differ"):
        dense.reload(pe)
    for e in (dense, twin, host, p, q):
        e.close()


# ----------------------------------------------------------------------------------------------- 7. API and CLI end to end
def test_reference_api_and_export_on_a_live_register_module(gpu, tmp_path):
    from oracle import ref_cpu
    from ssp2vit import export, vit_pruning as vp, weights as W
    from ssp2vit.engine import VitEngine
    from ssp2vit.mask_conjunction import Auto2SSPInterface
    w = _w("vit_test_patch16_32_reg4", seed=21, std=0.1)
    model = build_regtoken(w)
    px = _px(32, 32, seed=22)
    labels = ref_cpu.logits_of(model, px).argmax(-1)
    loader = [{"pixel_values": px[i:i + 8], "labels": labels[i:i + 8]} for i in range(0, 32, 8)]
    acc = vp.evaluate_top1(model, loader, device="cuda", progress=False)
    assert acc >= 0.9, acc
    att, mlp = Auto2SSPInterface(model, loader, device="cuda", batch_limit=2, min_remaining=32).fit()
    assert att.numel() == 4 and len(mlp) == 4
    res = vp.prune_vit_mlp_width(model, n_to_prune_per_block=[32] * 4, min_remaining=32, strategy="l1", collect_masks=True,
                                 precomputed_importance=[m.float() for m in mlp])
    out = vp.prune_vit_attention_blocks(res["model"], sparsity=0.25, dataloader=None, device="cuda", num_to_prune=1, show_progress=False,
                                        selected_indices=[int(torch.argsort(att)[0])])
    pm = out["model"]
    flat = W.from_module(pm)
    assert W.reg_tokens_of(flat) == 4 and flat["no_embed_class"] is True and sum(bool(flat.get(f"attn_absent.{i}")) for i in range(4)) == 1
    e = VitEngine(flat, max_images=32)
    got = vp.engine_for(pm, "cuda", max_images=32).forward_logits(px.to(gpu))
    assert torch.equal(got, e.forward_logits(px.to(gpu)))
    _check_logits(got.cpu(), ref_cpu.logits_of(pm, px).float(), "pruned live module vs its own CPU forward")
    back = W.load_checkpoint(export.save_timm_state_dict(pm, tmp_path, "reg"), heads=4)      # (the duck module has no config to say its heads)
    assert W.reg_tokens_of(back) == 4 and back["no_embed_class"] is True and int(back["fc1_w.0"].shape[0]) == 96
    e2 = VitEngine(back, max_images=32)
    assert torch.equal(e2.forward_logits(px.to(gpu)), got)
    e.close(); e2.close()
    vp.release_engines(free=True)


def test_cli_register_model_end_to_end(gpu, tmp_path):
    """auto_2ssp.py --model vit_test_patch16_32_reg4 (synthetic weights: registers, class-free positions, LayerScale) prunes and writes
    its report; no new flag."""
    cli = os.path.join(PKG, "auto_2ssp.py")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, cli, "--model", "vit_test_patch16_32_reg4", "--output-dir", str(out), "--sparsity_rate", "0.25",
                        "--min-remaining", "32", "--synthetic-calib", "64", "--eval-batches", "2", "--batch-size", "16", "--num-classes", "10"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert list(out.rglob("report-*.json")), "no report written"
