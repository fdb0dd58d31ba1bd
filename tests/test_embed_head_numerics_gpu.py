"""The two ends of the forward — patch_embed_kernel (csrc/patch.hip.h), its twin im2col_patch_kernel + gemm_bf16_kernel<EPI_PATCH> and
cls_row_kernel at the ingress; gemm_bf16_kernel<EPI_F32>, argmax_top1_kernel and dist_head_top1_kernel at the egress — through the only
entries that launch them (ssp2_embed, ssp2_head, ssp2_tail_group) on depth-1 engines of whatever geometry a case needs, against the
float64 statements of tests/embed_head_cases.py (proved on the CPU by tests/test_embed_head_statements_cpu.py).  The statements and
bounds below were written before the first GPU run.  u = 2^-24.  Every engine here has head dimension 64 (heads = dim / 64): the engine
builds its d_h = 80 attention for 257 .. 288 tokens only, and no test of this module runs an attention.

Patch embedding, exact operands, bit for bit, 100 % of the buffer.  Pixels and weights k / 8, |k| <= 15, bias k / 64, position table
arbitrary fp32:  x = fl32(pos[P + q] + float(bf16(fl32(acc + b)))), acc exact; prefix rows fl32(cls + pos[0]), fl32(dist + pos[1]).
Geometries (EMBED_CASES): K-tiles 1, 2, 3, 4, 5, 7, 10 of the element-wise gather (p = 4, 6, 7, 9, 10, 12, 14) and 3, 12, 27, 48 of the
16-byte one (p = 8, 16, 24, 32) — every depth at which a branch of the three-deep pixel ring is taken for the first or the last time —
dim 64 (half a column tile), 192, 320, 768, prefix 1 and 2, M = n * patches at 80, 126, 128, 129 (one patch per image), 132 .. 144, 261
(three row tiles), 387 and 400 (four).  Both layouts (contiguous; slabs of 2 or 3 images with a short last slab) and both paths
(patch_lds 1 / 0), whose buffers must be torch.equal.  x is the caller's buffer with 5 rows behind rows(n, group), pre-filled with a
sentinel: rows behind the last image keep it, pad rows between slabs are zero.  A second exact case (ROUNDING_CASES, p = 14 and p = 8)
has pixels that are no bf16 values: +-(1 + (2m + 1) / 256), the ties, and their fp32 neighbours on either side; the statement rounds
them with .to(torch.bfloat16) (RNE).  A swapped ky / kx, a wrong position row or a K-tile read before it landed moves elements by
multiples of 2^-6: nothing hides under a tolerance.
Special pixel values, a run of its own: one NaN, one +inf, one fp32 maximum (above the bf16 maximum: +inf once rounded) and one fp32
subnormal (2^-140: rounds to zero, or is flushed), each in one pixel of a patch of its own.  The NaN's patch is NaN in every column, the
infinities' patches are +inf / -inf / NaN by the sign / zero of the weight at that k, the subnormal's patch and every other row have
the clean run's bits.
Realistic operands (p = 14, p = 16, p = 4): normalised-image-like pixels with x 100 outliers, weights of std 0.02 .. 0.05 with x 8
outlier rows; the residual form's bound of tests/test_bf16_gemm_numerics_gpu.py with xin = pos:
  E_acc = (K + 1) u sum|a_k w_k|,  c = E_acc + u (|y| + E_acc),  |x - (pos + y)| <= 2^-8 (|y| + c) + c + u |pos + y|   element-wise.

Classifier head and top-1, on img 32 / patch 16 engines (5 tokens; 6 with a distillation token).  The prefix rows of x are balanced
+-4 rows, so the classifier's A operand is exactly +-lnf_g (gamma in 1, 0.5, 1.75, -3 by column); every other row of x is NaN and must
never be read.  Head weights k / 8, |k| <= 3, bias k / 64:  logit = float(bf16(fl32(acc + b))) bit for bit (NaN where NaN is expected,
whatever its payload).  Class counts 1, 10, 63, 64, 65, 127, 128, 129, 1000, 1001, 21843 (the scalar store's m < M && n < N), widths
64 .. 1280, image counts 1, 3, 4, 5, 127, 128, 129, 260; logits and pred are the caller's buffers with a sentinel row behind n;
contiguous and slab layouts; eng.head and eng.tail (attention of the neutral last block skipped: zero proj / fc2) give the same bits
and leave x alone.  pred must equal the written-out rule (lowest NaN index, else lowest index of the maximum) on the PREDICTED logits
and torch.argmax of the returned ones; `correct` is pre-loaded with 1000 and gains one per matching label, labels including -1, C and
2^40.  With |logit| of a few tens, the maximum of a row of bf16 logits is tied by chance in a few rows per hundred (printed);
TOP1_SCENARIOS add, at 1000 classes: equal maxima in other lanes of one loop step, in one lane at other steps, in both with the lowest
index in a late lane, every logit equal, every logit -inf, a +inf column, NaN bias columns above and below a +inf column and behind it,
+inf weights whose sum is +inf, -inf or NaN by the row's signs, and in every case one image whose prefix row is NaN.  Slots
(eng.tail(slots = s), shared labels, correct[s]) in both layouts, with labels that match a different slot from image to image.
Distillation head (prefix 2, two heads): logit = 0.5 * float(bf16(fl32(a + b))) of the two heads' exact logits, with chosen sums on
classes 0 .. 3 (a tie that rounds down to even, one that rounds up, +inf + -inf, magnitudes 2^20 apart), head_dist = -head on equal
rows (every class ties at 0), a NaN CLS row in one image and a NaN DIST row in another (every logit of those rows is written: NaN, not
the sentinel).  prefix = 2 without the second head: the DIST row, NaN here, is ignored.
Realistic operands (768 x 1000, 1280 x 1001): Gaussian rows with outlier channels, h = eng.layernorm of the same rows (the forward's
own launch), y in float64 over the bf16 values:  |logit - y| <= 2^-8 (|y| + c) + c, c as above.
How the bf16 MFMA rounds inside one instruction is not documented; a ratio above 1 would be answered by widening E_acc by at most 2
(truncating adds) and saying so here.
After the first GPU run nothing above had to change and no kernel had to: all cases passed, every exact case at 100 % identical bits on
both patch paths and both layouts, every sentinel intact.  Measured worst error / bound: realistic embedding 0.969 (p = 14), 0.962
(p = 16), 0.993 (p = 4); realistic head 0.965 (768 x 1000) and 0.943 (1280 x 1001) — the one bf16 rounding, 2^-8 |y|, is what sits against
the bound; E_acc stayed as stated, no widening for truncating adds was needed.  Rows whose maximum is tied by chance: 4 of 128 at 127
classes, 5 of 260 at 129, 7 of 260 at 1000.  Added after that run, on the same statements: the scenarios in BOTH heads of a distillation
engine and its slots case (dist_head_top1_kernel carries its own copy of the rule and of `period`).
Planted defects, each built once as a library of its own, run against this module once and reverted:
  ky / kx swapped in patch_embed_kernel's element-wise gather   every element-wise geometry of test_patch_embedding_exact_operands_bit_for_bit
                                                               (7 + the p = 14 ties case), the element-wise special-value case and two
                                                               realistic ones fail; the 16-byte geometries pass, as they must
  g.prefix + q -> q in patch_embed_kernel's position index      all 14 exact cases, both special-value cases, all 3 realistic ones
  v > best -> v >= best in argmax_top1_kernel's lane loop       test_top1_ties_infinities_and_nans [one lane at other steps], [both, lowest index
                                                               in a late lane], [every logit equal], [every logit -inf]
  oi < bi dropped from its cross-lane step                      test_head_logits_and_top1_bit_for_bit at 127, 129, 1000 and 21843 classes (the
                                                               chance ties) and the scenarios [both, ...], [every logit equal], [every logit
                                                               -inf]; [other lanes of one step] passes: the exchange order happens to end on
                                                               the lowest index there
  row % period -> row in its label index                        both cases of test_tail_slots_count_per_slot_against_shared_labels
"""
import time

import pytest
import torch

import embed_head_cases as EH

pytestmark = pytest.mark.gpu

SENT = -77.0
GUARD = 5
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    t0 = time.time()
    yield
    print(f"\n[embed / head numerics] module time {time.time() - t0:.1f} s")


def _engine(w, n):
    from ssp2vit.engine import VitEngine
    return VitEngine(w, device=DEV, max_images=n)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = EH.same_bits_or_nan(got, want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[:4].tolist()}"


# ------------------------------------------------------------------------------------------------------------- patch embedding
def _embed_both_paths(eng, px, n, group, what):
    """x on the CPU from patch_lds = 1, after asserting that patch_lds = 0 leaves the same buffer, sentinels included."""
    rows = eng.rows(n, group)
    bufs = []
    for lds in (1, 0):
        eng.set_option("patch_lds", lds)
        x = torch.full((rows + GUARD, eng.dim), SENT, dtype=torch.float32, device=DEV)
        assert eng.embed(px, x=x, group=group) is x
        bufs.append(x.cpu())
    eng.set_option("patch_lds", 1)
    assert not bool(EH.same_bits_or_nan(bufs[0], bufs[1]).any()), f"{what}: the LDS-staged and the im2col path differ"
    return bufs[0]


def _expected_buffer(stmt, n, tokens, group):
    total, first, pad = EH.embed_layout(n, tokens, group)
    want = torch.full((total + GUARD, stmt.shape[-1]), SENT)
    want[pad] = 0.0
    for t in range(tokens):
        want[first + t] = stmt[:, t]
    return want


@pytest.mark.parametrize("p,img,dim,prefix,n,group,pixels", [c + ("grid",) for c in EH.EMBED_CASES] + [c + ("ties",) for c in EH.ROUNDING_CASES])
def test_patch_embedding_exact_operands_bit_for_bit(p, img, dim, prefix, n, group, pixels):
    w = EH.flat_vit(img, p, dim, EH.heads_of(dim), 10, prefix=prefix)
    px = (EH.tie_pixels if pixels == "ties" else EH.exact_pixels)(n, img, seed=p)
    stmt = EH.embed_statement(px, w)
    eng = _engine(w, n)
    try:
        tokens = eng.tokens
        assert tokens == (img // p) ** 2 + prefix
        pxd = px.to(DEV)
        for grp in (0, group):
            what = f"p {p} img {img} dim {dim} prefix {prefix} n {n} group {grp} ({pixels})"
            want = _expected_buffer(stmt, n, tokens, grp)
            assert eng.rows(n, grp) + GUARD == want.shape[0], what
            if grp:
                slabs = -(-n // grp)
                assert slabs > 1 and n % grp != 0, "the slab run wants a short last slab"
            x = _embed_both_paths(eng, pxd, n, grp, what)
            _assert_same(x, want, what)
    finally:
        eng.close()


@pytest.mark.parametrize("p,img,dim,prefix,n", [(7, 28, 320, 1, 9), (8, 32, 192, 2, 9)])
def test_patch_embedding_special_pixel_values_stay_in_their_patch(p, img, dim, prefix, n):
    w = EH.flat_vit(img, p, dim, EH.heads_of(dim), 10, prefix=prefix)
    side = img // p
    # (image, patch, channel, ky, kx, value): a patch each
    spots = [(1, 0, 0, 0, 0, EH.NAN), (2, side * side - 1, 2, p - 1, p - 1, EH.INF), (4, side + 1, 1, 2, p - 2, torch.finfo(torch.float32).max),
             (n - 1, 2, 2, p - 2, 1, 2.0 ** -140)]
    clean = EH.exact_pixels(n, img, seed=100 + p)
    dirty = clean.clone()
    for im, q, c, ky, kx, v in spots:
        yy, xx = (q // side) * p + ky, (q % side) * p + kx
        clean[im, c, yy, xx] = 0.0 if v == 2.0 ** -140 else clean[im, c, yy, xx]
        dirty[im, c, yy, xx] = v
    assert float(dirty.to(torch.bfloat16)[spots[2][0]].max()) == EH.INF          # the fp32 maximum rounds to +inf
    eng = _engine(w, n)
    try:
        tokens = eng.tokens
        xc = _embed_both_paths(eng, clean.to(DEV), n, 0, "clean")
        _assert_same(xc, _expected_buffer(EH.embed_statement(clean, w), n, tokens, 0), "clean run")
        xd = _embed_both_paths(eng, dirty.to(DEV), n, 0, "special values")
    finally:
        eng.close()
    wk = w["patch_w"].reshape(dim, -1)
    want_nan = torch.zeros_like(xc, dtype=torch.bool)
    want_inf = torch.zeros_like(xc)                                              # +1: +inf, -1: -inf
    for im, q, c, ky, kx, v in spots[:3]:
        row = im * tokens + prefix + q
        col = wk[:, c * p * p + ky * p + kx]
        if v != v:
            want_nan[row] = True
        else:
            want_nan[row] = col == 0
            want_inf[row] = torch.sign(col)
            assert bool((col == 0).any()) and bool((col > 0).any()) and bool((col < 0).any())    # all three outcomes occur
    assert torch.equal(torch.isnan(xd), want_nan), "NaN elements are not the ones the special pixels own"
    assert torch.equal(xd == EH.INF, want_inf > 0) and torch.equal(xd == -EH.INF, want_inf < 0), "infinite elements differ"
    fin = ~want_nan & (want_inf == 0)
    assert torch.equal(_bits(xd)[fin], _bits(xc)[fin]), "a special pixel changed an element outside its patch (or the subnormal changed its own)"


@pytest.mark.parametrize("p,img,dim,prefix,n,group", EH.REALISTIC_EMBED)
def test_patch_embedding_realistic_operands_against_float64(p, img, dim, prefix, n, group):
    w = EH.flat_vit(img, p, dim, EH.heads_of(dim), 10, prefix=prefix)
    w["patch_w"] = EH.realistic_patch_weight(dim, p, seed=p)
    w["patch_b"] = (torch.randn(dim, generator=torch.Generator().manual_seed(p)) * 0.02).to(torch.bfloat16).float()
    px = EH.realistic_pixels(n, img, seed=7 * p)
    ref, bound = EH.embed_bound(px, w)
    eng = _engine(w, n)
    try:
        tokens = eng.tokens
        x = _embed_both_paths(eng, px.to(DEV), n, group, "realistic")
    finally:
        eng.close()
    assert bool((x[n * tokens:] == SENT).all())
    got = x[: n * tokens].view(n, tokens, dim)[:, prefix:].double()
    assert bool(torch.isfinite(got).all())
    ratio = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"\n[realistic embed p={p} img={img} dim={dim} M={n * (tokens - prefix)} K={3 * p * p}] worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------- classifier head
def _run(eng, x, n, group, entry, labels, slots=1):
    """One launch on the caller's buffers: logits with a sentinel row behind, pred likewise, correct pre-loaded with 1000."""
    tot = n * slots
    lg = torch.full((tot + 1, eng.classes), SENT, dtype=torch.float32, device=DEV)
    pr = torch.full((tot + 1,), -7, dtype=torch.int32, device=DEV)
    correct = torch.full((slots,), 1000, dtype=torch.int64, device=DEV)
    if entry == "head":
        assert slots == 1
        eng.head(x, n, labels=labels, correct=correct, group=group, logits=lg, pred=pr)
    else:
        eng.tail(x, n, attn_skip=[eng.depth - 1], labels=labels, correct=correct, slots=slots, group=group, logits=lg, pred=pr)
    return lg.cpu(), pr.cpu(), correct.cpu()


def _check(res, want, labels, what, slots=1):
    lg, pr, correct = res
    tot = want.shape[0]
    n = tot // slots
    assert bool((lg[tot] == SENT).all()) and int(pr[tot]) == -7, f"{what}: the row behind n was written"
    _assert_same(lg[:tot], want, f"{what}: logits")
    rule = EH.top1_rule(want)
    assert torch.equal(pr[:tot].long(), rule), f"{what}: pred differs from the rule at rows {(pr[:tot].long() != rule).nonzero().view(-1)[:8].tolist()}"
    assert torch.equal(pr[:tot].long(), lg[:tot].argmax(-1)), f"{what}: pred differs from torch.argmax of the returned logits"
    hits = (rule.view(slots, n) == labels.view(1, n)).sum(1)
    assert torch.equal(correct, 1000 + hits), f"{what}: correct {correct.tolist()} against {(1000 + hits).tolist()}"


def _head_both_entries(eng, rows, want, labels, group, what, slots=1):
    """eng.head and eng.tail on the same x (slots > 1: the tail alone): statement, sentinels, same bits, x untouched."""
    x = EH.head_rows_x(rows, eng.tokens, group, guard=GUARD).to(DEV)
    assert eng.rows(rows.shape[0], group) + GUARD == x.shape[0]
    x0 = x.clone()
    ld = labels.to(DEV)
    res = {}
    for entry in (("head", "tail") if slots == 1 else ("tail",)):
        res[entry] = _run(eng, x, rows.shape[0] // slots, group, entry, ld, slots)
        _check(res[entry], want, labels, f"{what}, {entry}, group {group}", slots)
        assert torch.equal(_bits(x), _bits(x0)), f"{what}: {entry} wrote into x"
    if slots == 1:
        assert not bool(EH.same_bits_or_nan(res["head"][0], res["tail"][0]).any()) and torch.equal(res["head"][1], res["tail"][1])
    return res


def _prefix_rows(n, dim, P, seed, nan_cls=(), nan_dist=()):
    rows = EH.balanced_rows(n * P, dim, seed).view(n, P, dim).clone()
    for i in nan_cls:
        rows[i, 0] = EH.NAN
    for i in nan_dist:
        rows[i, 1] = EH.NAN
    return rows


def _single_head_want(rows, w):
    return EH.head_logits(EH.head_operand(rows[:, 0], w["lnf_g"]), w["head_w"], w["head_b"])


@pytest.mark.parametrize("dim,classes,n,group", EH.HEAD_CASES)
def test_head_logits_and_top1_bit_for_bit(dim, classes, n, group):
    w = EH.head_case_weights(dim, classes)
    rows = _prefix_rows(n, dim, 1, seed=dim + classes + n, nan_cls=(1,) if n >= 3 else ())
    want = _single_head_want(rows, w)
    labels = EH.labels_for(EH.top1_rule(want), classes, seed=n)
    if n >= 100 and classes >= 10:
        assert 0 < int((EH.top1_rule(want) == labels).sum()) < n
        tied = (want == want.max(1, keepdim=True).values).sum(1) > 1
        print(f"\n[head dim={dim} C={classes} n={n}] rows whose maximum is tied: {int(tied.sum())}")
    eng = _engine(w, n)
    try:
        for grp in (0, group) if group else (0,):
            _head_both_entries(eng, rows, want, labels, grp, f"dim {dim} C {classes} n {n}")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def eng_1000():
    e = _engine(EH.head_case_weights(768, EH.TOP1_C), 16)
    yield e
    e.close()


@pytest.mark.parametrize("scenario", list(EH.TOP1_SCENARIOS))
def test_top1_ties_infinities_and_nans(eng_1000, scenario):
    dim, n = 768, 9
    w = EH.head_case_weights(dim, EH.TOP1_C, scenario=scenario)
    eng_1000.reload(w)
    rows = _prefix_rows(n, dim, 1, seed=len(scenario), nan_cls=(5,))
    want = _single_head_want(rows, w)
    rule = EH.top1_rule(want)
    assert int(rule[5]) == 0
    labels = EH.labels_for(rule, EH.TOP1_C, seed=3)
    for grp in (0, 4):
        _head_both_entries(eng_1000, rows, want, labels, grp, scenario)


@pytest.mark.parametrize("dim,classes,n,slots,group", EH.SLOT_CASES)
def test_tail_slots_count_per_slot_against_shared_labels(dim, classes, n, slots, group):
    w = EH.head_case_weights(dim, classes, scenario="+inf weights, per-row signs" if classes == EH.TOP1_C else None)
    tot = n * slots
    rows = _prefix_rows(tot, dim, 1, seed=tot + classes, nan_cls=(1, n + 2))         # a NaN row in slot 0 and another image of slot 1
    want = _single_head_want(rows, w)
    rule = EH.top1_rule(want).view(slots, n)
    labels = torch.stack([rule[0 if i < 2 else i % slots, i] for i in range(n)])    # images 0 and 1 carry slot 0's answer, image i slot (i mod slots)'s
    labels[n - 1] = 2 ** 40
    hits = (rule == labels.view(1, n)).sum(1)
    assert len(set(hits.tolist())) > 1 or slots == 1, "the slots should not all count the same"
    eng = _engine(w, tot)
    try:
        for grp in (0, group):
            _head_both_entries(eng, rows, want, labels, grp, f"slots {slots} x {n}", slots=slots)
    finally:
        eng.close()


def _dist_want(rows, w):
    a = EH.head_logits(EH.head_operand(rows[:, 0], w["lnf_g"]), w["head_w"], w["head_b"])
    b = EH.head_logits(EH.head_operand(rows[:, 1], w["lnf_g"]), w["head_dist_w"], w["head_dist_b"])
    return EH.dist_logits(a, b)


@pytest.mark.parametrize("dim,classes,n,group", EH.DIST_CASES)
def test_distillation_head_mean_and_top1_bit_for_bit(dim, classes, n, group):
    w = EH.dist_special(EH.head_case_weights(dim, classes, prefix=2, dist_head=True))
    rows = _prefix_rows(n, dim, 2, seed=dim + n, nan_cls=(1,), nan_dist=(2,))
    want = _dist_want(rows, w)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isnan(want[2]).all())
    if classes > 3:
        assert float(want[0, 0]) == 0.5 and float(want[0, 1]) == 0.5 * (1 + 2.0 ** -6) and bool(torch.isnan(want[:, 2]).all())
        assert float(want[0, 3]) == 2.0 ** 19 * (1 + 2.0 ** -7) and int(EH.top1_rule(want)[0]) == 2
    labels = EH.labels_for(EH.top1_rule(want), classes, seed=n)
    eng = _engine(w, n)
    try:
        assert eng.tokens == 6 and eng.dist_head == 1
        for grp in (0, group):
            _head_both_entries(eng, rows, want, labels, grp, f"dist dim {dim} C {classes} n {n}")
        # head_dist = -head on equal rows: a = -b, every mean is +0 and every class ties
        wc = EH.dist_cancelling(EH.head_case_weights(dim, classes, prefix=2, dist_head=True))
        eng.reload(wc)
        rows[:, 1] = rows[:, 0]
        rows[2, 1] = EH.NAN
        want = _dist_want(rows, wc)
        ok = torch.ones(n, dtype=torch.bool); ok[1] = ok[2] = False
        assert torch.equal(_bits(want[ok]), torch.zeros_like(_bits(want[ok]))) and bool((EH.top1_rule(want) == 0).all())
        labels = torch.zeros(n, dtype=torch.int64); labels[0] = -1
        _head_both_entries(eng, rows, want, labels, group, f"cancelling heads dim {dim} C {classes} n {n}")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def eng_dist_1000():
    e = _engine(EH.head_case_weights(320, EH.TOP1_C, prefix=2, dist_head=True), 16)
    yield e
    e.close()


@pytest.mark.parametrize("scenario", list(EH.TOP1_SCENARIOS))
def test_distillation_top1_ties_infinities_and_nans(eng_dist_1000, scenario):
    """The scenarios of the single head in BOTH heads: dist_head_top1_kernel's own copy of the rule."""
    dim, n = 320, 9
    w = EH.head_case_weights(dim, EH.TOP1_C, prefix=2, dist_head=True, scenario=scenario)
    eng_dist_1000.reload(w)
    rows = _prefix_rows(n, dim, 2, seed=len(scenario) + 50, nan_dist=(5,))
    want = _dist_want(rows, w)
    rule = EH.top1_rule(want)
    assert int(rule[5]) == 0 and bool(torch.isnan(want[5]).all())
    labels = EH.labels_for(rule, EH.TOP1_C, seed=4)
    for grp in (0, 4):
        _head_both_entries(eng_dist_1000, rows, want, labels, grp, f"dist, {scenario}")


def test_distillation_tail_slots_count_per_slot():
    dim, classes, n, slots, group = 192, 129, 4, 3, 2
    w = EH.head_case_weights(dim, classes, prefix=2, dist_head=True)
    tot = n * slots
    rows = _prefix_rows(tot, dim, 2, seed=77, nan_cls=(1,), nan_dist=(n + 2,))
    want = _dist_want(rows, w)
    rule = EH.top1_rule(want).view(slots, n)
    labels = torch.stack([rule[0 if i < 2 else i % slots, i] for i in range(n)])
    labels[n - 1] = -1
    assert len(set((rule == labels.view(1, n)).sum(1).tolist())) > 1
    eng = _engine(w, tot)
    try:
        for grp in (0, group):
            _head_both_entries(eng, rows, want, labels, grp, f"dist slots {slots} x {n}", slots=slots)
    finally:
        eng.close()


def test_two_prefix_tokens_with_one_head_ignore_the_distillation_row():
    dim, classes, n = 192, 65, 6
    w = EH.head_case_weights(dim, classes, prefix=2)
    rows = _prefix_rows(n, dim, 2, seed=9, nan_dist=range(n))
    want = _single_head_want(rows, w)
    assert bool(torch.isfinite(want).all())
    labels = EH.labels_for(EH.top1_rule(want), classes, seed=1)
    eng = _engine(w, n)
    try:
        assert eng.tokens == 6 and eng.dist_head == 0
        for grp in (0, 4):
            _head_both_entries(eng, rows, want, labels, grp, "prefix 2, one head")
    finally:
        eng.close()


@pytest.mark.parametrize("dim,classes,n", [(768, 1000, 130), (1280, 1001, 130)])
def test_head_realistic_operands_against_float64(dim, classes, n):
    w = EH.head_case_weights(dim, 10)
    w["classes"] = classes
    g = torch.Generator().manual_seed(dim)
    w["lnf_g"] = 1.0 + 0.1 * torch.randn(dim, generator=g); w["lnf_b"] = 0.1 * torch.randn(dim, generator=g)
    w["head_w"], w["head_b"] = EH.realistic_head_weight(classes, dim, seed=classes)
    rows = torch.randn(n, 1, dim, generator=g)
    rows[:, :, [5, dim // 3, dim - 2]] *= 100.0                       # outlier channels
    eng = _engine(w, n)
    try:
        x = EH.head_rows_x(rows, eng.tokens, 0, guard=GUARD).to(DEV)
        h = eng.layernorm(x, w["lnf_g"].to(DEV), w["lnf_b"].to(DEV), eng.eps, rows=n, gather=(eng.tokens, 0))
        res = {e: _run(eng, x, n, 0, e, torch.zeros(n, dtype=torch.int64, device=DEV)) for e in ("head", "tail")}
    finally:
        eng.close()
    lg = res["head"][0]
    assert torch.equal(lg, res["tail"][0]) and bool((lg[n] == SENT).all())
    hd, wd = h.cpu().double(), w["head_w"].to(torch.bfloat16).double()
    assert bool(torch.isfinite(hd).all())
    y = hd @ wd.T + w["head_b"].double()[None, :]
    e_acc = (dim + 1) * EH.U * (hd.abs() @ wd.abs().T)
    c = e_acc + EH.U * (y.abs() + e_acc)
    bound = 2.0 ** -8 * (y.abs() + c) + c
    err = (lg[:n].double() - y).abs()
    assert bool(torch.isfinite(err).all())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[realistic head dim={dim} C={classes} n={n}] worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(res["head"][1][:n].long(), lg[:n].argmax(-1))
