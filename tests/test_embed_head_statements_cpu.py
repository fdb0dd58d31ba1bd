"""CPU checks of tests/embed_head_cases.py: what tests/test_embed_head_numerics_gpu.py holds the kernels to is itself right.

* every exact-operand case really is exact: the integer numerators of its products, summed in absolute value per output element, stay
  below 2^24 units of their common granularity, so every partial sum in any order is an fp32 number (a case that fails this is a wrong
  case, not a kernel bug);
* the embedding statement agrees with the oracle's patch embedding (oracle/vit_modules.py under CPU autocast), the head statement with
  its final norm + head, within one bf16 ulp of the bf16 result (the oracle's tolerance: fp32 summation order and the one flip it causes);
* the written-out top-1 rule equals torch.argmax on rows with ties, +-inf, NaN and all -inf;
* balanced-sign rows normalise to exactly +-gamma after the bf16 rounding.
"""
import pytest
import torch

import embed_head_cases as EH
from oracle.vit_modules import build_from_flat

LIMIT = 2 ** 24


@pytest.mark.parametrize("p,img,dim,prefix,n,group", EH.EMBED_CASES + EH.ROUNDING_CASES)
def test_embedding_cases_accumulate_exactly(p, img, dim, prefix, n, group):
    w = EH.flat_vit(img, p, dim, EH.heads_of(dim), 10, prefix=prefix)
    rounding = (p, img, dim, prefix, n, group) in EH.ROUNDING_CASES
    px = (EH.tie_pixels if rounding else EH.exact_pixels)(n, img, seed=p)
    if rounding:                                   # every pixel sits on or beside a tie, none is a bf16 value, magnitudes stay in [1, 2]
        assert not bool((px.to(torch.bfloat16).float() == px).any())
        r = px.to(torch.bfloat16).float().abs()
        assert float(r.min()) >= 1.0 and float(r.max()) <= 2.0
        on_tie = (px.abs() * 256.0) == (px.abs() * 256.0).round()
        assert 0.2 < float(on_tie.float().mean()) < 0.5
    ka, kw = EH.embed_numerators(px, w)            # pixels in 1 / 128, weights in 1 / 8
    worst = EH.terms_bound(ka, kw)
    assert worst < LIMIT, f"sum |terms| reaches {worst} units of 2^-10"
    # the bias joins on the same grid: k / 64 = 16 k units
    assert bool((w["patch_b"] * 64.0 == (w["patch_b"] * 64.0).round()).all()) and bool((w["patch_b"].to(torch.bfloat16).float() == w["patch_b"]).all())
    assert worst + 16 * 127 < LIMIT


@pytest.mark.parametrize("dim,classes", sorted({(d, c) for d, c, _, _ in EH.HEAD_CASES + EH.DIST_CASES} | {(d, c) for d, c, _, _, _ in EH.SLOT_CASES}
                                               | {(768, EH.TOP1_C)}))
def test_head_cases_accumulate_exactly(dim, classes):
    scenarios = [None] + (list(EH.TOP1_SCENARIOS) if classes == EH.TOP1_C else [])
    for sc in scenarios:
        w = EH.head_case_weights(dim, classes, prefix=2, dist_head=True, scenario=sc)
        for key in ("head_w", "head_dist_w"):
            ka, kw = EH.head_numerators(w, key)    # |A| = |gamma| in quarters, weights in eighths
            worst = EH.terms_bound(ka, kw)
            assert worst < LIMIT, (sc, key, worst)
            b = torch.nan_to_num(w[key.replace("_w", "_b")], nan=0.0, posinf=0.0, neginf=0.0)
            assert bool((b.to(torch.bfloat16).float() == b).all()) and bool((b * 64.0 == (b * 64.0).round()).all())
            assert worst + float(b.abs().max()) * 32 < LIMIT            # the bias in units of 2^-5, rounded up by the fp32 add at most once


def test_balanced_rows_normalise_to_plus_minus_gamma():
    dim = 192
    rows = EH.balanced_rows(7, dim, seed=3)
    assert bool((rows.sum(1) == 0).all()) and bool((rows.abs() == 4.0).all())
    gamma = torch.tensor(EH.GAMMAS).repeat(dim // 4)
    assert bool((gamma.to(torch.bfloat16).float() == gamma).all())
    for eps in (1e-6, 1e-12):
        h = torch.nn.functional.layer_norm(rows, (dim,), gamma, torch.zeros(dim), eps).to(torch.bfloat16)
        assert torch.equal(h.double(), EH.head_operand(rows, gamma))


@pytest.mark.parametrize("C", [10, 65, 1000, 1001, 21843])
def test_top1_rule_equals_torch_argmax(C):
    g = torch.Generator().manual_seed(C)
    base = torch.randint(-3, 4, (12, C), generator=g).float()           # ties everywhere
    rows = [base.clone() for _ in range(8)]
    rows[1][:, C // 2] = EH.INF
    rows[2][:, C // 3] = -EH.INF
    rows[3][:, C - 1] = EH.NAN                                          # a NaN in the last column
    rows[4][:, C // 2] = EH.INF; rows[4][:, C - 1] = EH.NAN; rows[4][:, 3 % C] = EH.NAN
    rows[5].fill_(-EH.INF)
    rows[6].fill_(EH.NAN)
    rows[7][:, C // 2:] = EH.INF                                        # many +inf: the first one
    lg = torch.cat(rows)
    assert torch.equal(EH.top1_rule(lg), lg.argmax(-1))
    assert int(EH.top1_rule(rows[5])[0]) == 0 and int(EH.top1_rule(rows[4])[0]) == min(3 % C, C - 1)


def test_top1_scenarios_put_the_answer_where_they_say():
    """The scenarios of the GPU module, on the predicted logits: the tied classes are the maximum in every row, the lowest one wins."""
    dim, n = 768, 16
    rows = EH.balanced_rows(n, dim, seed=1)
    want = {"other lanes of one step": {131}, "one lane at other steps": {195}, "both, lowest index in a late lane": {190},
            "every logit equal": {0}, "every logit -inf": {0}, "+inf column": {321}, "NaN bias above and below +inf": {130},
            "NaN behind the maximum": {900}}
    for sc in EH.TOP1_SCENARIOS:
        w = EH.head_case_weights(dim, EH.TOP1_C, scenario=sc)
        lg = EH.head_logits(EH.head_operand(rows, w["lnf_g"]), w["head_w"], w["head_b"])
        pred = EH.top1_rule(lg)
        assert torch.equal(pred, lg.argmax(-1)), sc
        if sc in want:
            assert set(pred.tolist()) == want[sc], (sc, pred.tolist())
        else:                                                           # per-row signs: NaN, +inf and -inf rows all occur at class 417
            col = lg[:, 417]
            assert bool(torch.isnan(col).any()) and bool((col == EH.INF).any()) and bool((col == -EH.INF).any())
            assert bool((pred[torch.isnan(col)] == 417).all()) and bool((pred[col == EH.INF] == 417).all())
            assert bool((pred[col == -EH.INF] == 90).all())             # there class 90 is +inf


def test_distillation_sums_round_as_stated():
    a = torch.tensor([1.0, 1.0 + 2.0 ** -7, EH.INF, 2.0 ** 20 * (1 + 2.0 ** -7), 3.0])
    b = torch.tensor([2.0 ** -8, 2.0 ** -8, -EH.INF, 1 + 2.0 ** -7, -3.0])
    assert bool((a.to(torch.bfloat16).float() == a).all()) and bool((b[:2].to(torch.bfloat16).float() == b[:2]).all())
    v = EH.dist_logits(a, b)
    assert float(v[0]) == 0.5 and float(v[1]) == 0.5 * (1 + 2.0 ** -6) and bool(torch.isnan(v[2])) and float(v[3]) == 0.5 * float(a[3])
    assert float(v[4]) == 0.0
    assert float(a[3] + b[3]) != float(a[3].double() + b[3].double())   # the fp32 sum is itself rounded


def _ulp_ok(got_bf16_as_f32, ref_bf16_as_f32):
    return bool(((got_bf16_as_f32 - ref_bf16_as_f32).abs() <= ref_bf16_as_f32.abs() * 2.0 ** -7 + 1e-30).all())


def test_embedding_statement_agrees_with_the_oracle():
    w = EH.flat_vit(28, 7, 64, 1, 10, prefix=1)
    for px in (EH.exact_pixels(3, 28, seed=5), EH.realistic_pixels(3, 28, seed=6)):
        model = build_from_flat(w, "timm")
        with torch.no_grad(), torch.autocast(device_type="cpu", enabled=True):
            y = model.patch_embed(px)
        assert y.dtype == torch.bfloat16
        pos = w["pos"].view(-1, 64)
        x = EH.embed_statement(px, w)
        assert _ulp_ok(EH.embed_y(px, w), y.float())
        assert torch.equal(x[:, 0], (w["cls"].view(1, 64) + pos[0:1]).expand(3, 64))
    # exact operands leave no summation order to differ in: the same bits
    px = EH.exact_pixels(3, 28, seed=5)
    with torch.no_grad(), torch.autocast(device_type="cpu", enabled=True):
        y = model.patch_embed(px)
    assert torch.equal(EH.embed_statement(px, w)[:, 1:], y.float() + w["pos"].view(-1, 64)[1:])


def test_head_statement_agrees_with_the_oracle():
    dim, C, n = 192, 65, 6
    w = EH.head_case_weights(dim, C)
    model = build_from_flat(w, "timm")
    rows = EH.balanced_rows(n, dim, seed=2)
    with torch.no_grad(), torch.autocast(device_type="cpu", enabled=True):
        ref = model.head(model.norm(rows))
    assert ref.dtype == torch.bfloat16
    got = EH.head_logits(EH.head_operand(rows, w["lnf_g"]), w["head_w"], w["head_b"])
    assert _ulp_ok(got, ref.float())
    assert torch.equal(got, ref.float())            # exact operands: the same bits
