"""LayerScale on the MI355X: the EPI_RESID_LS epilogue of both GEMM kernels bit for bit against the host's separate multiply and add
(bf16 and e4m3 operands, in place and out of place, both walk directions, planted defects), an engine with gamma = 1 against an engine
without LayerScale bit for bit, whole models against the real reference's fixtures and the CPU restatement of
tests/layerscale_models.py, the evaluation tail, the x_in form and the apply step, the 1370-token DINOv2 geometry on the key-streaming
attention, fp8 at one cut, and the reference-named API / CLI end to end."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT
from layerscale_models import LS_GOLDEN_CASES, bf16_from_bits, build_layerscale, load_golden

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


@pytest.fixture(scope="module")
def eng(gpu):
    from ssp2vit.engine import VitEngine
    e = VitEngine(_w("vit_test_patch16_32_ls"), device=gpu, max_images=4)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------ 1. the epilogue
def _gamma(N, g):
    """Distinct per column: 0, negatives, powers of two, values near 1e-6 and one whose product with an O(1) value is subnormal."""
    v = (torch.rand(N, generator=g) * 1.9 + 0.05) * torch.where(torch.rand(N, generator=g) < 0.3, -1.0, 1.0)
    v[:8] = torch.tensor([0.0, -1.0, 2.0 ** -3, 4.0, 1e-6, -1.3e-6, 1e-38, -2.0 ** -20])
    assert v.unique().numel() == N
    return v


def _check_epilogue(run, y, M, N, g, tag):
    """run(x, xin, rev) launches the LayerScale form; y = float(bf16(pre)) from the unscaled entry into a zero x.  In place and out of
    place, both walk directions: x == xin + fl32(gamma * y) computed on the host as a separate multiply and add; a padded x keeps its
    sentinel in rows past M and columns past N; a one-column shift of gamma and a fused multiply-add on the host both miss it."""
    gamma = _gamma(N, g)
    xv = torch.randn(M, N, generator=g)
    xv[::3, 6] = 0.0                                              # the subnormal product survives the add there
    want = xv + gamma * y                                         # host fp32: the product is rounded, then the sum
    ldx = N + 64
    for rev in (0, 1):
        for inplace in (True, False):
            x = torch.full((M + GUARD, ldx), SENT, device="cuda")
            xin = None
            if inplace:
                x[:M, :N] = xv.cuda()
            else:
                xin = torch.full((M + GUARD, ldx), float("nan"), device="cuda")
                xin[:M, :N] = xv.cuda()
            run(x, xin, gamma, rev)
            torch.cuda.synchronize()
            got = x.cpu()
            assert torch.equal(got[:M, :N].view(torch.int32), want.view(torch.int32)), (tag, rev, inplace, int((got[:M, :N] != want).sum()))
            assert bool((got[M:] == SENT).all()) and bool((got[:, N:] == SENT).all()), (tag, rev, inplace)
    sub = want[::3, 6]
    assert bool(((sub != 0) & (sub.abs() < 2.0 ** -126)).any()), "the subnormal-product column holds no subnormal"
    shifted = xv + torch.roll(gamma, 1) * y                       # planted defects: the check must see them
    fused = (xv.double() + gamma.double() * y.double()).float()   # exact product, one rounding: what an fma would give
    n_sh, n_fu = int((shifted != want).sum()), int((fused.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"[ls-epilogue] {tag}: a shifted gamma moves {n_sh} of {M * N} elements, a fused multiply-add {n_fu}")
    assert n_sh > M * N // 2 and n_fu > 0


@pytest.mark.parametrize("kernel,M,N,K", [("big", 300, 256, 256), ("big", 300, 512, 256), ("big", 4099, 256, 256), ("big", 4099, 512, 256),
                                          ("small", 130, 192, 64), ("small", 130, 384, 192), ("small", 130, 192, 192), ("small", 130, 384, 64)])
def test_layerscale_epilogue_bf16_bit_for_bit(gpu, eng, kernel, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    wt = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.1
    y = eng.linear(a, wt, bias, "resid", x=torch.zeros(M, N, device=gpu), kernel=kernel).cpu()       # 0 + y is exact
    assert float(y.abs().max()) > 0.1

    def run(x, xin, gamma, rev):
        eng.linear(a, wt, bias, "resid", x=x, kernel=kernel, gamma=gamma, xin=xin, rev=rev)
    _check_epilogue(run, y, M, N, g, f"bf16 {kernel} M={M} N={N} K={K}")


@pytest.mark.parametrize("M,N,K,const", [(300, 256, 256, 0.0), (300, 512, 256, 0.0625), (4099, 256, 256, 0.0), (4099, 512, 256, 0.0)])
def test_layerscale_epilogue_e4m3_bit_for_bit(gpu, eng, M, N, K, const):
    g = torch.Generator().manual_seed(M + N + K + 1)
    enc = lambda v: v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    a8 = enc(torch.randn(M, K, generator=g) * 3).to(gpu)
    w8 = enc(torch.randn(N, K, generator=g) * 120).to(gpu)
    ws = (torch.rand(N, generator=g) * 4e-4 + 1e-4).to(gpu)
    asc = None if const else (torch.rand(M, generator=g) + 0.5).to(gpu)
    bias = torch.randn(N, generator=g) * 0.1
    y = eng.linear_e4m3(a8, w8, ws, bias, "resid", ascale=asc, ascale_const=const, x=torch.zeros(M, N, device=gpu)).cpu()
    assert float(y.abs().max()) > 0.1

    def run(x, xin, gamma, rev):
        eng.linear_e4m3(a8, w8, ws, bias, "resid", ascale=asc, ascale_const=const, x=x, xin=xin, rev=rev, gamma=gamma)
    _check_epilogue(run, y, M, N, g, f"e4m3 M={M} N={N} K={K} ascale_const={const}")


# ------------------------------------------------------------------------------------- 2. gamma = 1 changes nothing but the form
@pytest.mark.parametrize("n", [4, 24])
def test_unit_layerscale_engine_equals_the_plain_engine_bit_for_bit(gpu, n):
    """gamma = 1 on every branch: 1 * y is exact, so the LayerScale forms (the 128 x 128 kernel at 4 images, the 256 x 256 kernel at 24:
    4728 rows) must leave the streams after one block, the logits (the CLS-only tail) and the stage-1 scores of the plain engine, in the
    contiguous and the slab layout."""
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch16_224_d2", seed=5)
    w1 = dict(w, **{f"ls{b}.{i}": torch.ones(384) for b in (1, 2) for i in range(2)})
    plain, unit = VitEngine(w, max_images=n), VitEngine(w1, max_images=n)
    assert unit.layer_scale == ((True, True),) * 2 and plain.layer_scale == ((False, False),) * 2
    px = _px(n, 224, seed=1).to(gpu)
    for group in (0, n // 2):
        xa, xb = plain.embed(px, group=group), unit.embed(px, group=group)
        plain.layers(xa, n, 0, 1, score_group=group); unit.layers(xb, n, 0, 1, score_group=group)
        torch.cuda.synchronize()
        assert torch.equal(xa, xb), group
        sa = plain.forward_scores(px, "pre_gelu", "bf16_ref", group=group)
        sb = unit.forward_scores(px, "pre_gelu", "bf16_ref", group=group)
        assert torch.equal(sa, sb), group
    assert torch.equal(plain.forward_logits(px), unit.forward_logits(px))
    assert torch.equal(plain.forward_logits(px, attn_skip=[1]), unit.forward_logits(px, attn_skip=[1]))
    plain.close(); unit.close()


# ------------------------------------------------------------------------------ 4. the reference's fixtures and the restatement
def _check_logits(got, ref, tag):
    err = float((got.float() - ref.float()).abs().max())
    top = float(ref.float().abs().max())
    print(f"[ls-logits] {tag}: max |err| {err:.3e}, largest logit {top:.3e} ({err / (BF16_ULP * top):.2f} bf16 ulp of it)")
    assert err <= 2 * BF16_ULP * top, tag


@pytest.mark.parametrize("name", ["vit_test_patch16_32_ls", "vit_small_patch16_224_ls_d2"])
def test_dense_logits_and_stage1_scores_vs_the_cpu_restatement(gpu, name):
    """The engine built from the live CPU module against the module under CPU autocast: logits within 2 bf16 ulp of the largest logit;
    stage-1 scores, bf16 chain <= 2 ulp and >= 90 % identical, fp32 chain within rel 2e-3 + 1e-4 (pre-GELU site); the same weights
    without their LayerScale miss the logit bar (the scales are not ignored)."""
    from oracle import ref_cpu
    from ssp2vit import vit_pruning as vp, weights as W
    from ssp2vit.engine import VitEngine
    w = _w(name, seed=5)
    model = build_layerscale(w)
    flat = W.from_module(model)
    assert "ls1.0" in flat and "ls2.1" in flat
    n, img = 16, int(w["img"])
    px = _px(n, img, seed=7)
    e = VitEngine(flat, max_images=n)
    got = e.forward_logits(px.to(gpu)).cpu()
    ref = ref_cpu.logits_of(model, px).float()
    _check_logits(got, ref, name)
    bare = VitEngine({k: v for k, v in flat.items() if not k.startswith(("ls1.", "ls2."))}, max_images=n)
    off = float((bare.forward_logits(px.to(gpu)).cpu() - ref).abs().max())
    assert off > 8 * BF16_ULP * float(ref.abs().max()), off
    bare.close()
    batches = [{"pixel_values": px[:8]}, {"pixel_values": px[8:]}]
    for chain in ("bf16_ref", "fp32"):
        got_s = vp._compute_ffn_activation_importance(model, batches, device="cuda", score_chain=chain)
        ref_s = ref_cpu.ffn_activation_importance(model, batches, chain="autocast" if chain == "bf16_ref" else "fp32")
        for l, (a, r) in enumerate(zip(got_s, ref_s)):
            if chain == "bf16_ref":
                ulp = (a.cpu().view(torch.int16).int() - r.to(torch.bfloat16).view(torch.int16).int()).abs()
                print(f"[ls-scores] {name} block {l}: max {int(ulp.max())} ulp, {float((ulp == 0).float().mean()):.3f} identical")
                assert int(ulp.max()) <= 2 and float((ulp == 0).float().mean()) >= 0.9, (name, l, int(ulp.max()))
            else:
                assert torch.allclose(a.cpu(), r, rtol=2e-3, atol=1e-4), (name, l)
    vp.release_engines(free=True)
    e.close()


@pytest.mark.parametrize("tag", list(LS_GOLDEN_CASES))
def test_engine_vs_the_reference_fixtures(gpu, tag):
    """The engine on the live LayerScale module against the REAL reference's outputs (tests/golden/make_golden_layerscale.py): bf16
    stage-1 scores <= 2 ulp and >= 90 % identical; dense logits within 2 bf16 ulp of the largest logit; per image, top-1 correctness
    equal wherever the stored logits' margin decides it; each block's impact equal wherever the stored margins decide every image; the K
    selection equal when every impact is decided; the masks at the stored plan identical in every block whose cut the stored scores
    guarantee (ssp2vit.mask_parity) — every block of both fixtures, whose cut falls behind the fixtures' weak neurons."""
    import numpy as np
    from ssp2vit import vit_pruning as vp
    from ssp2vit.mask_conjunction import Auto2SSPInterface
    w, batches, z = load_golden(tag)
    model = build_layerscale(w)
    depth = int(w["depth"])
    t, min_rem, K = LS_GOLDEN_CASES[tag][3:6]
    imps = vp._compute_ffn_activation_importance(model, batches, device="cuda", score_chain="bf16_ref")
    ref_masks = np.unpackbits(z[f"mask.t{t}"], axis=1)
    res = vp.prune_vit_mlp_width(build_layerscale(w), n_to_prune_per_block=[t] * depth, min_remaining=min_rem, collect_masks=True,
                                 precomputed_importance=[a.float().cpu() for a in imps])
    # `guaranteed` as the project defines it (ssp2vit.mask_parity): no neuron within the band eps of the cut.  The engine's bf16-chain scores
    # are held to 2 bf16 ulp of the stored ones (below), a relative error of at most 2 * 2^-7; the band is twice that error
    from ssp2vit.mask_parity import mask_parity_report
    report = mask_parity_report([bf16_from_bits(z[f"s1_imp_bf16bits.{l}"]).float() for l in range(depth)], [t] * depth, min_rem, eps=2.0 ** -5)
    for l, a in enumerate(imps):
        r = bf16_from_bits(z[f"s1_imp_bf16bits.{l}"])
        ulp = (a.cpu().view(torch.int16).int() - r.view(torch.int16).int()).abs()
        print(f"[ls-golden] {tag} block {l}: scores max {int(ulp.max())} ulp, {float((ulp == 0).float().mean()):.3f} identical")
        assert int(ulp.max()) <= 2 and float((ulp == 0).float().mean()) >= 0.9, (tag, l)
        same = np.array_equal(np.asarray(res["ffn_prune_masks"][l], dtype=np.uint8), ref_masks[l, :r.numel()])
        print(f"[ls-golden] {tag} block {l}: mask identical {same} (guaranteed: {report['blocks'][l]['guaranteed']}, "
              f"cut margin {report['blocks'][l]['cut_margin']:.3f})")
        if report["blocks"][l]["guaranteed"]:
            assert same, (tag, l)
    assert report["blocks_guaranteed"] == depth, report              # the fixtures' cut is decisive in every block (weak_neurons)

    def decided(key_fmt):
        out = []
        for i in range(len(batches)):
            ref = bf16_from_bits(z[key_fmt.format(i=i)]).float()
            top2 = ref.topk(2, -1).values
            out.append(((top2[:, 0] - top2[:, 1]) > 2 * (2 * BF16_ULP * ref.abs().max()), ref))
        return out

    e = vp.engine_for(model, "cuda", max_images=32)
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
    print(f"[ls-golden] {tag}: top1 engine {top1} reference {float(z['top1'])}, decided interval [{blo}, {bhi}]")
    assert blo <= top1 <= bhi and blo <= float(z["top1"]) <= bhi
    att, _ = Auto2SSPInterface(model, batches, device="cuda", importance_mode="copy", batch_limit=5).fit()
    att = att.float().cpu()
    ref_att = torch.from_numpy(z["att_imp"])
    all_dec = True
    for blk in range(depth):
        plo, phi = check_model(f"bypass_logits_bf16bits.{blk}.{{i}}", [blk], f"attention {blk} bypassed")
        ilo, ihi = max(0.0, blo - phi), max(0.0, bhi - plo)
        print(f"[ls-golden] {tag} block {blk}: impact engine {float(att[blk])} reference {float(ref_att[blk])}, decided interval [{ilo}, {ihi}]")
        assert ilo - 1e-6 <= float(att[blk]) <= ihi + 1e-6, (tag, blk)
        all_dec = all_dec and ilo == ihi
    sel = sorted(int(i) for i in torch.argsort(att)[:K])
    print(f"[ls-golden] {tag}: selection engine {sel} reference {z[f's2_selected_k{K}'].tolist()} (every impact decided: {all_dec})")
    if all_dec:
        assert sel == z[f"s2_selected_k{K}"].tolist()
    vp.release_engines(free=True)


# ------------------------------------------------------------------------------------------ 5. tail, x_in form, apply step
@pytest.mark.parametrize("name", ["vit_small_patch16_224_ls_d2", "vit_test_patch16_32_ls"])
def test_tail_is_bit_identical_to_the_full_last_block(gpu, name):
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
    # a skipped attention leaves x untouched by the attention half: block = MLP half only, whatever ls1 holds
    x = e.embed(px); x0 = x.clone()
    e.layers(x, n, 0, 1, attn_skip=[0])
    w2 = dict(w); w2["ls1.0"] = torch.full_like(w["ls1.0"], 123.0)
    e2 = VitEngine(w2, max_images=n)
    y = e2.embed(px)
    assert torch.equal(y, x0)
    e2.layers(y, n, 0, 1, attn_skip=[0])
    assert torch.equal(x, y)
    e.close(); e2.close()


def test_x_in_form_and_block_by_block_equal_the_whole_call(gpu):
    """The stream entering a block read from another buffer (the search's prefix cache: ssp2_layers_from) and the blocks run one call
    each give the bits of one call over all blocks, at 24 images (the 256 x 256 kernel) in the slab layout."""
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch16_224_ls_d2", seed=9)
    n, group = 24, 8
    e = VitEngine(w, max_images=n)
    px = _px(n, 224, seed=3).to(gpu)
    x = e.embed(px, group=group)
    base = x.clone()
    e.layers(x, n, 0, 2, score_group=group)
    y = torch.empty_like(base)
    e.layers(y, n, 0, 1, score_group=group, x_in=base)
    e.layers(y, n, 1, 2, score_group=group)
    torch.cuda.synchronize()
    tok = e.tokens
    mpad = -(-group * tok // 128) * 128
    for s in range(n // group):
        a, b = x[s * mpad: s * mpad + group * tok], y[s * mpad: s * mpad + group * tok]
        assert torch.equal(a, b), s
    e.close()


def test_apply_into_twin_equals_an_engine_of_the_host_sliced_weights(gpu):
    """Width masks + a dropped attention applied into a pruned twin (device gathers; gamma is per hidden column and stays) give the logits,
    bit for bit, of an engine built from weights sliced on the host."""
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch16_224_ls_d2", seed=6)
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
    assert twin.layer_scale == dense.layer_scale
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
    dense.close(); twin.close(); host.close()


# --------------------------------------------------------------------------- 3. layers() against the operator composition
BLOCK_N = 24


@pytest.fixture(scope="module")
def block_engines(gpu):
    """bf16 and fp8 engines on the S/16 LayerScale cut and their pruned twins of widths (1030, 1536), the flat weights and the kept
    neurons per block."""
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch16_224_ls_d2", seed=3, spread=4.0)
    d_int = int(w["fc1_w.0"].shape[0])
    keep0 = torch.sort(torch.randperm(d_int, generator=torch.Generator().manual_seed(9))[:1030]).values
    masks = [torch.ones(d_int, dtype=torch.int32), torch.zeros(d_int, dtype=torch.int32)]
    masks[0][keep0] = 0
    out = {}
    for prec in ("bf16", "fp8"):
        dense = VitEngine(w, max_images=BLOCK_N, precision=prec)
        twin = dense.pruned_twin([1030, d_int], max_images=BLOCK_N)
        dense.apply_ffn_into(twin, masks)
        if prec == "fp8":
            twin._bind_stream()
            twin._check(twin.lib.ssp2_set_precision(twin.h, 1))     # a twin is created bf16: its e4m3 images from the pruned weights
        out[prec] = (dense, twin)
    torch.cuda.synchronize()
    yield w, out, [keep0, torch.arange(d_int)]
    for dense, twin in out.values():
        twin.close(); dense.close()


def _compose_ls_block(op, w, l, x, xin, n, tokens, group, heads, scale, keep, fp8):
    """Block l of a LayerScale forward from operator calls: x (f32 [M, D]) receives the block's output, the stream entering it is read
    from xin (None: x, in place).  fp8: LayerNorm, QKV, fc1 and fc2 on e4m3 operands, and (scale = the block's attention hand-off scale,
    not None) the out-projection too; both residual projections through the LayerScale entries with the block's gammas."""
    from ssp2vit.engine import ssp2_rows
    D, eps = int(w["dim"]), float(w["eps"])
    M = ssp2_rows(n, tokens, group)
    ld8 = (D + 127) // 128 * 128
    dev = lambda t: t.to("cuda", torch.float32).contiguous()  # noqa: E731
    g1, g2 = w[f"ls1.{l}"], w[f"ls2.{l}"]
    src = x if xin is None else xin

    def ln(stream, gk, bk):
        if not fp8:
            return op.layernorm(stream, dev(w[f"{gk}.{l}"]), dev(w[f"{bk}.{l}"]), eps, rows=M), None
        h8 = torch.zeros(M, ld8, dtype=torch.uint8, device="cuda")
        hs = torch.empty(M, device="cuda")
        op.layernorm(stream, dev(w[f"{gk}.{l}"]), dev(w[f"{bk}.{l}"]), eps, rows=M, out=h8, ascale=hs)
        return h8, hs

    def q8(wt, rows):
        b, s = op.quantise_e4m3(wt)
        return b[:rows], s[:rows]

    h, hs = ln(src, "ln1_g", "ln1_b")
    if fp8:
        qw, qs = q8(w[f"qkv_w.{l}"], 3 * D)
        qkv = op.linear_e4m3(h, qw, qs, w[f"qkv_b.{l}"], "bf16", ascale=hs)
    else:
        qkv = op.linear(h, w[f"qkv_w.{l}"], w[f"qkv_b.{l}"], "bf16")
    if fp8 and scale is not None:
        o8 = torch.zeros(M, ld8, dtype=torch.uint8, device="cuda")
        op.attention(qkv, n, tokens, heads, D // heads, group=group, out8=o8, out8_scale=scale)
        pw, ps = q8(w[f"proj_w.{l}"], D)
        op.linear_e4m3(o8, pw, ps, w[f"proj_b.{l}"], "resid", ascale_const=1.0 / scale, x=x, xin=xin, gamma=g1)
    else:
        o = op.attention(qkv, n, tokens, heads, D // heads, group=group)
        op.linear(o, w[f"proj_w.{l}"], w[f"proj_b.{l}"], "resid", x=x, xin=xin, gamma=g1)
    h, hs = ln(x, "ln2_g", "ln2_b")
    d = keep.numel()
    ld_int = (d + 63) // 64 * 64
    if fp8:
        ld8_int = (ld_int + 127) // 128 * 128                      # ceil128(ld_int): fc1's N, fc2's K
        fw, fs = op.quantise_e4m3(w[f"fc1_w.{l}"][keep])
        fb = torch.zeros(ld8_int)
        fb[:d] = w[f"fc1_b.{l}"][keep]
        act = op.linear_e4m3(h, fw[:ld8_int], fs[:ld8_int], fb, "gelu", ascale=hs)
        f2w, f2s = op.quantise_e4m3(w[f"fc2_w.{l}"][:, keep])
        op.linear_e4m3(act, f2w[:D], f2s[:D], w[f"fc2_b.{l}"], "resid", x=x, gamma=g2)
    else:
        f1 = torch.zeros(ld_int, D); f1[:d] = w[f"fc1_w.{l}"][keep]
        fb = torch.zeros(ld_int); fb[:d] = w[f"fc1_b.{l}"][keep]
        f2 = torch.zeros(D, ld_int); f2[:, :d] = w[f"fc2_w.{l}"][:, keep]
        act = op.linear(h, f1, fb, "gelu")
        op.linear(act, f2, w[f"fc2_b.{l}"], "resid", x=x, gamma=g2)
    return x


@pytest.mark.parametrize("prec,which,group,prefix,fp8_proj,from_xin", [
    ("bf16", "dense", 0, 0, 1, False), ("bf16", "dense", 4, 8, 1, True), ("bf16", "twin", 4, 8, 1, False),
    ("fp8", "dense", 0, 0, 1, False), ("fp8", "dense", 4, 8, 1, True), ("fp8", "dense", 0, 0, 0, False), ("fp8", "twin", 4, 8, 1, False)])
def test_layerscale_blocks_equal_their_operator_composition(gpu, block_engines, prec, which, group, prefix, fp8_proj, from_xin):
    """layers() block by block on the S/16 LayerScale cut (24 images, >= 4096 rows: the 256 x 256 kernel, and in fp8 every projection on
    e4m3 operands) against the block composed from operator calls — the LayerScale entries for the two residual projections — bit for bit
    on every image row: bf16 and fp8, contiguous and slab layout, the stage-1 hook on a slab prefix (the split fc1 launch), the fp8
    out-projection on e4m3 (the hand-off scale's constant) and on bf16, a width-pruned twin of ragged width 1030, and the first block's
    stream read from another buffer (x_in)."""
    from ssp2vit.engine import ssp2_rows
    w, engines, keeps = block_engines
    dense, twin = engines[prec]
    e = dense if which == "dense" else twin
    fp8 = prec == "fp8"
    n, tokens, heads = BLOCK_N, e.tokens, int(w["heads"])
    M = ssp2_rows(n, tokens, group)
    assert M >= 4096
    img = torch.zeros(M, dtype=torch.bool)
    mpad = -(-group * tokens // 128) * 128 if group else 0
    for i in range(n):
        r = (i // group) * mpad + (i % group) * tokens if group else i * tokens
        img[r:r + tokens] = True
    imgc = img.cuda()
    x = (torch.randn(M, int(w["dim"]), generator=torch.Generator().manual_seed(M + prefix)) * img[:, None]).cuda()
    if fp8:
        e.set_option("fp8_proj", fp8_proj)
    try:
        for l in range(int(w["depth"])):
            keep = keeps[l] if which == "twin" else torch.arange(int(w[f"fc1_w.{l}"].shape[0]))
            use_xin = from_xin and l == 0
            base = x.clone()
            xr = torch.zeros_like(x) if use_xin else x.clone()
            y = torch.zeros_like(x) if use_xin else x
            kw = dict(score_group=group, x_in=base if use_xin else None)
            if prefix:
                e.layers(y, n, l, l + 1, score_site="pre_gelu", score_images=prefix, **kw)
            else:
                e.layers(y, n, l, l + 1, **kw)
            scale = e.lib.ssp2_fp8_attn_scale(e.h, l) if (fp8 and fp8_proj) else None
            _compose_ls_block(dense, w, l, xr, base if use_xin else None, n, tokens, group, heads, scale, keep, fp8)
            torch.cuda.synchronize()
            if use_xin:
                assert torch.equal(base, x)                          # the stream that was read is left alone
            diff = (y[imgc] != xr[imgc])
            assert not bool(diff.any()), f"block {l}: {int(diff.sum())} of {int(img.sum()) * x.shape[1]} elements differ"
            assert bool(torch.isfinite(y[imgc]).all()) and not torch.equal(y[imgc], base[imgc])
            x = torch.where(imgc[:, None], y, torch.zeros_like(y))
    finally:
        if fp8:
            e.set_option("fp8_proj", 1)


# ------------------------------------------------------------------------------------------ 5b. one pass == two passes
@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_one_pass_equals_the_two_separate_passes_on_a_layerscale_model(gpu, precision):
    """core.prune_pass (the route fit() and the CLI take: stage-1 hook on the search's baseline forward, tails over all slots) against
    core.stage1_scores + core.depth_search_counts on the LayerScale S/16 cut: score tensors and counts EQUAL, for both score chains,
    equal and unequal batch limits, a ragged last batch, the layer-major and the candidate-major search."""
    from ssp2vit import core
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch16_224_ls_d2", seed=4, std=0.04, spread=4.0)
    depth, d_int, T, bsz = int(w["depth"]), int(w["fc1_w.0"].shape[0]), 197, 24
    big = VitEngine(w, max_images=core.lm_capacity_images(T, depth, 2 * bsz, bsz), precision=precision)
    small = VitEngine(w, max_images=2 * bsz, precision=precision)
    g = torch.Generator().manual_seed(31)
    batches = []
    for n in (bsz, bsz, bsz, bsz - 3):
        px = torch.randn(n, 3, 224, 224, generator=g)
        x = big.embed(px.cuda()); big.layers(x, n)
        lb = big.head(x, n, want_pred=True)[1].long().cpu()
        lb[::5] = (lb[::5] + 1) % 10                                 # a few wrong teachers: the baseline is not 100 %
        batches.append({"pixel_values": px, "labels": lb})
    same = lambda a, b: len(a) == len(b) and all(p.dtype == q.dtype and torch.equal(p, q) for p, q in zip(a, b))  # noqa: E731
    d_ints = [d_int] * depth
    for eng in (big, small):
        for chain in ("fp32", "bf16_ref"):
            for s_lim, q_lim, chunk in ((None, None, 2 * bsz), (4, 2, bsz), (2, 3, 2 * bsz)):
                ref_s = core.stage1_scores(eng, batches, d_ints, "pre_gelu", batch_limit=s_lim, score_chain=chain, chunk_images=2 * bsz)
                ref_c = core.depth_search_counts(eng, batches, depth, batch_limit=q_lim, chunk_images=chunk)
                got_s, got_c = core.prune_pass(eng, batches, d_ints, "pre_gelu", depth, score_limit=s_lim, search_limit=q_lim,
                                               score_chain=chain, chunk_images=2 * bsz, eval_chunk_images=chunk)
                assert same(got_s, ref_s), (precision, chain, s_lim, q_lim)
                assert got_c == ref_c, (precision, chain, s_lim, q_lim, got_c, ref_c)
                assert 0 < ref_c[0] <= ref_c[2]
    big.close(); small.close()


def test_set_layer_scale_refuses_a_bad_layer_branch_or_pointer(gpu):
    """With a live handle: SSP2_EINVAL (-1) for a layer out of range, a branch other than 0 / 1 and a null gamma, before the device is
    touched (the pointer handed over is never dereferenced); the engine's scales are left as they were."""
    import ctypes as C
    from ssp2vit.engine import VitEngine
    e = VitEngine(_w("vit_test_patch16_32_ls"), max_images=4)
    px = _px(4, 32).to(gpu)
    before = e.forward_logits(px).clone()
    fake = C.c_void_p(0x1000)
    for layer, branch, ptr in ((-1, 0, fake), (4, 0, fake), (0, -1, fake), (0, 2, fake), (0, 0, None), (3, 1, None)):
        assert e.lib.ssp2_set_layer_scale(e.h, layer, branch, ptr, 1) == -1, (layer, branch)
        assert e.lib.ssp2_last_error()
    assert e.lib.ssp2_set_layer_scale(None, 0, 0, fake, 1) == -1
    assert torch.equal(e.forward_logits(px), before)
    e.close()


# ------------------------------------------------------------------------------------------------------- 6. 1370 tokens
def test_dinov2_geometry_on_the_streaming_attention_vs_the_restatement(gpu):
    """vit_small_patch14_dinov2 cut to two blocks at 518 pixels: 1370 tokens on the key-streaming kernels (attn_stream=1), 2 images,
    logits and fp32-chain stage-1 scores against the CPU restatement within the long-sequence bars."""
    from oracle import ref_cpu
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch14_dinov2_d2", seed=12, std=0.02)
    model = build_layerscale(w)
    n, px = 2, _px(2, 518, seed=13)
    with pytest.raises(Exception, match="SSP2_OPT_ATTN_STREAM"):
        VitEngine(w, max_images=n, attn_stream=0)
    e = VitEngine(w, max_images=n, attn_stream=1)
    assert e.tokens == 1370
    got = e.forward_logits(px.to(gpu)).cpu()
    _check_logits(got, ref_cpu.logits_of(model, px).float(), "vit_small_patch14_dinov2_d2 stream")
    sc = e.forward_scores(px.to(gpu), "pre_gelu", "fp32")[0].cpu() / n
    for l, r in enumerate(ref_cpu.ffn_activation_importance(model, [{"pixel_values": px}], chain="fp32")):
        rel = (sc[l, :r.numel()] - r).abs() / r.abs().clamp_min(1e-3)
        print(f"[ls-long] block {l}: scores rel max {float(rel.max()):.2e} mean {float(rel.mean()):.2e}")
        assert float(rel.max()) <= 5e-3 and float(rel.mean()) <= 5e-4, (l, float(rel.max()), float(rel.mean()))
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 7. fp8
def test_fp8_layerscale_cut_tracks_the_bf16_engine(gpu):
    """The S/16 LayerScale cut in fp8 mode (out-projection and fc2 on the e4m3 EPI_RESID_LS form) within the existing fp8 bars: logits
    rel L2 <= 0.15, stage-1 scores mean rel <= 2 % / max <= 10 %, masks >= 95 % identical at a quarter pruned."""
    from ssp2vit.engine import VitEngine
    w = _w("vit_small_patch16_224_ls_d2", seed=8, spread=4.0)
    d_int = int(w["fc1_w.0"].shape[0])
    ref = VitEngine(w, max_images=64)
    f8 = VitEngine(w, max_images=64, precision="fp8")
    px = _px(64, 224, seed=4).to(gpu)
    lr, l8 = ref.forward_logits(px).cpu(), f8.forward_logits(px).cpu()
    rel = float((l8 - lr).norm() / lr.norm())
    sr, s8 = ref.forward_scores(px, "pre_gelu")[0].cpu(), f8.forward_scores(px, "pre_gelu")[0].cpu()
    err = (s8[:, :d_int] - sr[:, :d_int]).abs() / sr[:, :d_int].abs().clamp_min(1e-6)
    t = d_int // 4

    def cut(sc):                                                   # the t lowest scores are pruned
        m = torch.zeros(d_int, dtype=torch.bool)
        m[sc.argsort()[:t]] = True
        return m
    same = min(float((cut(sr[l, :d_int]) == cut(s8[l, :d_int])).float().mean()) for l in range(2))
    print(f"[ls-fp8] logits rel {rel:.4f}; scores rel mean {float(err.mean()):.4f} max {float(err.max()):.4f}; masks identical {same:.4f}")
    assert not torch.equal(l8, lr)
    assert rel <= 0.15 and float(err.mean()) <= 0.02 and float(err.max()) <= 0.10 and same >= 0.95
    ref.close(); f8.close()


# ----------------------------------------------------------------------------------------------- 8. API and CLI end to end
def test_reference_api_on_a_live_layerscale_module(gpu):
    from oracle import ref_cpu
    from ssp2vit import vit_pruning as vp, weights as W
    from ssp2vit.engine import VitEngine
    from ssp2vit.mask_conjunction import Auto2SSPInterface
    w = _w("vit_test_patch16_32_ls", seed=21, std=0.1)
    model = build_layerscale(w)
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
    assert pm.blocks[0].mlp.fc1.out_features == 96 and isinstance(pm.blocks[0].ls1, torch.nn.Module)
    flat = W.from_module(pm)
    assert all(f"ls{b}.{i}" in flat for b in (1, 2) for i in range(4)) and sum(bool(flat.get(f"attn_absent.{i}")) for i in range(4)) == 1
    e = VitEngine(flat, max_images=32)
    got = vp.engine_for(pm, "cuda", max_images=32).forward_logits(px.to(gpu))
    assert torch.equal(got, e.forward_logits(px.to(gpu)))
    _check_logits(got.cpu(), ref_cpu.logits_of(pm, px).float(), "pruned live module vs its own CPU forward")
    e.close()
    vp.release_engines(free=True)


def test_cli_layerscale_model_end_to_end(gpu, tmp_path):
    """auto_2ssp.py --model vit_test_patch16_32_ls (synthetic weights with LayerScale) prunes and writes its report; --weights reads the
    timm checkpoint of a LayerScale module back."""
    from ssp2vit.weights import synthetic_weights
    cli = os.path.join(PKG, "auto_2ssp.py")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    out = tmp_path / "out"
    common = ["--sparsity_rate", "0.25", "--min-remaining", "32", "--synthetic-calib", "64", "--eval-batches", "2", "--batch-size", "16",
              "--num-classes", "10"]
    r = subprocess.run([sys.executable, cli, "--model", "vit_test_patch16_32_ls", "--output-dir", str(out), *common],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert list(out.rglob("report-*.json")), "no report written"
    m = build_layerscale(synthetic_weights("vit_test_patch16_32_ls", classes=10, seed=4))
    ck = tmp_path / "ls.pth"
    torch.save(m.state_dict(), ck)
    r = subprocess.run([sys.executable, cli, "--weights", str(ck), "--heads", "4", "--output-dir", str(tmp_path / "o2"), *common],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
