"""The fp8 projections (csrc/gemm256.hip.h gemm256_bf16_kernel<EPI, SCORE, F8 = true>) and the weight quantiser
(csrc/misc.hip.h quant_rows_e4m3_kernel) on their own buffers (ssp2_linear_e4m3 / ssp2_quantise_rows_e4m3: the very launches of the
forward) against plain host statements of the same operations.  The statements and bounds below were written before the first GPU
run.  u = 2^-24 (fp32 unit roundoff); e4m3 is OCP e4m3fn (bias 7, 3 mantissa bits, +-448, 0x7f / 0xff NaN, no infinity).

Quantiser, bit for bit.  Row r: amax = max |w| over the row's cols bf16 values, scale = fl32(amax / 448) (1 for a zero row),
inv = fl32(1 / scale), byte = RNE e4m3 of clamp(fl32(w inv), +-448).  Pad columns [cols, ld8) and pad rows [rows, rows_pad) are zero
bytes, pad scales 1.  No byte is 0x7f or 0xff.  Rows whose amax is 448 * 2^k make w inv exact: they carry every e4m3 code, every
midpoint between neighbouring codes (ties to even) and the subnormal range; rows whose fl32(amax inv) rounds past 448 must land on
0x7e.  (torch's float8_e4m3fn cast rounds to nearest even and turns overflow into NaN: the host clamps first.)

Exact-arithmetic operands, bit for bit.  A and W hold e4m3 values k / 8, |k| <= 15: every product is a multiple of 2^-6 below 4, every
partial sum of K <= 3072 of them stays below 2^14, so the fp32 accumulation is exact in any order.  ascale (per row) and wscale (per
column) are powers of two, 2^-20 ... 2^20, neighbours orders of magnitude apart, so acc * ascale * wscale is exact too; the bias is bf16.
The only roundings left are the epilogue's fma and the casts:
  bf16      out = bf16(fl32(acc asc wsc + b))          (fl32 of the exact sum: float64 holds it within 53 >= 2 * 24 + 2 bits, so
                                                       rounding through float64 is innocuous)
  residual  x = fl32(xin + float(that))
  fc1       byte = e4m3(clamp(T[pre], +-448)), pre = that bf16 value, T = the kernel's own bf16 erf-GELU, tabulated over all 65 536 bf16
            values through ssp2_linear_bf16 with an identity weight (the same gelu_erf_pk).
The premise that the scaled f8f6f4 MFMA adds such products exactly is checked by these cases: 100 % of the elements must match.

Score slab.  Per 128-row tile and segment (the rows of the tile's first / second image, pad and out-of-range rows excluded) the
fp32 sum of squares of n <= 128 terms: |slab - S| <= (n + 1) u S + n 2^-126 against the float64 sum S of the predicted bf16 values (pre
for site 1, T[pre] for site 2).  A segment without rows must be exactly 0.  (The n 2^-126 term was added after the first GPU run: the
kernel flushes fp32 subnormal squares to zero — a one- or two-row segment whose GELU outputs are ~1e-20 came back 0 — and each term
it loses that way is below 2^-126.)

Realistic operands, against a float64 bound.  A: the LayerNorm's e4m3 bytes with its per-row ascale (QKV, fc1), e4m3(o * 16) with
ascale_const = 1/16 (out-projection), or GELU-like bytes with scale 1 (fc2); W: this quantiser's bytes of bf16 weights (std 0.02-0.05,
outlier rows), scales not powers of two.  Reference y = P asc wsc + b, P = sum_k a_k w_k over the DEQUANTISED bytes in float64
(products of 4-bit significands: float64 is exact to ~2^-50).  How the f8f6f4 MFMA aligns and adds the 64 products of one step is not
documented anywhere, so the step term is a MEASURED model, labelled as such:
  step  |error of one 64-deep step| <= 64 * ALIGN * max_j |p_j| with ALIGN = 2^-18 (the step keeps at least 18 bits below its largest
        product).  The first statement, ALIGN = 2^-23 (one 24-bit alignment), was exceeded up to 7.4x on the hardware, and 2^-20 still
        up to 1.6x.  With 2^-18 the worst ratio is 0.98: the step term is then no longer what decides, the one bf16 rounding 2^-8 |y|
        is tight against the bound (as in the LayerNorm test).  Each case prints its worst ratio against the 2^-23 model too ("r24"),
        so the hardware's behaviour is re-measured on every run.
  E_acc = sum_steps 64 ALIGN max_step |p| + (K / 64 + 1) u sum_k |p_k|          (plus the fp32 additions of the step results)
  c     = |asc wsc| (E_acc (1 + u) + u |P|) + u (|y| + |asc wsc| E_acc) + u |y|   (acc * asc, the fma rounding)
  bf16  |out - y| <= 2^-8 (|y| + c) + c
  resid |x - (xin + y)| <= 2^-8 (|y| + c) + c + u (|xin + y| + 2^-8 (|y| + c) + c)
The worst error / bound is printed per case.  (Treating e4m3 subnormal operands as flushed to zero fits the hardware worse: they are
honoured.)

Block wiring, bit for bit.  layers() of an fp8 engine on a two-block cut of S/16 (24 images, >= 4096 rows: every projection on e4m3
operands), contiguous and in the slab layout, with the stage-1 hook on a prefix of the slabs (the forward's split fc1 launch), with
the out-projection on bf16 (fp8_proj = 0), and on a pruned twin of ragged width 1030 (ld_int 1088, fc1 N = fc2 K = 1152), must equal
block by block the same block composed from the operator entries: LN1 (e4m3 + ascale) -> QKV (this quantiser's bytes, ascale) ->
attention (e4m3 output at the block's hand-off scale) -> residual with ascale_const = 1 / scale -> LN2 -> fc1 e4m3 -> fc2 residual.
Bit equality also shows that the device quantiser gives the bytes of the engine's own images (quantise_mat: the same kernel).

Guards.  Rows of x past M and output columns >= N hold a sentinel that must survive; ascale past M is NaN and rows of A past M hold
the e4m3 NaN code (reads are clamped to M - 1: no NaN may reach an output); the slab layout's pad rows of A hold NaN bytes and NaN
ascale (the scores must not see them); fc1 pad columns (pruned width: N = ceil128(ld_int) > d_int) must come out exactly 0.  The
forward's split fc1 launch (rows [M0, M) with A, ascale and out moved by M0 rows) must equal those rows of the whole launch bit for bit.
"""
import time

import pytest
import torch

from conftest import load_tiny_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN8 = 0x7F            # e4m3 NaN code
SENT = -77.0           # f32 / bf16 sentinel
SENT8 = 0x5A           # byte sentinel
GUARD = 5              # rows behind M


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from ssp2vit.engine import VitEngine
    w, _, _ = load_tiny_golden("timm")
    e = VitEngine(w, device="cuda:0", max_images=4)
    t0 = time.time()
    yield e
    print(f"\n[fp8 gemm numerics] module time {time.time() - t0:.1f} s")
    e.close()


DEC = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().double()   # byte -> value (NaN at 0x7f, 0xff)


def enc(v: torch.Tensor) -> torch.Tensor:
    """RNE e4m3 bytes of f32 values, saturating at +-448 (host, CPU)."""
    return v.detach().to("cpu", torch.float32).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def dec(b: torch.Tensor) -> torch.Tensor:
    return DEC.to(b.device)[b.long()]


@pytest.fixture(scope="module")
def gelu_table(eng):
    """T[bits] = the kernel's bf16 erf-GELU of the bf16 value with those bits (ssp2_linear_bf16, identity weight, 256 x 256 kernel)."""
    bits = torch.arange(65536, dtype=torch.int32)
    x = (bits << 16).view(torch.float32).to(torch.bfloat16).view(1024, 64).cuda()
    out = eng.linear(x, torch.eye(64), None, "gelu", kernel="big")
    torch.cuda.synchronize()
    return out.view(-1).cpu()


def bf16_bits(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF


# ---------------------------------------------------------------------------------------------------------------------- quantiser
def _quant_ref(w: torch.Tensor, rows_pad: int, ld8: int):
    wf = w.to(torch.bfloat16).float()
    rows, cols = wf.shape
    amax = wf.abs().amax(1)
    sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = 1.0 / sc
    b = torch.zeros(rows_pad, ld8, dtype=torch.uint8)
    b[:rows, :cols] = enc(wf * inv[:, None])
    s = torch.ones(rows_pad)
    s[:rows] = sc
    return b, s


def _quant_rows(cols: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    rows = []
    pos = DEC[1:0x7F].float()                                    # every positive finite code, 2^-9 .. 448
    # midpoints between neighbouring codes (ties; the subnormal ones among them), the tie 2^-10 between 0 and the smallest code, and
    # 3 * 2^-11 = 0.75 of that code (rounds up to it)
    mids = torch.cat([torch.tensor([2.0 ** -10, 3 * 2.0 ** -11]), (pos[:-1] + pos[1:]) / 2])
    grid = torch.cat([pos, -pos, mids, -mids, torch.tensor([0.0])])
    for k in range(-20, 21, 4):                                  # amax = 448 * 2^k: w * inv exact
        r = grid[torch.randperm(grid.numel(), generator=g)] * 2.0 ** k
        row = torch.zeros(cols)
        row[: min(cols, r.numel())] = r[:cols]
        row[cols - 1] = 448.0 * 2.0 ** k
        rows.append(row)
    # amaxes whose fl32(amax * inv) rounds past 448: the top code, never NaN
    bits = torch.arange(0x3C00, 0x3F80, dtype=torch.int32)      # bf16 values 2^-7 .. 1
    a = (bits << 16).view(torch.float32)
    past = a[(a * (1.0 / (a / 448.0))) > 448.0]
    assert past.numel() > 16
    for j in range(8):
        am = float(past[j * (past.numel() // 8)])
        row = (torch.rand(cols, generator=g) * 2 - 1) * am
        row[j * 7 % cols] = am if j % 2 else -am
        rows.append(row)
    rows.append(torch.zeros(cols))                               # all-zero row
    one = torch.zeros(cols); one[cols // 3] = -0.0371; rows.append(one)    # single non-zero entries
    one = torch.zeros(cols); one[0] = 3.0e4; rows.append(one)
    for j in range(40):                                          # random rows, std 0.02 .. 0.05, some with an outlier
        row = torch.randn(cols, generator=g) * (0.02 + 0.03 * j / 40)
        if j % 5 == 0:
            row[(j * 131) % cols] *= 40
        rows.append(row)
    return torch.stack(rows)


@pytest.mark.parametrize("cols,extra_pad", [(1030, 3), (768, 0), (128, 70), (3072, 1)])
def test_quantiser_bit_for_bit(eng, cols, extra_pad):
    w = _quant_rows(cols, seed=cols).to(torch.bfloat16)
    rows = w.shape[0]
    rows_pad = (rows + 255) // 256 * 256 if extra_pad == 0 else rows + extra_pad
    ld8 = (cols + 127) // 128 * 128
    w8, sc = eng.quantise_e4m3(w.cuda(), rows_pad=rows_pad, ld8=ld8)
    torch.cuda.synchronize()
    w8, sc = w8.cpu(), sc.cpu()
    rb, rs = _quant_ref(w, rows_pad, ld8)
    assert torch.equal(sc.view(torch.int32), rs.view(torch.int32)), "row scales differ from fl32(amax / 448)"
    bad = (w8 != rb)
    assert not bad.any(), f"{int(bad.sum())} bytes differ, first at {bad.nonzero()[:4].tolist()}: got {w8[bad][:4].tolist()} want {rb[bad][:4].tolist()}"
    assert not ((w8 & 0x7F) == 0x7F).any(), "NaN code written"
    # what the rows were built to reach: every code and the top code on the rows that round past 448
    if cols >= 512:
        assert len(set(w8[:11].flatten().tolist())) == 254
    assert all(int((w8[11 + j] & 0x7F).max()) == 0x7E for j in range(8))


# --------------------------------------------------------------------------------------------------------------- exact operands
def _exact_operands(M, N, K, seed, alo=-20, ahi=20, pad_rows=GUARD):
    g = torch.Generator().manual_seed(seed)
    ka = torch.randint(-15, 16, (M + pad_rows, K), generator=g)
    kw = torch.randint(-15, 16, (N, K), generator=g)
    a8 = enc(ka.float() / 8)
    a8[M:] = NAN8                                                # rows past M are never read
    w8 = enc(kw.float() / 8)
    e_a = torch.randint(alo, ahi + 1, (M,), generator=g)
    asc = torch.full((M + pad_rows,), float("nan"))
    asc[:M] = torch.pow(2.0, e_a.double()).float()
    wsc = torch.pow(2.0, torch.randint(alo, ahi + 1, (N,), generator=g).double()).float()
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).float()
    return ka, kw, a8, w8, asc, wsc, bias


def _exact_pre(ka, kw, asc, wsc, bias, M, ascale_const=0.0):
    """fl32(acc asc wsc + b) exactly: acc from the integer k's (exact in float64 on the device)."""
    acc = (ka[:M].cuda().double() @ kw.cuda().double().T) / 64.0
    s = asc[:M].cuda().double()[:, None] if ascale_const == 0.0 else ascale_const
    return (acc * s * wsc.cuda().double()[None, :] + bias.cuda().double()[None, :]).float()


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (255, 192, 256), (257, 320, 768), (4099, 1152, 3072), (12608, 768, 1152)])
def test_exact_operands_bf16_and_residual_bit_for_bit(eng, M, N, K, rev):
    ka, kw, a8, w8, asc, wsc, bias = _exact_operands(M, N, K, seed=M + N + K)
    a8d, w8d, ascd, wscd = a8.cuda(), w8.cuda(), asc.cuda(), wsc.cuda()
    pre = _exact_pre(ka, kw, asc, wsc, bias, M)
    want = pre.to(torch.bfloat16)
    out = torch.full((M + GUARD, N + 64), SENT, dtype=torch.bfloat16, device="cuda")
    eng.linear_e4m3(a8d, w8d, wscd, bias, "bf16", rows=M, ascale=ascd, out=out, rev=rev)
    same = out[:M, :N].view(torch.int16) == want.view(torch.int16)
    assert bool(same.all()), f"bf16 out: {int((~same).sum())} of {M * N} elements differ"
    assert bool((out[M:] == SENT).all()) and bool((out[:, N:] == SENT).all()), "wrote outside [M, N)"
    # residual, out of place through xin and in place
    g = torch.Generator().manual_seed(M)
    xin = torch.full((M + GUARD, N), SENT, device="cuda")
    xin[:M] = (torch.randn(M, N, generator=g) * 3).cuda()
    x = torch.full_like(xin, SENT)
    eng.linear_e4m3(a8d, w8d, wscd, bias, "resid", rows=M, ascale=ascd, x=x, xin=xin, rev=rev)
    wantx = xin[:M] + want.float()
    assert torch.equal(x[:M].view(torch.int32), wantx.view(torch.int32)), "residual (out of place) differs"
    assert bool((x[M:] == SENT).all()) and bool((xin[M:] == SENT).all())
    eng.linear_e4m3(a8d, w8d, wscd, bias, "resid", rows=M, ascale=ascd, x=xin, rev=1 - rev)
    assert torch.equal(xin[:M].view(torch.int32), wantx.view(torch.int32)), "residual (in place) differs"
    assert bool((xin[M:] == SENT).all())


@pytest.mark.parametrize("M,N,K", [(256, 64, 128), (4099, 768, 768)])
def test_exact_operands_constant_ascale_bit_for_bit(eng, M, N, K):
    """ascale_const = 1/16 (the out-projection's): every row scaled by it, no per-row array read."""
    ka, kw, a8, w8, asc, wsc, bias = _exact_operands(M, N, K, seed=7 * M + K)
    pre = _exact_pre(ka, kw, asc, wsc, bias, M, ascale_const=1.0 / 16)
    x = torch.full((M + GUARD, N), SENT, device="cuda")
    x[:M] = 0.25
    eng.linear_e4m3(a8.cuda(), w8.cuda(), wsc.cuda(), bias, "resid", rows=M, ascale_const=1.0 / 16, x=x)
    want = 0.25 + pre.to(torch.bfloat16).float()
    assert torch.equal(x[:M].view(torch.int32), want.view(torch.int32))
    assert bool((x[M:] == SENT).all())


def _fc1_bytes_want(pre: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    t = T[bf16_bits(pre.cpu())].float()
    return enc(t)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (257, 192, 256), (4099, 1152, 768), (12608, 3072, 768)])
def test_exact_operands_fc1_e4m3_bit_for_bit(eng, gelu_table, M, N, K, rev):
    ka, kw, a8, w8, asc, wsc, bias = _exact_operands(M, N, K, seed=3 * M + N, alo=-6, ahi=2)
    pre = _exact_pre(ka, kw, asc, wsc, bias, M)
    out = torch.full((M + GUARD, N + 64), SENT8, dtype=torch.uint8, device="cuda")
    eng.linear_e4m3(a8.cuda(), w8.cuda(), wsc.cuda(), bias, "gelu", rows=M, ascale=asc.cuda(), out=out, rev=rev)
    got = out.cpu()
    want = _fc1_bytes_want(pre, gelu_table)
    same = got[:M, :N] == want
    assert bool(same.all()), f"fc1 bytes: {int((~same).sum())} of {M * N} differ, first at {(~same).nonzero()[:4].tolist()}"
    assert bool((got[M:] == SENT8).all()) and bool((got[:, N:] == SENT8).all()), "wrote outside [M, N)"
    if M > 256:                                                  # neither saturated nor zero for the most part
        assert float(((want & 0x7F != 0x7E) & (want & 0x7F != 0)).float().mean()) > 0.2


# ------------------------------------------------------------------------------------------------------------------ score slab
def _slab_ref(sv: torch.Tensor, M: int, tokens: int, group: int, n_img: int, slab_ld: int):
    """float64 sums of squares per (128-row tile, segment) and the number of terms, from the kernel's row -> sample rule."""
    from ssp2vit.engine import ssp2_rows
    m = torch.arange(M)
    if group > 0 and group < n_img:
        mpad = -(-group * tokens // 128) * 128
        sbk = m // mpad
        ml = m - sbk * mpad
        img_in = ml // tokens
        valid = img_in < torch.clamp(n_img - sbk * group, max=group)
        sample = sbk * (group + 1) + img_in                    # distinct per slab; pad rows are invalid anyway
        first_sample = sbk * (group + 1) + ((m // 128) * 128 - sbk * mpad) // tokens
    else:
        valid = torch.ones(M, dtype=torch.bool)
        sample = m // tokens
        first_sample = ((m // 128) * 128) // tokens
    assert M >= ssp2_rows(n_img, tokens, group)
    seg = (sample - first_sample).clamp(0, 1)
    assert bool(((sample - first_sample)[valid] <= 1).all())
    nt = 2 * ((M + 255) // 256)
    S = torch.zeros(nt, 2, slab_ld, dtype=torch.float64, device=sv.device)
    cnt = torch.zeros(nt, 2, dtype=torch.float64)
    v = sv[:, :slab_ld].double() ** 2
    tile = m // 128
    for t in range(nt):
        for s in range(2):
            sel = valid & (tile == t) & (seg == s)
            cnt[t, s] = float(sel.sum())
            if sel.any():
                S[t, s] = v[sel.to(sv.device)].sum(0)
    return S, cnt


@pytest.mark.parametrize("tokens,n_img,group", [(128, 5, 0), (130, 7, 0), (197, 7, 0), (257, 5, 0), (197, 7, 3), (130, 9, 4),
                                                (257, 5, 2), (197, 21, 4)])
@pytest.mark.parametrize("site", [1, 2])
def test_score_slab_against_float64(eng, gelu_table, tokens, n_img, group, site):
    from ssp2vit.engine import ssp2_rows
    M = ssp2_rows(n_img, tokens, group)
    N, K, slab_ld = 320, 256, 300
    ka, kw, a8, w8, asc, wsc, bias = _exact_operands(M, N, K, seed=tokens * 31 + n_img + group, alo=-6, ahi=2)
    # slab pad rows: NaN bytes and NaN scales — never counted
    if group > 0 and group < n_img:
        mpad = -(-group * tokens // 128) * 128
        m = torch.arange(M)
        sbk = m // mpad
        pad = (m - sbk * mpad) >= torch.clamp(n_img - sbk * group, max=group) * tokens
        a8[:M][pad] = NAN8
        asc[:M][pad] = float("nan")
    else:
        pad = torch.zeros(M, dtype=torch.bool)
    assert bool(pad.any()) == (group > 0 and group < n_img and (group * tokens) % 128 != 0)
    ka_pre = ka.clone(); ka_pre[:M][pad] = 0
    asc_pre = asc.clone(); asc_pre[:M][pad] = 1.0
    pre = _exact_pre(ka_pre, kw, asc_pre, wsc, bias, M)
    pre_b = pre.to(torch.bfloat16)
    sv = pre_b.float() if site == 1 else gelu_table[bf16_bits(pre.cpu())].float().cuda()
    out = torch.full((M + GUARD, N), SENT8, dtype=torch.uint8, device="cuda")
    out, slab = eng.linear_e4m3(a8.cuda(), w8.cuda(), wsc.cuda(), bias, "gelu", rows=M, ascale=asc.cuda(), out=out,
                                score_site=site, tokens=tokens, group=group, n_img=n_img, slab_ld=slab_ld)
    got = out.cpu()
    want = _fc1_bytes_want(pre, gelu_table)
    ok = ~pad
    assert bool((got[:M][ok] == want[ok]).all()), "fc1 bytes of the scoring epilogue differ"
    assert bool((got[M:] == SENT8).all())
    S, cnt = _slab_ref(sv, M, tokens, group, n_img, slab_ld)
    err = (slab.double() - S).abs()
    bound = (cnt.cuda()[:, :, None] + 1) * U * S + cnt.cuda()[:, :, None] * 2.0 ** -126
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert bool(torch.isfinite(slab).all()), "slab holds NaN: a pad row or an unwritten entry"
    assert bool((err <= bound).all()), f"slab error / bound {ratio:.3g} (site {site}, tokens {tokens}, group {group})"
    print(f"\n[slab site {site} tokens {tokens} n {n_img} group {group}] worst error / bound {ratio:.3f}")


# --------------------------------------------------------------------------------------------------------------- split launch
def test_split_fc1_launch_equals_the_whole_launch(eng):
    """The kernel side of the forward's fused stage-1 + search launch: the scored slabs [0, M0) with the scoring epilogue, the rest
    [M0, M) without it, A / ascale / out moved by M0 rows (bytes) here in Python.  Rows [M0, M) and the scored slabs' slab entries must
    equal the whole launch.  That the forward itself moves A, ascale and out this way is pinned by the block-wiring test below."""
    from ssp2vit.engine import ssp2_rows
    tokens, group, n_img, n_pref = 197, 4, 24, 8
    M = ssp2_rows(n_img, tokens, group)
    mpad = -(-group * tokens // 128) * 128
    M0 = (n_pref // group) * mpad
    N, K = 1152, 768
    g = torch.Generator().manual_seed(11)
    a8 = enc(torch.randn(M + GUARD, K, generator=g) * 60)
    a8[M:] = NAN8
    asc = torch.full((M + GUARD,), float("nan"))
    asc[:M] = torch.rand(M, generator=g) * 0.02 + 0.001
    w8 = enc(torch.randn(N, K, generator=g) * 100)
    wsc = torch.rand(N, generator=g) * 1e-3 + 1e-4
    bias = torch.randn(N, generator=g) * 0.1
    a8d, ascd, w8d, wscd = a8.cuda(), asc.cuda(), w8.cuda(), wsc.cuda()
    full, slab_full = eng.linear_e4m3(a8d, w8d, wscd, bias, "gelu", rows=M, ascale=ascd, score_site=1, tokens=tokens, group=group,
                                      n_img=n_img, slab_ld=N)
    plain_full = eng.linear_e4m3(a8d, w8d, wscd, bias, "gelu", rows=M, ascale=ascd)
    out = torch.full((M + GUARD, N), SENT8, dtype=torch.uint8, device="cuda")
    _, slab0 = eng.linear_e4m3(a8d, w8d, wscd, bias, "gelu", rows=M0, ascale=ascd, out=out, score_site=1, tokens=tokens,
                               group=group, n_img=n_pref, slab_ld=N)
    eng.linear_e4m3(a8d[M0:], w8d, wscd, bias, "gelu", rows=M - M0, ascale=ascd[M0:], out=out[M0:])
    assert torch.equal(out[:M], plain_full[:M]), "split launch differs from the whole launch"
    assert torch.equal(full[:M0], plain_full[:M0]), "the scoring epilogue's bytes differ from the plain epilogue's"
    assert bool((out[M:] == SENT8).all())
    t0 = M0 // 128
    assert torch.equal(slab0[:t0], slab_full[:t0]), "slab of the scored prefix differs"


# ------------------------------------------------------------------------------------------------------- pruned fc1 width
def test_pruned_fc1_pad_columns_are_zero(eng, gelu_table):
    """d_int = 1030: ld_int = 1088, the fp8 fc1 writes N = ceil128(ld_int) = 1152 columns from the quantised weight image (rows past
    d_int: zero bytes, scale 1, bias 0); the pad columns must be exactly 0 for fc2, which reads them as K."""
    M, K, d_int = 4099, 384, 1030
    ld8_int = ((d_int + 63) // 64 * 64 + 127) // 128 * 128
    assert ld8_int == 1152
    g = torch.Generator().manual_seed(5)
    w = torch.randn(d_int, K, generator=g) * 0.04
    w8, wsc = eng.quantise_e4m3(w)
    assert w8.shape[0] >= ld8_int and bool((w8[d_int:] == 0).all()) and bool((wsc[d_int:] == 1).all())
    bias = torch.zeros(ld8_int)
    bias[:d_int] = torch.randn(d_int, generator=g) * 0.02
    a8 = enc(torch.randn(M, K, generator=g) * 100).cuda()
    asc = (torch.rand(M, generator=g) * 0.02 + 0.005).cuda()
    out = torch.full((M, ld8_int), SENT8, dtype=torch.uint8, device="cuda")
    eng.linear_e4m3(a8, w8[:ld8_int], wsc[:ld8_int], bias, "gelu", ascale=asc, out=out)
    assert bool((out[:, d_int:] == 0).all()), "fc1 pad columns are not zero"
    assert float((out[:, :d_int] != 0).float().mean()) > 0.3


# ------------------------------------------------------------------------------------------------------- realistic operands
ALIGN = 2.0 ** -18     # MEASURED model of one 64-deep f8f6f4 step (see the docstring): the 24-bit statement, 2^-23, was exceeded 7x


def _bound_acc(a_deq: torch.Tensor, w_deq: torch.Tensor):
    """P and the accumulation bounds of the 2^-23 statement and of the ALIGN model (float64, one row block at a time)."""
    K = a_deq.shape[1]
    P = a_deq @ w_deq.T
    S = a_deq.abs() @ w_deq.abs().T
    step = torch.zeros_like(P)
    for s in range(K // 64):
        prod = a_deq[:, None, 64 * s:64 * s + 64].abs() * w_deq[None, :, 64 * s:64 * s + 64].abs()
        step += prod.amax(-1)
    add = (K / 64 + 1) * U * S
    return P, 64 * ALIGN * step + add, 64 * 2.0 ** -23 * step + add


def _out_bounds(P, E, sw, bias, xin):
    y = P * sw + bias
    c = sw.abs() * (E * (1 + U) + U * P.abs()) + U * (y.abs() + sw.abs() * E) + U * y.abs()
    bb = 2.0 ** -8 * (y.abs() + c) + c
    return y, bb, bb + U * ((xin + y).abs() + bb)


@pytest.mark.parametrize("M,N,K,form", [(255, 192, 256, "ln"), (4099, 320, 768, "ln"), (257, 1152, 1152, "ln"), (12608, 3072, 768, "ln"),
                                        (4099, 768, 3072, "none"), (12608, 64, 128, "const"), (4099, 768, 768, "const")])
def test_realistic_operands_against_float64(eng, M, N, K, form):
    """A: "ln" the LayerNorm's e4m3 bytes + per-row ascale (QKV, fc1); "const" e4m3(o * 16) with ascale_const = 1/16 (out-projection);
    "none" GELU-like e4m3 activations with scale 1 (fc2).  W: this quantiser's bytes.  Bound: the docstring's, with the ALIGN model."""
    g = torch.Generator().manual_seed(M + K)
    a8 = torch.full((M + GUARD, K), NAN8, dtype=torch.uint8, device="cuda")
    ascd = None
    if form == "const":                                          # the e4m3 attention output: e4m3(o * 16)
        a8[:M] = enc(torch.randn(M, K, generator=g) * 4.0).cuda()
    elif form == "none":                                         # the fc1 -> fc2 hand-off: GELU output bytes, no scale
        a8[:M] = enc(torch.relu(torch.randn(M, K, generator=g)) * 3.0 - 0.1).cuda()
    else:
        x = torch.randn(M + GUARD, K, generator=g)
        x[:, 5] += 30.0                                          # an outlier channel
        gamma = 1.0 + 0.3 * torch.randn(K, generator=g)
        beta = 0.05 * torch.randn(K, generator=g)
        ascd = torch.full((M + GUARD,), float("nan"), device="cuda")
        eng.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), 1e-6, rows=M, out=a8, ascale=ascd)
    w = torch.randn(N, K, generator=g) * (0.02 + 0.03 * torch.rand(N, 1, generator=g))
    w[::17] *= 8.0                                               # outlier rows
    w8, wsc = eng.quantise_e4m3(w)
    w8, wsc = w8[:N], wsc[:N]
    bias = (torch.randn(N, generator=g) * 0.02).to(torch.bfloat16).float()
    kw = dict(ascale=ascd) if form == "ln" else dict(ascale_const=1.0 / 16 if form == "const" else 0.0)
    out = torch.full((M + GUARD, N + 64), SENT, dtype=torch.bfloat16, device="cuda")
    eng.linear_e4m3(a8, w8, wsc, bias, "bf16", rows=M, out=out, **kw)
    xin = (torch.randn(M + GUARD, N, generator=g) * 2).cuda()
    xin[M:] = SENT
    xo = torch.full_like(xin, SENT)
    eng.linear_e4m3(a8, w8, wsc, bias, "resid", rows=M, x=xo, xin=xin, **kw)
    asc = ascd[:M].double() if form == "ln" else torch.full((M,), 1.0 / 16 if form == "const" else 1.0, dtype=torch.float64, device="cuda")
    w_deq = dec(w8).double()
    bd = bias.cuda().double()[None, :]
    worst_b = worst_r = worst_24 = 0.0
    for r0 in range(0, M, 512):
        r1 = min(M, r0 + 512)
        P, E, E24 = _bound_acc(dec(a8[r0:r1]).double(), w_deq)
        sw = asc[r0:r1, None] * wsc.double()[None, :]
        xi = xin[r0:r1].double()
        y, bb, br = _out_bounds(P, E, sw, bd, xi)
        eb = (out[r0:r1, :N].double() - y).abs()
        assert bool(torch.isfinite(eb).all()), "non-finite output: a NaN scale or row past M was read"
        worst_b = max(worst_b, float((eb / bb).max()))
        worst_r = max(worst_r, float(((xo[r0:r1].double() - (xi + y)).abs() / br).max()))
        worst_24 = max(worst_24, float((eb / _out_bounds(P, E24, sw, bd, xi)[1]).max()))
    print(f"\n[realistic M={M} N={N} K={K} {form}] worst error / bound: bf16 {worst_b:.3f}, resid {worst_r:.3f} (r24: {worst_24:.2f})")
    assert worst_b <= 1.0 and worst_r <= 1.0
    assert bool((out[M:] == SENT).all()) and bool((out[:, N:] == SENT).all()) and bool((xo[M:] == SENT).all())


# --------------------------------------------------------------------------------------------------------------- block wiring
BLOCK_N = 24


@pytest.fixture(scope="module")
def fp8_block_engines():
    """An fp8 engine on the S/16 two-block cut and its pruned twin of widths (1030, 1536), with the weights (flat dictionary) and the
    kept neurons of the twin's block 0."""
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    w = synthetic_weights("vit_small_patch16_224_d2", classes=10, seed=3, std=0.03, bias_std=0.02, spread=4.0)
    dense = VitEngine(w, max_images=BLOCK_N, precision="fp8")
    d_int = int(w["fc1_w.0"].shape[0])
    g = torch.Generator().manual_seed(9)
    keep0 = torch.sort(torch.randperm(d_int, generator=g)[:1030]).values
    masks = [torch.ones(d_int, dtype=torch.int32), torch.zeros(d_int, dtype=torch.int32)]
    masks[0][keep0] = 0
    twin = dense.pruned_twin([1030, d_int], max_images=BLOCK_N)
    dense.apply_ffn_into(twin, masks)
    twin._bind_stream()
    twin._check(twin.lib.ssp2_set_precision(twin.h, 1))         # a twin is created bf16: its e4m3 images from the pruned weights (quantise_mat)
    torch.cuda.synchronize()
    keeps = [keep0, torch.arange(d_int)]
    yield w, dense, twin, keeps
    twin.close()
    dense.close()


def _compose_block(op, w, l, x, n, tokens, group, heads, scale, keep):
    """Block l of the fp8 forward on x (f32 [M, D], updated and returned) from operator calls; scale: the block's attention hand-off
    scale (None: out-projection on bf16)."""
    from ssp2vit.engine import ssp2_rows
    D = int(w["dim"])
    eps = float(w["eps"])
    M = ssp2_rows(n, tokens, group)
    ld8 = (D + 127) // 128 * 128
    dev = lambda t: t.to("cuda", torch.float32).contiguous()  # noqa: E731

    def ln(gk, bk):
        h8 = torch.zeros(M, ld8, dtype=torch.uint8, device="cuda")
        hs = torch.empty(M, device="cuda")
        op.layernorm(x, dev(w[f"{gk}.{l}"]), dev(w[f"{bk}.{l}"]), eps, rows=M, out=h8, ascale=hs)
        return h8, hs

    def q8(wt, rows):
        b, s = op.quantise_e4m3(wt)
        return b[:rows], s[:rows]

    h8, hs = ln("ln1_g", "ln1_b")
    qw, qs = q8(w[f"qkv_w.{l}"], 3 * D)
    qkv = op.linear_e4m3(h8, qw, qs, w[f"qkv_b.{l}"], "bf16", ascale=hs)
    if scale is not None:
        o8 = torch.zeros(M, ld8, dtype=torch.uint8, device="cuda")
        op.attention(qkv, n, tokens, heads, D // heads, group=group, out8=o8, out8_scale=scale)
        pw, ps = q8(w[f"proj_w.{l}"], D)
        op.linear_e4m3(o8, pw, ps, w[f"proj_b.{l}"], "resid", ascale_const=1.0 / scale, x=x)
    else:
        o = op.attention(qkv, n, tokens, heads, D // heads, group=group)
        op.linear(o, w[f"proj_w.{l}"], w[f"proj_b.{l}"], "resid", x=x)
    h8, hs = ln("ln2_g", "ln2_b")
    d = keep.numel()
    ld8_int = ((d + 63) // 64 * 64 + 127) // 128 * 128          # ceil128(ld_int): fc1's N, fc2's K
    fw, fs = op.quantise_e4m3(w[f"fc1_w.{l}"][keep])
    fb = torch.zeros(ld8_int)
    fb[:d] = w[f"fc1_b.{l}"][keep]
    act = op.linear_e4m3(h8, fw[:ld8_int], fs[:ld8_int], fb, "gelu", ascale=hs)
    assert bool((act[:, d:] == 0).all()), "fc1 pad columns"
    f2w, f2s = op.quantise_e4m3(w[f"fc2_w.{l}"][:, keep])
    assert f2w.shape[1] == ld8_int
    op.linear_e4m3(act, f2w[:D], f2s[:D], w[f"fc2_b.{l}"], "resid", x=x)
    return x


@pytest.mark.parametrize("which,group,prefix,fp8_proj", [("dense", 0, 0, 1), ("dense", 4, 0, 1), ("dense", 4, 8, 1), ("dense", 0, 0, 0),
                                                          ("twin", 0, 0, 1), ("twin", 4, 8, 1)])
def test_fp8_blocks_equal_their_operator_composition(fp8_block_engines, which, group, prefix, fp8_proj):
    """layers() block by block against the block composed from operator calls, bit for bit on every image row (see the docstring).
    prefix > 0: the stage-1 hook on the first `prefix` images (whole slabs) — the forward splits fc1 at M0 and moves A, ascale and out."""
    from ssp2vit.engine import ssp2_rows
    w, dense, twin, keeps = fp8_block_engines
    e = dense if which == "dense" else twin
    n, tokens, heads = BLOCK_N, e.tokens, int(w["heads"])
    M = ssp2_rows(n, tokens, group)
    assert M >= 4096                                             # every projection of the launch runs on e4m3 operands
    img = torch.zeros(M, dtype=torch.bool)
    mpad = -(-group * tokens // 128) * 128 if group else 0
    for i in range(n):
        r = (i // group) * mpad + (i % group) * tokens if group else i * tokens
        img[r:r + tokens] = True
    g = torch.Generator().manual_seed(M + prefix)
    x = (torch.randn(M, int(w["dim"]), generator=g) * img[:, None]).cuda()
    e.set_option("fp8_proj", fp8_proj)
    try:
        for l in range(int(w["depth"])):
            keep = keeps[l] if which == "twin" else torch.arange(int(w[f"fc1_w.{l}"].shape[0]))
            xr = x.clone()
            if prefix:
                e.layers(x, n, l, l + 1, score_site="pre_gelu", score_group=group, score_images=prefix)
            else:
                e.layers(x, n, l, l + 1, score_group=group)
            scale = e.lib.ssp2_fp8_attn_scale(e.h, l) if fp8_proj else None
            _compose_block(dense, w, l, xr, n, tokens, group, heads, scale, keep)
            torch.cuda.synchronize()
            diff = (x[img.cuda()] != xr[img.cuda()])
            assert not bool(diff.any()), f"block {l}: {int(diff.sum())} of {int(img.sum()) * x.shape[1]} elements differ"
            assert bool(torch.isfinite(x[img.cuda()]).all())
            x = torch.where(img.cuda()[:, None], x, torch.zeros_like(x))
    finally:
        e.set_option("fp8_proj", 1)
