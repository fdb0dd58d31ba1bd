"""The bf16 projections — gemm_bf16_kernel<EPI, SCORE> (csrc/gemm.hip.h, 128 x 128 tiles) and gemm256_bf16_kernel<EPI, SCORE, false>
(csrc/gemm256*.hip.h, 256 x 256 tiles) — on their own buffers (ssp2_linear_bf16_ex / ssp2_linear_ls_bf16: the very launches of the
forward) against plain float64 statements of the same operations.  The statements and bounds below were written before the first GPU
run.  u = 2^-24 (fp32 unit roundoff).

Exact-arithmetic operands, bit for bit, 100 % of the elements.  A and W hold bf16 values k / 8, |k| <= 15, drawn per element: every
product is a multiple of 2^-6 below 4, every partial sum of K <= 3072 of them stays below 2^14, so the fp32 accumulation is exact in
any order; the bias is bf16-representable.  The only roundings left are the epilogue's:
  bf16      out = bf16(fl32(acc + b))                  (acc + b spans fewer than 53 bits: float64 holds it, .float() is fl32)
  residual  x = fl32(xin + float(out)), xin a buffer of its own (x pre-filled with NaN: written, never read) and in place
  LayerScale x = fl32(xin + fl32(gamma * float(out))), gamma fp32 and not a power of two (24 x 8 bits: the product is exact in float64)
  fc1       out = T[pre], pre = that bf16 value, T = the kernel's own bf16 erf-GELU tabulated over all 65 536 bf16 values through an
            identity weight (T itself against erf: tests/test_gpu_parity.py test_gelu_epilogue_on_every_bf16_value); out2 == pre
            (128 x 128 kernel).  The fc1 cases run on A / 8 (still exact) so that the pre-activations sit where GELU bends.
Both kernels (the 256 x 256 one on every shape: the entry accepts them all), rev 0 and 1; the two kernels' buffers must be
torch.equal, sentinels included.  Shapes: M in 1, 63, 127, 128, 129, 255, 256, 257, 300, 4099 and the ragged many-tile 12608 x 768 x
1152; N in 64, 192, 320, 768 (partial 128- and 256-column tiles); K in 64 .. 256 (one to three K-tiles of the small kernel, fewer than
four of the large one) and 3072.

Guards, in the same cases.  A: lda = K + 8, GUARD = 5 rows behind M; gap columns and rows past M hold NaN.  W: ldw = K + 8, NaN in the
gap, rows N .. ceil256(N) zero (the contract).  out / out2: ldo = N + 8; x / xin: ldx = N + 4; rows past M and columns past N hold a
sentinel that must survive.  No NaN in any output element of a row below M (bit equality with the NaN-free prediction says so).

Score slab, both sites, both kernels.  Per 128-row entry and segment (the rows of the entry's first / second image; the slab layout's
pad rows and rows behind the last image count nowhere) the fp32 sum of squares of n <= 128 terms:
  |slab - S| <= (n + 1) u S + n 2^-126
against the float64 sum S of the predicted bf16 values (pre for site 1, T[pre] for site 2; the operands are exact, so the prediction
is) — the fp8 module's statement, its subnormal-flush term included.  A segment without rows must be exactly 0, every entry of the
[2 ceil(M / 256), 2, slab_ld] slab is written, and the two kernels' slabs are bit-identical.  Image i's rows are scaled by 2^(i mod 3)
and each image's first and last row carry the largest magnitudes (|k| 12 .. 15 against <= 5): a boundary row credited to the
neighbouring image, or dropped, errs by orders of magnitude more than the bound.  Pad rows of A hold NaN.  N = 192 with slab_ld = 192
and N = 320 with slab_ld = 264, where the weight rows (= output columns) at and past slab_ld are NaN: a column the slab does not have
must not be written into the next entry.  Once M is larger than the layout (600 more rows of valid data: they count nowhere).
The forward's split fc1 launch — the hooked prefix of whole slabs, then rows [M0, M) without the hook — must equal the whole launch
bit for bit, slab entries of the prefix included.

Realistic operands against float64.  A: LayerNorm-like bf16 rows with outlier channels (x 100 in a few columns); W: std 0.02 .. 0.05
with outlier rows (x 8); bias bf16.  y = sum_k a_k w_k + b in float64 over the bf16 values.
  E_acc = (K + 1) u sum_k |a_k w_k|                    (correctly rounded fp32 additions in any order)
  c     = E_acc + u (|y| + E_acc)                      (the bias add)
  bf16  |out - y| <= 2^-8 (|y| + c) + c
  resid |x - (xin + y)| <= 2^-8 (|y| + c) + c + u |xin + y|
How the bf16 MFMA rounds inside one instruction is not documented; a ratio above 1 would be answered by widening E_acc by at most 2
(truncating adds) and saying so here.  Each case also prints its worst ratio against the older test's model, 2^-8 |y| + 2e-6 sum|terms|
("old"), so the hardware's behaviour is on record.

After the first GPU run nothing above had to change: every exact case came back at 100 % identical bits on both kernels and both walk
directions, every sentinel intact.  Measured worst error / bound: slab 0.333 (site 1) and 0.387 (site 2), the same on both kernels;
realistic operands 0.983 / 0.975 / 0.962 / 0.867 for the four shapes, bf16 and residual alike (the one bf16 rounding, 2^-8 |y|, is what
sits against the bound; E_acc stayed as stated, no widening for truncating adds was needed) and 0.990 .. 0.995 against the older model.
One thing the entry does for the slab statement: the 128 x 128 kernel has no tile for the odd last 128-row entry of a
[2 ceil(M / 256)] slab, so ssp2_linear_bf16_ex zeroes that entry before the launch (the 256 x 256 kernel writes it itself).  Planted
defects, each run once: `bnd` + 1 in the 128 x 128 kernel's score epilogue (an image's last row credited to the previous image) fails
every layout but tokens = 128 by 1e7 .. 1e39 times the bound.
"""
import functools
import time

import pytest
import torch

from conftest import load_tiny_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -77.0           # f32 / bf16 sentinel
GUARD = 5              # rows behind M
NAN = float("nan")
KERNELS = ("small", "big")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from ssp2vit.engine import VitEngine
    w, _, _ = load_tiny_golden("timm")
    e = VitEngine(w, device="cuda:0", max_images=4)
    t0 = time.time()
    yield e
    _exact_case.cache_clear()
    print(f"\n[bf16 gemm numerics] module time {time.time() - t0:.1f} s")
    e.close()


@pytest.fixture(scope="module")
def gelu_table(eng):
    """T[bits] = the kernel's bf16 erf-GELU of the bf16 value with those bits (identity weight, 256 x 256 kernel), on the device."""
    bits = torch.arange(65536, dtype=torch.int32)
    x = (bits << 16).view(torch.float32).to(torch.bfloat16).view(1024, 64).cuda()
    out = eng.linear(x, torch.eye(64), None, "gelu", kernel="big")
    torch.cuda.synchronize()
    return out.view(-1).clone()


def bf16_bits(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF


def _same_bits(got: torch.Tensor, want: torch.Tensor, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    v = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    bad = got.contiguous().view(v) != want.contiguous().view(v)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[:4].tolist()}"


def _buffers(ka: torch.Tensor, kw: torch.Tensor, scale: float = 0.125):
    """A [M + GUARD, K + 8] and W [ceil256(N), K + 8] on the device from integer k's (value k * scale): NaN in the gap columns and in
    the rows of A past M, zero in the rows of W past N.  Returns the buffers and the operand views the entry gets."""
    M, K = ka.shape
    N = kw.shape[0]
    A = torch.full((M + GUARD, K + 8), NAN, dtype=torch.bfloat16, device="cuda")
    A[:M, :K] = (ka.float() * scale).to(torch.bfloat16).cuda()
    W = torch.zeros((N + 255) // 256 * 256, K + 8, dtype=torch.bfloat16, device="cuda")
    W[:N, K:] = NAN
    W[:N, :K] = (kw.float() * 0.125).to(torch.bfloat16).cuda()
    return A, W, A[:, :K], W[:N, :K]


def _sent(rows, cols, dtype):
    return torch.full((rows, cols), SENT, dtype=dtype, device="cuda")


def _guards_ok(buf: torch.Tensor, M: int, N: int, what: str):
    assert bool((buf[M:] == SENT).all()), f"{what}: rows past M were written"
    assert bool((buf[:, N:] == SENT).all()), f"{what}: columns past N were written"


# --------------------------------------------------------------------------------------------------------------- exact operands
@functools.lru_cache(maxsize=1)
def _exact_case(M, N, K):
    """Operands, buffers and the float64 predictions of one shape (shared by the rev = 0 / 1 cases; never modified)."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    ka = torch.randint(-15, 16, (M, K), generator=g)
    kw = torch.randint(-15, 16, (N, K), generator=g)
    A, W, a, w = _buffers(ka, kw)
    Ag, _, ag, _ = _buffers(ka, kw, scale=2.0 ** -6)            # fc1: A / 8
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).float()
    acc = (ka.cuda().double() @ kw.cuda().double().T) / 64.0
    b = bias.cuda().double()[None, :]
    pre = (acc + b).float().to(torch.bfloat16)                   # bf16(fl32(acc + b))
    pre_g = (acc / 8.0 + b).float().to(torch.bfloat16)
    xin = _sent(M + GUARD, N + 4, torch.float32)
    xin[:M, :N] = (torch.randn(M, N, generator=g) * 3).cuda()
    gamma = (0.1 + 1.3 * torch.rand(N, generator=g)).float()
    assert not bool((torch.frexp(gamma)[0] == 0.5).any())         # no power of two
    xi = xin[:M, :N].double()
    want_x = (xi + pre.double()).float()
    want_ls = (xi + (gamma.cuda().double()[None, :] * pre.double()).float().double()).float()
    return dict(A=A, W=W, a=a, w=w, Ag=Ag, ag=ag, bias=bias, pre=pre, pre_g=pre_g, xin=xin, gamma=gamma, want_x=want_x, want_ls=want_ls,
                a_dense=a[:M].contiguous(), w_dense=w.contiguous())


EXACT_SHAPES = [(1, 64, 64), (63, 192, 128), (127, 320, 192), (128, 64, 256), (129, 768, 64), (255, 192, 3072), (256, 320, 128),
                (257, 64, 192), (300, 768, 256), (4099, 192, 64), (4099, 320, 3072), (12608, 768, 1152)]


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_operands_every_form_bit_for_bit(eng, gelu_table, M, N, K, rev):
    c = _exact_case(M, N, K)
    xin0 = c["xin"].clone()
    want_g = gelu_table[bf16_bits(c["pre_g"])]
    res = {}
    for kern in KERNELS:
        kw = dict(rows=M, kernel=kern, rev=rev)
        out = _sent(M + GUARD, N + 8, torch.bfloat16)
        eng.linear_ex(c["a"], c["w"], c["bias"], "bf16", out=out, **kw)
        _same_bits(out[:M, :N], c["pre"], f"{kern} bf16 out")
        _guards_ok(out, M, N, f"{kern} bf16 out")
        # residual through xin: x is written, never read
        x = _sent(M + GUARD, N + 4, torch.float32)
        x[:M, :N] = NAN
        eng.linear_ex(c["a"], c["w"], c["bias"], "resid", x=x, xin=c["xin"], **kw)
        _same_bits(x[:M, :N], c["want_x"], f"{kern} residual through xin")
        _guards_ok(x, M, N, f"{kern} residual x")
        # ... and in place, walking the other way
        xp = c["xin"].clone()
        eng.linear_ex(c["a"], c["w"], c["bias"], "resid", x=xp, rows=M, kernel=kern, rev=1 - rev)
        _same_bits(xp[:M, :N], c["want_x"], f"{kern} residual in place")
        _guards_ok(xp, M, N, f"{kern} residual in place")
        # LayerScale (ssp2_linear_ls_bf16: dense operands, x / xin at ldx = N + 4)
        xl = _sent(M + GUARD, N + 4, torch.float32)
        xl[:M, :N] = NAN
        eng.linear(c["a_dense"], c["w_dense"], c["bias"], "resid", x=xl, kernel=kern, gamma=c["gamma"], xin=c["xin"], rev=rev)
        _same_bits(xl[:M, :N], c["want_ls"], f"{kern} LayerScale residual")
        _guards_ok(xl, M, N, f"{kern} LayerScale x")
        # fc1 (+ the pre-GELU copy on the 128 x 128 kernel)
        og = _sent(M + GUARD, N + 8, torch.bfloat16)
        o2 = _sent(M + GUARD, N + 8, torch.bfloat16) if kern == "small" else None
        eng.linear_ex(c["ag"], c["w"], c["bias"], "gelu", out=og, out2=o2, **kw)
        _same_bits(og[:M, :N], want_g, f"{kern} fc1 out")
        _guards_ok(og, M, N, f"{kern} fc1 out")
        if o2 is not None:
            _same_bits(o2[:M, :N], c["pre_g"], "small fc1 out2 (pre-GELU copy)")
            _guards_ok(o2, M, N, "small fc1 out2")
            og_plain = _sent(M + GUARD, N + 8, torch.bfloat16)
            eng.linear_ex(c["ag"], c["w"], c["bias"], "gelu", out=og_plain, **kw)
            assert torch.equal(og_plain, og), "fc1 with and without the pre-GELU copy differ"
        assert torch.equal(c["xin"], xin0), "xin was written"
        res[kern] = (out, x, xp, xl, og)
    for s, b in zip(res["small"], res["big"]):
        assert torch.equal(s, b), "the two kernels' buffers differ"
    if M >= 128 and K <= 256:                                    # the fc1 cases sit where GELU bends: neither all identity nor all zero
        pg = c["pre_g"].float().abs()
        assert float(((pg > 0.05) & (pg < 3)).float().mean()) > 0.2


# ------------------------------------------------------------------------------------------------------------------ score slab
def _layout(M: int, tokens: int, group: int, n_img: int):
    """Per row: counted?, image index (global), and per row the image index of its 128-row entry's first row — the kernels' rule."""
    m = torch.arange(M)
    if group > 0 and group < n_img:
        mpad = -(-group * tokens // 128) * 128
        sbk = m // mpad
        ml = m - sbk * mpad
        img_in = ml // tokens
        valid = img_in < torch.clamp(n_img - sbk * group, max=group)
        sample = sbk * group + img_in
        first = sbk * group + ((m // 128) * 128 - sbk * mpad) // tokens
    else:
        valid = torch.ones(M, dtype=torch.bool)
        sample = m // tokens
        first = ((m // 128) * 128) // tokens
    return valid, sample, first


def _slab_ref(sv: torch.Tensor, valid, sample, first, slab_ld: int):
    """float64 sums of squares per (128-row entry, segment) and the number of terms."""
    M = sv.shape[0]
    assert bool(((sample - first)[valid] <= 1).all()) and bool(((sample - first)[valid] >= 0).all())
    seg = (sample - first).clamp(0, 1)
    nt = 2 * ((M + 255) // 256)
    S = torch.zeros(nt, 2, slab_ld, dtype=torch.float64, device=sv.device)
    cnt = torch.zeros(nt, 2, dtype=torch.float64)
    v = sv[:, :slab_ld].double() ** 2
    tile = torch.arange(M) // 128
    for t in range(nt):
        for s in range(2):
            sel = valid & (tile == t) & (seg == s)
            cnt[t, s] = float(sel.sum())
            if sel.any():
                S[t, s] = v[sel.to(sv.device)].sum(0)
    return S, cnt.to(sv.device)


SLAB_LAYOUTS = [(128, 5, 0, 0), (130, 7, 0, 0), (197, 7, 0, 0), (257, 5, 0, 0), (577, 3, 0, 0), (197, 7, 3, 0), (130, 9, 4, 0), (257, 5, 2, 0),
                (197, 11, 4, 0), (197, 7, 3, 600)]                # (tokens, n_img, group, rows of M past the layout); 11 in 4s: a last group of 3


@pytest.mark.parametrize("tokens,n_img,group,extra", SLAB_LAYOUTS)
@pytest.mark.parametrize("site", [1, 2])
def test_score_slab_against_float64(eng, gelu_table, tokens, n_img, group, extra, site):
    from ssp2vit.engine import ssp2_rows
    rows = ssp2_rows(n_img, tokens, group)
    M, K = rows + extra, 128
    valid, sample, first = _layout(M, tokens, group, n_img)
    if group == 0:
        assert extra == 0 and bool(valid.all())
    pad = ~valid & (torch.arange(M) < rows)                      # the slab layout's pad rows
    assert bool(pad.any()) == (0 < group < n_img and (group * tokens) % 128 != 0)
    for N, slab_ld in ((192, 192), (320, 264)):
        g = torch.Generator().manual_seed(tokens * 31 + n_img * 7 + group + N)
        ka = torch.randint(-5, 6, (M, K), generator=g)
        key = torch.where(valid, sample, torch.full_like(sample, -1))
        nb = torch.full((1,), -2)
        edge = valid & ((key != torch.cat([nb, key[:-1]])) | (key != torch.cat([key[1:], nb])))   # each image's first and last row: the largest magnitudes
        assert int(edge.sum()) == 2 * n_img and int(valid.sum()) == n_img * tokens
        big = torch.randint(12, 16, (M, K), generator=g) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)
        ka = torch.where(edge[:, None], big, ka)
        ka = ka * (2 ** (sample % 3))[:, None]                   # image i scaled by 2^(i mod 3): |a| <= 15 / 8 * 4, products below 16
        kw = torch.randint(-15, 16, (N, K), generator=g)
        A, W, a, w = _buffers(ka, kw, scale=2.0 ** -6)           # A / 8 as in the fc1 cases (exact)
        A[:M][pad.cuda()] = NAN                                  # pad rows: the scores must not see them
        W[slab_ld:N] = NAN                                       # output columns the slab does not have
        bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).float()
        acc = (ka.cuda().double() @ kw.cuda().double().T) / 512.0
        pre = (acc + bias.cuda().double()[None, :]).float().to(torch.bfloat16)
        act = gelu_table[bf16_bits(pre)]
        sv = (pre if site == 1 else act).float()
        S, cnt = _slab_ref(sv, valid, sample, first, slab_ld)
        bound = (cnt[:, :, None] + 1) * U * S + cnt[:, :, None] * 2.0 ** -126
        ok = valid.cuda()
        slabs = {}
        for kern in KERNELS:
            out = _sent(M + GUARD, N + 8, torch.bfloat16)
            o2 = _sent(M + GUARD, N + 8, torch.bfloat16) if kern == "small" else None
            out, slab = eng.linear_ex(a, w, bias, "gelu", rows=M, kernel=kern, out=out, out2=o2, score_site=site, tokens=tokens,
                                      group=group, n_img=n_img, slab_ld=slab_ld)
            _same_bits(out[:M, :slab_ld][ok], act[:, :slab_ld][ok], f"{kern} fc1 out of the scoring epilogue")
            _guards_ok(out, M, N, f"{kern} fc1 out")
            if o2 is not None:
                _same_bits(o2[:M, :slab_ld][ok], pre[:, :slab_ld][ok], "small out2 of the scoring epilogue")
                _guards_ok(o2, M, N, "small out2")
            assert slab.shape == S.shape
            assert bool(torch.isfinite(slab).all()), f"{kern}: slab holds NaN: a pad row, a column past slab_ld or an unwritten entry"
            err = (slab.double() - S).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
            print(f"\n[slab {kern} site {site} tokens {tokens} n {n_img} group {group} M {M} N {N}] worst error / bound {ratio:.3f}")
            assert bool((slab[cnt == 0] == 0).all()), f"{kern}: a segment without rows is not 0"
            assert bool((err <= bound).all()), f"{kern}: slab error / bound {ratio:.3g} (site {site}, tokens {tokens}, group {group}, N {N})"
            slabs[kern] = slab
        assert torch.equal(slabs["small"], slabs["big"]), "the two kernels' slabs differ"


# --------------------------------------------------------------------------------------------------------------- split launch
@pytest.mark.parametrize("kern", KERNELS)
def test_split_fc1_launch_equals_the_whole_launch(eng, kern):
    """The kernel side of the forward's fused stage-1 + search launch: the hooked slabs [0, M0) with the scoring epilogue, the rest
    [M0, M) without it, A and out moved by M0 rows."""
    from ssp2vit.engine import ssp2_rows
    tokens, group, n_img, n_pref = 197, 4, 12, 8
    M = ssp2_rows(n_img, tokens, group)
    mpad = -(-group * tokens // 128) * 128
    M0 = (n_pref // group) * mpad
    N, K = 320, 128
    g = torch.Generator().manual_seed(11)
    A, W, a, w = _buffers(torch.randint(-15, 16, (M, K), generator=g), torch.randint(-15, 16, (N, K), generator=g), scale=2.0 ** -6)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).float()
    kw = dict(kernel=kern, score_site=1, tokens=tokens, group=group, slab_ld=N)
    plain = _sent(M + GUARD, N + 8, torch.bfloat16)
    eng.linear_ex(a, w, bias, "gelu", rows=M, kernel=kern, out=plain)
    full = _sent(M + GUARD, N + 8, torch.bfloat16)
    _, slab_full = eng.linear_ex(a, w, bias, "gelu", rows=M, out=full, n_img=n_img, **kw)
    out = _sent(M + GUARD, N + 8, torch.bfloat16)
    _, slab0 = eng.linear_ex(a, w, bias, "gelu", rows=M0, out=out, n_img=n_pref, **kw)
    assert bool((out[M0:] == SENT).all())
    eng.linear_ex(a[M0:], w, bias, "gelu", rows=M - M0, kernel=kern, out=out[M0:])
    assert bool(torch.isfinite(plain[:M, :N].float()).all())
    assert torch.equal(out, plain), "split launch differs from the whole launch"
    assert torch.equal(full, plain), "the scoring epilogue's output differs from the plain epilogue's"
    t0 = M0 // 128
    assert bool(torch.isfinite(slab0).all()) and torch.equal(slab0[:t0], slab_full[:t0]), "slab of the scored prefix differs"


# ------------------------------------------------------------------------------------------------------- realistic operands
@pytest.mark.parametrize("M,N,K,kernels", [(255, 192, 256, KERNELS), (4099, 320, 768, KERNELS), (257, 1152, 1152, KERNELS),
                                           (12608, 768, 3072, ("big",))])
def test_realistic_operands_against_float64(eng, M, N, K, kernels):
    g = torch.Generator().manual_seed(M + K)
    av = torch.randn(M, K, generator=g)
    av[:, [5, K // 3, K - 2]] *= 100.0                           # outlier channels
    A = torch.full((M + GUARD, K + 8), NAN, dtype=torch.bfloat16, device="cuda")
    A[:M, :K] = av.to(torch.bfloat16).cuda()
    wv = torch.randn(N, K, generator=g) * (0.02 + 0.03 * torch.rand(N, 1, generator=g))
    wv[::17] *= 8.0                                              # outlier rows
    W = torch.zeros((N + 255) // 256 * 256, K + 8, dtype=torch.bfloat16, device="cuda")
    W[:N, K:] = NAN
    W[:N, :K] = wv.to(torch.bfloat16).cuda()
    a, w = A[:, :K], W[:N, :K]
    bias = (torch.randn(N, generator=g) * 0.02).to(torch.bfloat16).float()
    xin = _sent(M + GUARD, N + 4, torch.float32)
    xin[:M, :N] = (torch.randn(M, N, generator=g) * 2).cuda()
    wd, bd = w.double(), bias.cuda().double()[None, :]
    outs = {}
    for kern in kernels:
        out = _sent(M + GUARD, N + 8, torch.bfloat16)
        eng.linear_ex(a, w, bias, "bf16", rows=M, kernel=kern, out=out)
        x = _sent(M + GUARD, N + 4, torch.float32)
        x[:M, :N] = NAN
        eng.linear_ex(a, w, bias, "resid", rows=M, kernel=kern, x=x, xin=xin)
        _guards_ok(out, M, N, f"{kern} out")
        _guards_ok(x, M, N, f"{kern} x")
        outs[kern] = (out, x)
    if len(kernels) == 2:
        assert torch.equal(outs["small"][0], outs["big"][0]) and torch.equal(outs["small"][1], outs["big"][1]), "the two kernels differ"
    out, x = outs[kernels[-1]]
    worst_b = worst_r = worst_old = 0.0
    for r0 in range(0, M, 2048):
        r1 = min(M, r0 + 2048)
        ad = a[r0:r1].double()
        S = ad.abs() @ wd.abs().T
        y = ad @ wd.T + bd
        e_acc = (K + 1) * U * S
        c = e_acc + U * (y.abs() + e_acc)
        bb = 2.0 ** -8 * (y.abs() + c) + c
        eb = (out[r0:r1, :N].double() - y).abs()
        xi = xin[r0:r1, :N].double()
        er = (x[r0:r1, :N].double() - (xi + y)).abs()
        assert bool(torch.isfinite(eb).all()) and bool(torch.isfinite(er).all()), "non-finite output: a gap column or a row past M was read"
        worst_b = max(worst_b, float((eb / bb.clamp_min(1e-300)).max()))
        worst_r = max(worst_r, float((er / (bb + U * (xi + y).abs()).clamp_min(1e-300)).max()))
        worst_old = max(worst_old, float((eb / (2.0 ** -8 * y.abs() + 2e-6 * (S + bd.abs()) + 1e-30)).max()))
    print(f"\n[realistic M={M} N={N} K={K}] worst error / bound: bf16 {worst_b:.3f}, resid {worst_r:.3f} (old: {worst_old:.3f})")
    assert worst_b <= 1.0 and worst_r <= 1.0
