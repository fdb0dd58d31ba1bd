"""The attention kernels (csrc/attn.hip.h) and the LayerNorm kernel (csrc/misc.hip.h, csrc/common.hip.h ln_row_*) on their own
buffers (ssp2_attention_bf16 / ssp2_layernorm: the very launches of the forward) against plain float64 statements of the same
operations, on inputs built so that a wrong kernel errs by far more than a correct one can.

Every input is exactly representable in the kernel's own input type (bf16 q / k / v; fp32 x, gamma, beta), so the only
differences come from the kernel's internal rounding points.  The bounds below are derived from those points, element by
element and from the data; they were written down before the first GPU run.  u = 2^-24 (fp32 unit roundoff).

Attention (per query row: p = softmax(s) of the float64 scores s = q.k / sqrt(d_h), o = sum_j p_j v_j, S1 = sum_j p_j |v_j|):
  scores   fp32 MFMA dot products of d_h exact bf16 products: |s_raw err| <= (d_h + 2) u A, A = max_j sum_i |q_i k_ji|.
  exponent a_j = fma(s_j, c2, -max c2), c2 = fl(scale) fl(log2 e) (relative error <= 3u).  The rounding of -max c2 is common to
           the row and cancels in the normalisation; c2's error, the fma rounding and, on the split ninth tile of the d_h = 80
           kernel, the per-wave maxima and the rescale exp2((m_w - M) c2) add <= 17 u smax c2 (smax = max_j |s_raw_j|), so
           delta = c2 ((d_h + 2) u A + 17 u smax) in the log2 domain and each numerator e_j carries a relative error
           eta <= ln2 delta + 4u (v_exp_f32: <= 2 ulp).
  P        rounded to bf16 for P V: relative 2^-8 per key (numerator only; bf16 keeps 8 significant bits, unit roundoff 2^-8).
  sums     row sum in fp32, <= 8 NT + 2 sequential adds per lane plus the split merge: sigma = (8 NT + 20) u;
           P V accumulates 32 NT products (exact bf16 x bf16) in fp32: acc = (32 NT + 16) u of sum |p~_j v_j|.
  output   1 / sum and the product: 3u; one bf16 rounding: 2^-8 relative.
  => core = (e_num S1 + e_den |o|) / (1 - e_den) + 3u (|o| + S1),  e_num = eta + 2^-8 (1 + eta) + acc (1 + 2^-8),  e_den = eta + sigma
     |o_kernel - o| <= 2^-8 (|o| + core) + core + 1e-30.
  (A first statement, 2^-9 |o| + (2^-9 + 2 ds + 2^-20) S1, was wrong twice: the unit roundoff of bf16 is 2^-8, not 2^-9 — a value in
  [2^e, 2^(e+1)) rounds by up to 2^(e-8) — and the fp32 P V accumulation and row sum, (32 NT + 16) u, are 2^-15.8 at 288 keys,
  not below 2^-20.  A float32 emulation of the kernel's rounding points sat at up to 1.12 of that first bound.)
  e4m3 output (fp8 mode, e4m3(o * scale), saturating at +-448): against clamp(o, +-448 / scale), which is 1-Lipschitz:
     |o8 / scale - clamp(o)| <= core + 2^-4 (min(|o|, 448 / scale) + core) + 2^-10 / scale
  (e4m3: 3 mantissa bits, relative half-ulp 2^-4 for normals, absolute 2^-10 below 2^-6).  The saturation counter is 0 when
  every |o scale| + core scale < 448 and non-zero when some |o scale| > 448 + core scale.

LayerNorm (per row: mu, sigma^2 of the float64 row, r = 1 / sqrt(sigma^2 + eps), y = (x - mu) r gamma + beta), MAXV = ceil(D / 256):
  mean     sum over (pairs, quads, MAXV chunks, 6 wave-reduction levels) then * fl(1 / D):
           dmu = (MAXV + 8) u sum|x| / D + 2u |mu|.
  variance sum of fma(d, d, q), d = fl(x - mean): sum (x - mean)^2 = D (sigma^2 + dmu^2) exactly, so
           var = (sigma^2 + dmu^2)(1 + (4 MAXV + 10) u) + eps (1 + u):  rho_v = (dmu^2 + (4 MAXV + 10) u (sigma^2 + dmu^2) + u eps) / (sigma^2 + eps).
  rstd     v_rsq + one Newton step, <= 4u: rho_r = rho_v / 2 + rho_v^2 + 4u.
  z        fl(fl(x - mean) rstd): dz = r (dmu + |x - mu| (rho_r + 2.01 u)) (1 + rho_r + 3u).
  output   fma(z, gamma, beta) once rounded, then bf16:
           |y_kernel - y| <= 2^-8 |y| + (1 + 2^-8) (|gamma| dz + u (|y| + |gamma| dz)) + 1e-30.
  Rows whose mean is exact (all-zero rows, constant power-of-two rows) give x - mean = 0: the output is exactly bf16(beta).
  Large means: the bound is sharp where |mu| / sigma <= 1e4 — the rows (10, 1e-2), (100, 1e-2), (3e4, 3), (3e4, 30), (-2e3, 0.5)
  of BIG_MEAN (mu, sigma).  The row (3e4, 1e-2) constrains nothing: dmu ~ 2e-2 exceeds sigma there (fp32 x itself is spaced 2e-3
  apart at 3e4), so dz ~ 100 |gamma| while |z| <~ 3; it only checks that such a row gives finite output.
  e4m3 form (per-row scale, ascale = amax / 448 of the bf16 outputs): a dequantised element q ascale is within
     B + (2^-4 + 6u) (|y| + B) + 2^-10 ascale of y, the row's largest output lands on code +-448 exactly, and
     |ascale - max|y| / 448| <= max B / 448 + 3u ascale.

NaN guards: every row the kernels must not read (slab pad rows, guard rows behind the last image, the gap of a strided x, the
token rows a CLS gather skips, the q columns the CLS-only form takes from its compact buffer) holds NaN inside the allocation,
and every output element the kernels must not write holds a sentinel that is checked afterwards.
"""
import math

import numpy as np
import pytest
import torch

from conftest import load_tiny_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LN2 = math.log(2.0)
SENT = -77.0           # bf16 sentinel of unwritten output
SENT8 = 0x5A           # byte sentinel of unwritten e4m3 output
GUARD = 5              # NaN rows behind the last image


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from ssp2vit.engine import VitEngine
    w, _, _ = load_tiny_golden("timm")
    e = VitEngine(w, device="cuda:0", max_images=4)
    yield e
    e.close()


def _e4m3_table():
    t = np.zeros(256)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = m * 2.0 ** -9 if e == 0 else (float("nan") if (e == 15 and m == 7) else (1 + m / 8) * 2.0 ** (e - 7))
        t[b] = -v if s else v
    return torch.tensor(t, dtype=torch.float64)


E4M3 = _e4m3_table()


def _decode8(b):
    return E4M3.to(b.device)[b.long()]


def _bf(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------------------- attention
def _image_rows(n, tokens, group, dev):
    from ssp2vit.engine import ssp2_rows
    from ssp2vit._lib import SLAB_ALIGN
    if 0 < group < n:
        mpad = -(-group * tokens // SLAB_ALIGN) * SLAB_ALIGN
        start = [(i // group) * mpad + (i % group) * tokens for i in range(n)]
    else:
        start = [i * tokens for i in range(n)]
    idx = torch.tensor(start, device=dev)[:, None] + torch.arange(tokens, device=dev)[None, :]
    return idx, ssp2_rows(n, tokens, group)


PATTERNS = ("uniform", "random", "peak_first", "peak_last", "peak_tile", "two_max", "tie_last", "peak_neg")


def _attn_inputs(n, tokens, heads, d_h, g, patterns, v_big=0.0):
    """q, k, v float32 [n, heads, tokens, d_h], bf16-representable; image i takes patterns[i % len(patterns)].  Peak heights
    alternate by head (scaled score 40 on even heads, 6 on odd ones)."""
    NT = (tokens + 31) // 32
    sc = 1.0 / math.sqrt(d_h)
    q = torch.empty(n, heads, tokens, d_h)
    k = torch.empty(n, heads, tokens, d_h)
    for i in range(n):
        pat = patterns[i % len(patterns)]
        for h in range(heads):
            target = 40.0 if h % 2 == 0 else 6.0
            lam = target / (sc * d_h)                                     # q ~ r (|r|^2 = d_h), k_peak = lam r: scaled score ~ target
            r = torch.randint(0, 2, (d_h,), generator=g).float() * 2 - 1
            qq = r[None, :] + 0.05 * torch.randn(tokens, d_h, generator=g)
            kk = 0.3 * torch.randn(tokens, d_h, generator=g)
            if pat == "uniform":
                kk[:] = torch.randn(d_h, generator=g)[None, :]           # identical keys: every score equal
                qq = torch.randn(tokens, d_h, generator=g)
            elif pat == "random":
                qq = 1.2 * torch.randn(tokens, d_h, generator=g)
                kk = 1.2 * torch.randn(tokens, d_h, generator=g)
            elif pat == "peak_first":
                kk[0] = lam * r
            elif pat == "peak_last":
                kk[tokens - 1] = lam * r
            elif pat == "peak_tile":                                      # query t peaks on a key of tile t % NT
                dirs = torch.randint(0, 2, (NT, d_h), generator=g).float() * 2 - 1
                for t in range(NT):
                    j = min(32 * t + (7 * t + 3 + h) % 32, tokens - 1)
                    kk[j] = lam * dirs[t]
                qq = dirs[torch.arange(tokens) % NT] + 0.05 * torch.randn(tokens, d_h, generator=g)
            elif pat == "two_max":                                        # two equal maxima in different key tiles
                j1, j2 = min(3 + h, tokens - 1), min(32 * (NT - 1) - 1 + (tokens > 32) * 3, tokens - 1)
                j2 = j2 if j2 != j1 else max(0, j1 - 1)
                kk[j1] = lam * r
                kk[j2] = lam * r
            elif pat == "tie_last":                                       # the last valid key tied with the maximum
                kk[0] = lam * r
                kk[tokens - 1] = lam * r
            elif pat == "peak_neg":                                       # one maximum, large negative scores everywhere else
                t = (i + h) % NT
                j = min(32 * t + (5 * h + 3 * i) % 32, tokens - 1)
                kk = -lam * r[None, :] + 0.3 * torch.randn(tokens, d_h, generator=g)
                kk[j] = lam * r
            q[i, h] = qq
            k[i, h] = kk
    v = torch.randn(n, heads, tokens, d_h, generator=g)
    v[1::2, :, :, 3::16] *= 64.0                                          # outlier channels on odd images
    if v_big:
        v[:, :, :, :8] *= v_big
    return _bf(q), _bf(k), _bf(v)


def _attn_ref(q, k, v, d_h):
    """float64 reference and the derived element-wise bound of the bf16 output (module docstring)."""
    q, k, v = q.double(), k.double(), v.double()
    tokens = q.shape[2]
    NT = (tokens + 31) // 32
    scale = 1.0 / math.sqrt(d_h)
    raw = q @ k.transpose(-1, -2)
    p = torch.softmax(raw * scale, dim=-1)
    o = p @ v
    S1 = p @ v.abs()
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    smax = raw.abs().amax(-1, keepdim=True)
    c2 = scale / LN2
    delta = c2 * ((d_h + 2) * U * A + 17 * U * smax)
    eta = LN2 * delta + 4 * U
    sig = (8 * NT + 20) * U
    acc = (32 * NT + 16) * U
    e_num = eta + 2.0 ** -8 * (1 + eta) + acc * (1 + 2.0 ** -8)
    e_den = eta + sig
    core = (e_num * S1 + e_den * o.abs()) / (1 - e_den) + 3 * U * (o.abs() + S1)
    return o, core


def _pack_qkv(q, k, v, idx, rows, dev, ldq_extra=0):
    n, heads, tokens, d_h = q.shape
    dim = heads * d_h
    qkv = torch.full((rows + GUARD, 3 * dim), float("nan"), dtype=torch.bfloat16, device=dev)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(n * tokens, dim)
    qkv[idx.reshape(-1)] = torch.cat([flat(q), flat(k), flat(v)], dim=1).to(dev, torch.bfloat16)
    return qkv


def _to_rows(o):
    """[n, heads, tokens, d_h] -> [n * tokens, dim], image-major: the order of out[idx.reshape(-1)] for the image rows idx"""
    n, heads, tokens, d_h = o.shape
    return o.permute(0, 2, 1, 3).reshape(n * tokens, heads * d_h)


def _check_attn(eng, q, k, v, d_h, group, tag, persist=None, live=None, rev=0, ldo_pad=8, stats=None, patterns=PATTERNS):
    dev = torch.device("cuda:0")
    n, heads, tokens, _ = q.shape
    dim = heads * d_h
    idx, rows = _image_rows(n, tokens, group, dev)
    qkv = _pack_qkv(q, k, v, idx, rows, dev)
    out = torch.full((rows + GUARD, dim + ldo_pad), SENT, dtype=torch.bfloat16, device=dev)
    eng.attention(qkv, n, tokens, heads, d_h, group=group, out=out, persist=persist, live=live, rev=rev)
    torch.cuda.synchronize()
    o, core = _attn_ref(q.to(dev), k.to(dev), v.to(dev), d_h)
    bound = 2.0 ** -8 * (o.abs() + core) + core + 1e-30
    got = out[idx.reshape(-1), :dim].double()
    err = (got - _to_rows(o)).abs()
    ratio = err / _to_rows(bound)
    assert not torch.isnan(got).any(), f"{tag}: NaN in the output (a pad / guard row leaked)"
    written = torch.zeros(rows + GUARD, dim + ldo_pad, dtype=torch.bool, device=dev)
    written[idx.reshape(-1), :dim] = True
    assert bool((out[~written].float() == SENT).all()), f"{tag}: an element outside the image rows / columns was written"
    # per pattern (image i <-> patterns[i % len(patterns)], as _attn_inputs dealt them) worst ratio
    r_img = ratio.reshape(n, tokens, dim).amax(dim=(1, 2)).cpu()
    if stats is not None:
        for i in range(n):
            key = (tag, patterns[i % len(patterns)])
            stats[key] = max(stats.get(key, 0.0), float(r_img[i]))
    worst = float(ratio.max())
    if worst > 1.0:
        w = int(ratio.argmax())
        row, col = divmod(w, dim)
        pytest.fail(f"{tag}: attention error {float(err.view(-1)[w]):.3e} exceeds its bound {float(_to_rows(bound).view(-1)[w]):.3e} "
                    f"(ratio {worst:.2f}) at token-row {row} col {col}; per image {[round(float(x), 2) for x in r_img]}")
    return worst


def _forms(d_h, tokens):
    NT = (tokens + 31) // 32
    persistent = (d_h == 64 and 4 <= NT <= 7) or (d_h == 80 and tokens == 257)
    has_live = (d_h == 64 and NT == 7 and (tokens - 192 + 7) >> 3 == 1) or (d_h == 80 and tokens == 257)
    forms = [("one-item", False, None)]
    if persistent:
        forms.append(("persist", True, False))
        if has_live:
            forms.append(("persist+LIVE", True, True))
    return forms


ATTN_GEOMS = [(64, t) for t in (5, 17, 32, 33, 50, 64, 65, 97, 101, 128, 145, 170, 192, 193, 197, 200, 201, 224, 226, 257, 288)] + \
             [(80, 257), (80, 260), (80, 288), (16, 5), (16, 32)]


@pytest.mark.parametrize("d_h,tokens", ATTN_GEOMS)
def test_attention_vs_float64_every_geometry_and_form(eng, d_h, tokens):
    """Every supported (d_h, tokens) pair, each kernel form the engine has for it (one-item kernel; persistent; persistent with
    the compile-time LIVE padding), eight score patterns (one per image: uniform, random, peaked on the first / the last valid
    key / a key of every key tile, two equal maxima in different tiles, the last valid key tied with the maximum, one maximum
    among large negative scores), V with outlier channels and mixed signs; slab layout with NaN pad and guard rows and an
    output row stride past dim."""
    g = torch.Generator().manual_seed(1000 * d_h + tokens)
    heads = 3 if d_h != 16 else 2
    q, k, v = _attn_inputs(len(PATTERNS), tokens, heads, d_h, g, PATTERNS)
    stats = {}
    for name, persist, live in _forms(d_h, tokens):
        for group in (3, 0):
            _check_attn(eng, q, k, v, d_h, group, f"d_h={d_h} T={tokens} {name}", persist=persist, live=live,
                        rev=group == 0, ldo_pad=8 if group else 0, stats=stats)
    for (tag, pat), r in sorted(stats.items()):
        print(f"[attn-vs-f64] {tag:<28} {pat:<10} max err/bound {r:.3f}")


@pytest.mark.parametrize("d_h,tokens,heads,live", [(64, 197, 4, True), (64, 197, 4, False), (64, 145, 4, None), (80, 257, 16, True),
                                                   (80, 257, 16, False)])
def test_attention_vs_float64_item_counts_and_walk_directions(eng, d_h, tokens, heads, live):
    """Persistent kernels with fewer items than CUs, exactly as many, and a count that is not a multiple of the CU count, walked
    both ways; for d_h = 80 at 257 tokens the split ninth query's maximum sits in each of the eight waves' key ranges (the
    peak_neg pattern moves it over the nine key tiles with the image and head)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator().manual_seed(77 + d_h + tokens)
    stats = {}
    for items in (min(40, n_cu // 2), n_cu, n_cu + heads * 3 + (heads if (n_cu + 3 * heads) % n_cu == 0 else 0)):
        n = -(-items // heads)
        pats = ("peak_neg",) * 9 + PATTERNS if d_h == 80 else PATTERNS
        q, k, v = _attn_inputs(n, tokens, heads, d_h, g, pats)
        for rev in (0, 1):
            _check_attn(eng, q, k, v, d_h, 4 if n > 4 else 0, f"d_h={d_h} T={tokens} items={n * heads} rev={rev} live={live}",
                        persist=True, live=live, rev=rev, stats=stats, patterns=pats)
    worst = {}
    for (_, pat), r in stats.items():
        worst[pat] = max(worst.get(pat, 0.0), r)
    print(f"[attn-items] d_h={d_h} T={tokens} live={live}: max err/bound " + ", ".join(f"{p} {r:.3f}" for p, r in sorted(worst.items())))


@pytest.mark.parametrize("d_h,tokens", [(64, 197), (64, 50), (64, 257), (80, 257), (80, 288), (16, 5)])
def test_cls_only_attention_vs_float64(eng, d_h, tokens):
    """The CLS-only form of the evaluation tail: q from a compact [n, dim] buffer (the qkv buffer's q columns are NaN), the
    compact [n, ldo] output; rows past n keep their sentinel."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5 + tokens)
    heads = 3
    n = len(PATTERNS)
    q, k, v = _attn_inputs(n, tokens, heads, d_h, g, PATTERNS)
    dim = heads * d_h
    for group in (3, 0):
        idx, rows = _image_rows(n, tokens, group, dev)
        qkv = _pack_qkv(q, k, v, idx, rows, dev)
        qkv[:, :dim] = float("nan")
        q_cls = q[:, :, 0, :].reshape(n, dim).to(dev, torch.bfloat16).contiguous()
        out = torch.full((n + GUARD, dim + 8), SENT, dtype=torch.bfloat16, device=dev)
        eng.attention(qkv, n, tokens, heads, d_h, group=group, out=out, q_cls=q_cls)
        torch.cuda.synchronize()
        o, core = _attn_ref(q.to(dev), k.to(dev), v.to(dev), d_h)
        o0, c0 = o[:, :, 0, :].reshape(n, dim), core[:, :, 0, :].reshape(n, dim)
        bound = 2.0 ** -8 * (o0.abs() + c0) + c0 + 1e-30
        got = out[:n, :dim].double()
        assert not torch.isnan(got).any()
        ratio = (got - o0).abs() / bound
        print(f"[attn-cls] d_h={d_h} T={tokens} group={group}: max err/bound {float(ratio.max()):.3f}")
        assert float(ratio.max()) <= 1.0, (d_h, tokens, group, float(ratio.max()))
        assert bool((out[:n, dim:].float() == SENT).all()) and bool((out[n:].float() == SENT).all())


@pytest.mark.parametrize("d_h,tokens,live", [(64, 197, True), (64, 197, False), (64, 101, None), (64, 224, None), (80, 257, True),
                                             (80, 257, False)])
def test_attention_e4m3_output_and_saturation_count(eng, d_h, tokens, live):
    """fp8 mode's attention output e4m3(o * 16) (persistent kernels) against clamp(o, +-28) within the derived bound; with
    moderate V (max |o * 16| ~ 24) and with V scaled so that the largest |o * 16| sits at 400..440 — on the top exponent's codes,
    below 448 by more than the bound — the saturation counter stays 0; with V x 40 in eight channels (|o * 16| well past 448)
    it counts, and the clipped elements sit on the +-448 code."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(31 + d_h + tokens)
    heads = 4 if d_h == 64 else 16
    n = 9 if d_h == 80 else len(PATTERNS)
    scale = 16.0
    pats = ("peak_neg",) * 9 if d_h == 80 else PATTERNS
    for case in ("moderate", "near448", "saturating"):
        v_big = 40.0 if case == "saturating" else 0.0
        q, k, v = _attn_inputs(n, tokens, heads, d_h, g, pats, v_big=v_big)
        if not v_big:
            v = _bf(v.clamp(-1.5, 1.5))                                    # moderate: |o * 16| < 448 with a margin
        if case == "near448":                                              # the largest |o * 16| to ~420 (V stays bf16-representable)
            o0, _ = _attn_ref(q.to(dev), k.to(dev), v.to(dev), d_h)
            v = _bf(v * (420.0 / (scale * float(o0.abs().max()))))
        dim = heads * d_h
        idx, rows = _image_rows(n, tokens, 4, dev)
        qkv = _pack_qkv(q, k, v, idx, rows, dev)
        out8 = torch.full((rows + GUARD, dim + 16), SENT8, dtype=torch.uint8, device=dev)
        sat = torch.zeros(4, dtype=torch.int32, device=dev)
        eng.attention(qkv, n, tokens, heads, d_h, group=4, out8=out8, out8_scale=scale, sat=sat[1:2], persist=True, live=live)
        torch.cuda.synchronize()
        o, core = _attn_ref(q.to(dev), k.to(dev), v.to(dev), d_h)
        o, core = _to_rows(o), _to_rows(core)
        lim = 448.0 / scale
        got = _decode8(out8[idx.reshape(-1), :dim]) / scale
        bound = core + 2.0 ** -4 * (o.abs().clamp(max=lim) + core) + 2.0 ** -10 / scale
        ratio = (got - o.clamp(-lim, lim)).abs() / bound
        assert not torch.isnan(got).any()
        written = torch.zeros(rows + GUARD, dim + 16, dtype=torch.bool, device=dev)
        written[idx.reshape(-1), :dim] = True
        assert bool((out8[~written] == SENT8).all()), "e4m3 output written outside the image rows / columns"
        assert int(sat[0]) == 0 and int(sat[2]) == 0 and int(sat[3]) == 0, "the counter's neighbours were written"
        count = int(sat[1])
        print(f"[attn-e4m3] d_h={d_h} T={tokens} live={live} {case}: max err/bound {float(ratio.max()):.3f}, "
              f"saturated waves {count}, max |o*16| {float(o.abs().max()) * scale:.0f}")
        assert float(ratio.max()) <= 1.0, (d_h, tokens, live, case, float(ratio.max()))
        if not v_big:
            assert float((o.abs() + core).max()) * scale < 448.0
            if case == "near448":
                assert float(o.abs().max()) * scale > 400.0
            assert count == 0, (case, count)
        else:
            clear = o.abs() * scale > 448.0 + core * scale
            assert bool(clear.any())
            assert count > 0
            assert bool((got[clear].abs() == lim).all()) and bool((got[clear].sign() == o[clear].sign()).all())


def test_wrappers_refuse_layouts_the_kernels_do_not_read(eng):
    """The kernels read qkv at a row stride of 3 * dim, the compact CLS queries at dim and a gathered x at D: a padded or
    strided buffer of any of them is refused instead of being read at the wrong stride."""
    dev = torch.device("cuda:0")
    n, tokens, heads, d_h = 2, 50, 2, 64
    dim = heads * d_h
    qkv = torch.zeros(n * tokens, 3 * dim, dtype=torch.bfloat16, device=dev)
    wide = torch.zeros(n * tokens, 3 * dim + 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError):
        eng.attention(wide, n, tokens, heads, d_h)                                  # extra columns
    with pytest.raises(ValueError):
        eng.attention(wide[:, :3 * dim], n, tokens, heads, d_h)                     # padded row stride
    q_wide = torch.zeros(n, dim + 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError):
        eng.attention(qkv, n, tokens, heads, d_h, q_cls=q_wide[:, :dim])
    with pytest.raises(ValueError):
        eng.attention(qkv, n, tokens, heads, d_h, q_cls=q_wide)
    D = 256
    g1, b1 = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    with pytest.raises(ValueError):
        eng.layernorm(torch.zeros(n * tokens, D + 4, device=dev), g1, b1, 1e-6, rows=n, gather=(tokens, 0))
    with pytest.raises(ValueError):
        eng.layernorm(torch.zeros(n * tokens * D, device=dev), g1, b1, 1e-6, rows=n, gather=(tokens, 0))
    out = eng.attention(qkv, n, tokens, heads, d_h)                                 # the accepted layout runs
    torch.cuda.synchronize()
    assert out.shape == (n * tokens, dim) and bool((out == 0).all())


# ------------------------------------------------------------------------------------------------------------- LayerNorm
LN_KINDS = ("gaussian", "big_mean", "outliers", "sigma_eps", "zero", "const_pow2", "gaussian_mean1")
BIG_MEAN = ((10.0, 1e-2), (3e4, 30.0), (3e4, 3.0), (100.0, 1e-2), (3e4, 1e-2), (-2e3, 0.5))      # (mu, sigma); (3e4, 1e-2): finite output only (docstring)


def _ln_rows(rows, D, eps, g):
    x = torch.empty(rows, D)
    kinds = []
    for r in range(rows):
        kind = LN_KINDS[r % len(LN_KINDS)]
        kinds.append(kind)
        z = torch.randn(D, generator=g)
        if kind == "gaussian":
            x[r] = z * float(torch.empty(1).uniform_(0.1, 4.0, generator=g)) + float(torch.randn(1, generator=g))
        elif kind == "big_mean":
            mu, s = BIG_MEAN[(r // len(LN_KINDS)) % len(BIG_MEAN)]
            x[r] = mu + s * z
        elif kind == "outliers":
            x[r] = z
            ch = torch.randint(0, D, (3,), generator=g)
            x[r, ch] = torch.tensor([100.0, -400.0, 1000.0])
        elif kind == "sigma_eps":
            c = (0.5, 1.0, 2.0)[(r // len(LN_KINDS)) % 3]
            x[r] = math.sqrt(eps) * (3.0 + c * z)
        elif kind == "zero":
            x[r] = 0.0
        elif kind == "const_pow2":
            x[r] = (-1.0) ** r * 2.0 ** ((r // len(LN_KINDS)) % 21 - 10)
        else:
            x[r] = 1.0 + z
    return x, kinds


def _ln_gamma_beta(D, g):
    gamma = 1.0 + 0.3 * torch.randn(D, generator=g)
    gamma[torch.randint(0, D, (max(1, D // 20),), generator=g)] = 0.0
    gamma[torch.randint(0, D, (max(1, D // 50),), generator=g)] *= 40.0
    beta = _bf(0.5 * torch.randn(D, generator=g))                         # bf16-representable: exact-mean rows give exactly beta
    return gamma, beta


def _ln_ref(x, gamma, beta, eps):
    """float64 reference and the derived element-wise bound of the bf16 output (module docstring)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    D = x.shape[1]
    maxv = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5}.get(-(-D // 256), 8)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    y = (x - mu) * r * gamma + beta
    dmu = (maxv + 8) * U * x.abs().sum(1, keepdim=True) / D + 2 * U * mu.abs()
    rho_v = (dmu ** 2 + (4 * maxv + 10) * U * (var + dmu ** 2) + U * eps) / (var + eps)
    rho_r = rho_v / 2 + rho_v ** 2 + 4 * U
    dz = r * (dmu + (x - mu).abs() * (rho_r + 2.01 * U)) * (1 + rho_r + 3 * U)
    gd = gamma.abs() * dz
    bound = 2.0 ** -8 * y.abs() + (1 + 2.0 ** -8) * (gd + U * (y.abs() + gd)) + 1e-30
    return y, bound


def _ln_check(y_k, y, bound, beta, kinds, tag, fp8_ascale=None):
    """-> worst ratio per row kind; asserts the bound and the exact-beta rows"""
    dev = y.device
    if fp8_ascale is None:
        got = y_k.double()
        full_bound = bound
    else:
        got = _decode8(y_k) * fp8_ascale.double()[:, None]
        full_bound = bound + (2.0 ** -4 + 6 * U) * (y.abs() + bound) + 2.0 ** -10 * fp8_ascale.double()[:, None]
    assert not torch.isnan(got).any(), f"{tag}: NaN in the output (a skipped row / gap leaked)"
    ratio = (got - y).abs() / full_bound
    kind_t = torch.tensor([LN_KINDS.index(kd) for kd in kinds], device=dev)
    out = {}
    for ki, kd in enumerate(LN_KINDS):
        sel = kind_t == ki
        if bool(sel.any()):
            out[kd] = float(ratio[sel].max())
    worst = float(ratio.max())
    if worst > 1.0:
        w = int(ratio.argmax())
        row, col = divmod(w, y.shape[1])
        pytest.fail(f"{tag}: LayerNorm error {float((got - y).abs().view(-1)[w]):.3e} > bound {float(full_bound.view(-1)[w]):.3e} "
                    f"(ratio {worst:.2f}) at row {row} ({kinds[row]}) col {col}")
    exact = torch.tensor([kd in ("zero", "const_pow2") for kd in kinds], device=dev)
    if fp8_ascale is None and bool(exact.any()):
        want = beta.to(dev, torch.bfloat16)[None, :].expand(int(exact.sum()), -1)
        assert torch.equal(y_k[exact].view(torch.int16), want.view(torch.int16)), f"{tag}: an exact-mean row is not exactly beta"
    return out


def _ln_fp8_extra(y8, ascale, y, bound, tag):
    vals = _decode8(y8)
    amax = vals.abs().amax(1)
    nz = y.abs().amax(1) > 0
    assert bool((amax[nz] == 448.0).all()), f"{tag}: a row's largest output is not on the +-448 code"
    a_ref = y.abs().amax(1) / 448.0
    a_b = bound.amax(1) / 448.0 + 3 * U * ascale.double()
    assert bool(((ascale.double() - a_ref).abs() <= a_b).all()), f"{tag}: ascale off its bound"


LN_WIDTHS = (192, 256, 384, 512, 640, 768, 1000, 1024, 1100, 1280, 1600, 2048)


@pytest.mark.parametrize("D", LN_WIDTHS)
def test_layernorm_vs_float64_widths_rows_eps_and_forms(eng, D):
    """Every MAXV instantiation in both the FULL and the predicated form (D = 192 .. 2048), 1 / 3 / 4099 rows (4099 also with the
    reverse walk), eps 1e-6 and 1e-12, seven row kinds (Gaussian; |mean| up to 3e4 with sigma down to 1e-2; outlier channels;
    sigma ~ sqrt(eps); all-zero and constant power-of-two rows, which must give exactly beta; mean 1), gamma with zeros and
    outliers; bf16 output (strided, NaN in the gap and in guard rows, an output stride past D) and the e4m3 per-row-scaled form."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(D)
    gamma, beta = _ln_gamma_beta(D, g)
    gd, bd = gamma.to(dev), beta.to(dev)
    stats = {}
    for eps in (1e-6, 1e-12):
        xs, kinds = _ln_rows(4099, D, eps, g)
        for rows, rev in ((1, 0), (3, 0), (4099, 0), (4099, 1)):
            x = xs[:rows]
            stride = D + 8
            xbuf = torch.full((rows + GUARD, stride), float("nan"), device=dev)
            xbuf[:rows, :D] = x.to(dev)
            y, bound = _ln_ref(x.to(dev), gd, bd, eps)
            out = torch.full((rows + GUARD, D + 4), SENT, dtype=torch.bfloat16, device=dev)
            eng.layernorm(xbuf, gd, bd, eps, rows=rows, in_stride=stride, out=out, rev=rev)
            torch.cuda.synchronize()
            tag = f"D={D} rows={rows} eps={eps:g} rev={rev}"
            res = _ln_check(out[:rows, :D], y, bound, beta, kinds[:rows], tag + " bf16")
            assert bool((out[:rows, D:].float() == SENT).all()) and bool((out[rows:].float() == SENT).all()), tag
            for kd, r in res.items():
                stats[("bf16", eps, kd)] = max(stats.get(("bf16", eps, kd), 0.0), r)
            y8 = torch.full((rows + GUARD, D + 4), SENT8, dtype=torch.uint8, device=dev)
            asc = torch.full((rows + GUARD,), -1.0, device=dev)
            eng.layernorm(xbuf, gd, bd, eps, rows=rows, in_stride=stride, out=y8, ascale=asc, rev=rev)
            torch.cuda.synchronize()
            res = _ln_check(y8[:rows, :D], y, bound, beta, kinds[:rows], tag + " e4m3", fp8_ascale=asc[:rows])
            _ln_fp8_extra(y8[:rows, :D], asc[:rows], y, bound, tag + " e4m3")
            assert bool((y8[:rows, D:] == SENT8).all()) and bool((y8[rows:] == SENT8).all()) and bool((asc[rows:] == -1.0).all()), tag
            for kd, r in res.items():
                stats[("e4m3", eps, kd)] = max(stats.get(("e4m3", eps, kd), 0.0), r)
    for (form, eps, kd), r in sorted(stats.items()):
        print(f"[ln-vs-f64] D={D:<5} {form:<5} eps={eps:<6g} {kd:<15} max err/bound {r:.3f}")


@pytest.mark.parametrize("D,tokens,group", [(768, 197, 2), (768, 197, 0), (192, 5, 2), (1280, 257, 3), (1600, 50, 0)])
def test_layernorm_cls_gather_vs_float64(eng, D, tokens, group):
    """The CLS-row form of the classifier head / tail: the CLS row of every image of a token matrix (slab layout or contiguous),
    every other row of it NaN (pad rows of the slabs included)."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(D + tokens + group)
    gamma, beta = _ln_gamma_beta(D, g)
    gd, bd = gamma.to(dev), beta.to(dev)
    n = 7
    idx, rows = _image_rows(n, tokens, group, dev)
    for eps in (1e-6, 1e-12):
        x, kinds = _ln_rows(n, D, eps, g)
        xbuf = torch.full((rows + GUARD, D), float("nan"), device=dev)
        xbuf[idx[:, 0]] = x.to(dev)
        y, bound = _ln_ref(x.to(dev), gd, bd, eps)
        out = torch.full((n + GUARD, D + 4), SENT, dtype=torch.bfloat16, device=dev)
        eng.layernorm(xbuf, gd, bd, eps, rows=n, gather=(tokens, group), out=out)
        torch.cuda.synchronize()
        res = _ln_check(out[:n, :D], y, bound, beta, kinds, f"gather D={D} T={tokens} group={group} eps={eps:g}")
        assert bool((out[:n, D:].float() == SENT).all()) and bool((out[n:].float() == SENT).all())
        print(f"[ln-cls] D={D} T={tokens} group={group} eps={eps:g}: max err/bound {max(res.values()):.3f}")
