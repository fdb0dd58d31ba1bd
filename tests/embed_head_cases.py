"""TEST INFRASTRUCTURE — cases, operands and float64 statements for the two ends of the forward (never imported by the product path).

Shared by tests/test_embed_head_statements_cpu.py (which proves on the CPU that the exact cases are exact and that the statements agree
with the oracle's modules) and tests/test_embed_head_numerics_gpu.py (which holds ssp2_embed / ssp2_head / ssp2_tail* to them).

Ingress   x[row(i) + P + q, :] = fl32(pos[P + q] + float(bf16(fl32(acc + b)))),  acc = sum_k bf16(pixel[i, q, k]) * bf16(W[:, k]),
          k = c p^2 + ky p + kx; prefix rows x[row(i) + t, :] = fl32((cls, dist)[t] + pos[t]).
Egress    h = bf16(LayerNorm(x[row(i) + t])); logit = float(bf16(fl32(sum_k h_k * bf16(W[c, k]) + b[c]))); with the distillation head
          logit = 0.5 * float(bf16(fl32(a + b))) of the two heads' logits a (CLS row) and b (DIST row).
Top-1     lowest index of a NaN if the row has one, else lowest index of the maximum (`top1_rule`).

Exact operands make `acc` exact in fp32 in any order: pixels / weights k / 8 with |k| <= 15 (every product a multiple of 2^-6), the
head's A operand +-g from balanced-sign rows (`balanced_rows`) against weights k / 8 with |k| <= 3.  `terms_bound` returns, per case,
the largest row sum of |terms| in units of the products' granularity: below 2^24 every partial sum is an fp32 integer multiple of it.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

NAN, INF = float("nan"), float("inf")
U = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------------------- the case lists
# patch embedding: (patch, img, dim, prefix, n images, group of the slab run).  K-tiles 1 2 3 4 5 7 10 on the element-wise gather, 3 12 27
# 48 on the 16-byte one; M = n * patches below / at 128, just past it, in three and in four row tiles; every group leaves a short last
# slab.  The last geometry has ONE patch per image: the only way to M = 129 exactly (129 = 3 * 43 is no other square's multiple).
EMBED_CASES = [
    (4, 16, 64, 1, 8, 3),         # K  48, 1 K-tile,  M 128
    (6, 24, 192, 2, 5, 2),        # K 108, 2,         M  80
    (7, 28, 320, 1, 9, 2),        # K 147, 3,         M 144
    (9, 27, 768, 2, 15, 2),       # K 243, 4,         M 135 (odd side)
    (10, 40, 192, 2, 25, 3),      # K 300, 5,         M 400 (four row tiles)
    (12, 36, 64, 1, 29, 3),       # K 432, 7,         M 261 (three row tiles)
    (14, 42, 768, 2, 14, 3),      # K 588, 10,        M 126
    (8, 32, 320, 1, 8, 3),        # K 192, 3, vec,    M 128
    (16, 48, 192, 2, 43, 3),      # K 768, 12, vec,   M 387
    (24, 48, 64, 1, 33, 2),       # K 1728, 27, vec,  M 132
    (32, 64, 768, 1, 32, 3),      # K 3072, 48, vec,  M 128
    (16, 16, 64, 1, 129, 50),     # one patch per image: M 129, slabs of 50 + 50 + 29
]
ROUNDING_CASES = [(14, 42, 192, 1, 10, 3), (8, 32, 64, 2, 9, 2)]       # pixels on and beside the bf16 ties (element-wise / 16-byte gather)
REALISTIC_EMBED = [(14, 42, 320, 1, 15, 0), (16, 48, 768, 2, 15, 0), (4, 16, 192, 1, 40, 0)]

# classifier head on img 32 / patch 16 engines: (dim, classes, n images, group).  Every class count of the ragged scalar store, every
# width, every image count (rows per block of the top-1 kernels: 4; row tiles of the GEMM: 128), 1000 classes at 768, 21843 at 64.
HEAD_CASES = [
    (64, 1, 5, 2), (192, 10, 3, 2), (320, 63, 4, 3), (768, 64, 1, 0), (1280, 65, 129, 7), (64, 127, 128, 8), (192, 128, 127, 9),
    (320, 129, 260, 7), (768, 1000, 260, 8), (1280, 1001, 5, 3), (64, 21843, 4, 3),
]
DIST_CASES = [(64, 1, 3, 2), (192, 65, 129, 7), (320, 129, 4, 3), (768, 1000, 128, 8), (1280, 1001, 5, 2)]
SLOT_CASES = [(192, 129, 4, 3, 2), (320, 1000, 6, 2, 3)]               # (dim, classes, n per slot, slots, group of the slab run)
TOP1_C = 1000                                                         # the scenarios below sit at classes c, c + 1, c + 37, c + 64, c + 640
GAMMAS = (1.0, 0.5, 1.75, -3.0)                                       # lnf gamma per column, bf16-representable (quarters)


def heads_of(dim: int) -> int:
    """Head dimension 64 at every width: the only one the engine builds attention kernels for at 2 .. 18 tokens (no test here runs them)."""
    return dim // 64


# ------------------------------------------------------------------------------------------------------------------- flat dicts
def _grid(g: torch.Generator, shape, lim: int, scale: float) -> torch.Tensor:
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).float() * scale


def flat_vit(img: int, patch: int, dim: int, heads: int, classes: int, prefix: int = 1, dist_head: bool = False, inter: int = 64,
             eps: float = 1e-6, seed: int = 0) -> Dict:
    """The flat dictionary of a depth-1 ViT, every tensor present.  Matrices are k / 8 with |k| <= 15 (the head: |k| <= 3), biases
    k / 64 with |k| <= 127 (bf16-representable), cls / dist / pos arbitrary fp32, the final norm's gamma cycles over GAMMAS with beta 0.
    The block is NEUTRAL — proj and fc2 are zero — so that the tail, run with its attention skipped, hands the prefix rows on unchanged."""
    if dist_head and prefix != 2:
        raise ValueError("the distillation head reads the distillation token: prefix = 2")
    g = torch.Generator().manual_seed(1000 * seed + 7 * img + patch + dim + classes)
    tokens = (img // patch) ** 2 + prefix
    w: Dict = dict(img=img, patch=patch, dim=dim, heads=heads, depth=1, classes=classes, eps=eps)
    if prefix != 1:
        w["prefix_tokens"] = prefix
    w["patch_w"] = _grid(g, (dim, 3, patch, patch), 15, 0.125)
    w["patch_b"] = _grid(g, (dim,), 127, 2.0 ** -6)
    w["cls"] = torch.randn(1, 1, dim, generator=g)
    w["pos"] = torch.randn(1, tokens, dim, generator=g)
    w["ln1_g.0"] = torch.ones(dim); w["ln1_b.0"] = torch.zeros(dim)
    w["qkv_w.0"] = _grid(g, (3 * dim, dim), 3, 2.0 ** -6); w["qkv_b.0"] = torch.zeros(3 * dim)
    w["proj_w.0"] = torch.zeros(dim, dim); w["proj_b.0"] = torch.zeros(dim)
    w["ln2_g.0"] = torch.ones(dim); w["ln2_b.0"] = torch.zeros(dim)
    w["fc1_w.0"] = _grid(g, (inter, dim), 3, 2.0 ** -6); w["fc1_b.0"] = torch.zeros(inter)
    w["fc2_w.0"] = torch.zeros(dim, inter); w["fc2_b.0"] = torch.zeros(dim)
    w["lnf_g"] = torch.tensor(GAMMAS).repeat(dim // 4); w["lnf_b"] = torch.zeros(dim)
    w["head_w"] = _grid(g, (classes, dim), 3, 0.125)
    w["head_b"] = _grid(g, (classes,), 127, 2.0 ** -6)
    if prefix == 2:
        w["dist"] = torch.randn(1, 1, dim, generator=g)
    if dist_head:
        w["head_dist_w"] = _grid(g, (classes, dim), 3, 0.125)
        w["head_dist_b"] = _grid(g, (classes,), 127, 2.0 ** -6)
    return w


# ------------------------------------------------------------------------------------------------------------ patch embedding
def exact_pixels(n: int, img: int, seed: int) -> torch.Tensor:
    """k / 8, |k| <= 15."""
    return _grid(torch.Generator().manual_seed(seed), (n, 3, img, img), 15, 0.125)


def tie_pixels(n: int, img: int, seed: int) -> torch.Tensor:
    """fp32 pixels that are NOT bf16 values: +-(1 + (2m + 1) / 256), the exact ties between neighbouring bf16 values in [1, 2), and the
    fp32 neighbour below and above each tie, a third each.  Rounded (RNE) they are (128 + j) / 128: products with k / 8 keep a
    granularity of 2^-10."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, 3, img, img)
    m = torch.randint(0, 128, shape, generator=g)
    tie = (1.0 + (2 * m + 1).float() / 256.0)                       # exact in fp32
    bits = tie.view(torch.int32) + torch.randint(-1, 2, shape, generator=g).to(torch.int32)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return bits.view(torch.float32) * sign


def realistic_pixels(n: int, img: int, seed: int) -> torch.Tensor:
    """Normalised-image-like values with a few x 100 outliers."""
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(n, 3, img, img, generator=g) * 1.2
    px.view(-1)[torch.randint(0, px.numel(), (max(4, px.numel() // 997),), generator=g)] *= 100.0
    return px


def realistic_patch_weight(dim: int, patch: int, seed: int) -> torch.Tensor:
    """std 0.02 .. 0.05 per output row, every 17th row x 8."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(dim, 3, patch, patch, generator=g) * (0.02 + 0.03 * torch.rand(dim, 1, 1, 1, generator=g))
    w[::17] *= 8.0
    return w


def patch_rows(px: torch.Tensor, patch: int) -> torch.Tensor:
    """[n, 3, img, img] -> [n, patches, 3 p^2]: patch q = py * side + px, column k = c p^2 + ky p + kx (the flattened conv weight)."""
    n, c, img, _ = px.shape
    s = img // patch
    return px.view(n, c, s, patch, s, patch).permute(0, 2, 4, 1, 3, 5).reshape(n, s * s, c * patch * patch)


def embed_terms(px: torch.Tensor, w: Dict):
    """float64 operands of the statement: bf16-rounded patch rows [n, patches, K], bf16-rounded weight [dim, K], bf16 bias [dim]."""
    a = patch_rows(px.to(torch.bfloat16).double(), int(w["patch"]))
    wt = w["patch_w"].to(torch.bfloat16).double().reshape(int(w["dim"]), -1)
    return a, wt, w["patch_b"].to(torch.bfloat16).double()


def embed_y(px: torch.Tensor, w: Dict) -> torch.Tensor:
    """fp32 [n, patches, dim] holding bf16 values: float(bf16(fl32(acc + b))), acc in float64."""
    a, wt, b = embed_terms(px, w)
    return (a @ wt.T + b).float().to(torch.bfloat16).float()


def embed_statement(px: torch.Tensor, w: Dict) -> torch.Tensor:
    """fp32 [n, tokens, dim]: the residual stream after the embedding.  The sum is taken in float64 (exact for the exact cases), the
    two roundings and the position add are fp32 / bf16 operations of the CPU, which round as the statement says."""
    prefix = int(w.get("prefix_tokens", 1))
    y = embed_y(px, w)
    pos = w["pos"].float().view(-1, int(w["dim"]))
    pre = [(w["cls"].float().view(1, -1) + pos[0:1])]
    if prefix == 2:
        pre.append(w["dist"].float().view(1, -1) + pos[1:2])
    pre = torch.cat(pre).unsqueeze(0).expand(px.shape[0], -1, -1)
    return torch.cat([pre, pos[prefix:].unsqueeze(0) + y], dim=1)


def embed_bound(px: torch.Tensor, w: Dict):
    """(reference pos + y in float64, element-wise bound) of the realistic cases, patch rows only [n, patches, dim]:
    E_acc = (K + 1) u sum|a_k w_k|, c = E_acc + u (|y| + E_acc), |x - (pos + y)| <= 2^-8 (|y| + c) + c + u |pos + y|."""
    prefix = int(w.get("prefix_tokens", 1))
    a, wt, b = embed_terms(px, w)
    K = a.shape[-1]
    y = a @ wt.T + b
    e_acc = (K + 1) * U * (a.abs() @ wt.abs().T)
    c = e_acc + U * (y.abs() + e_acc)
    ref = w["pos"].double().view(-1, int(w["dim"]))[prefix:].unsqueeze(0) + y
    return ref, 2.0 ** -8 * (y.abs() + c) + c + U * ref.abs()


def embed_layout(n: int, tokens: int, group: int):
    """(rows of the layout, first row of every image, pad rows between slabs) — csrc/engine.hip make_rowmap / total_rows."""
    img = torch.arange(n)
    if group <= 0 or group >= n:
        return n * tokens, img * tokens, torch.zeros(0, dtype=torch.long)
    mpad = -(-group * tokens // 128) * 128
    first = (img // group) * mpad + (img % group) * tokens
    slabs = -(-n // group)
    pad = torch.cat([torch.arange(s * mpad + group * tokens, (s + 1) * mpad) for s in range(slabs - 1)]) if mpad > group * tokens \
        else torch.zeros(0, dtype=torch.long)
    return int(first[-1]) + tokens, first, pad


def terms_bound(ka: torch.Tensor, kw: torch.Tensor) -> int:
    """Largest row sum of |integer numerators of the products|: int64 [M, K] x [N, K]."""
    return int((ka.abs().to(torch.int64) @ kw.abs().to(torch.int64).T).max())


def embed_numerators(px: torch.Tensor, w: Dict):
    """Integer numerators of the bf16-rounded pixels (in 1 / 128) and of the weights (in 1 / 8) of an exact case: products in 2^-10."""
    a, wt, _ = embed_terms(px, w)
    ka, kw = a * 128.0, wt * 8.0
    assert bool((ka == ka.round()).all()) and bool((kw == kw.round()).all()), "operands off their grid"
    return ka.reshape(-1, ka.shape[-1]).to(torch.int64), kw.to(torch.int64)


# ------------------------------------------------------------------------------------------------------------- classifier head
def balanced_rows(n: int, dim: int, seed: int, a: float = 4.0) -> torch.Tensor:
    """fp32 [n, dim]: every row holds +a in dim / 2 columns and -a in the others (a random arrangement per row): mean 0, variance a^2,
    both exact in fp32 in any order, so LayerNorm with gamma g and beta 0 gives +-g (1 - eps / (2 a^2) ...) = +-g after the bf16 rounding."""
    g = torch.Generator().manual_seed(seed)
    s = torch.ones(n, dim)
    for i in range(n):
        s[i, torch.randperm(dim, generator=g)[: dim // 2]] = -1.0
    return s * a


def head_rows_x(rows: torch.Tensor, tokens: int, group: int, guard: int = 0) -> torch.Tensor:
    """fp32 [layout rows + guard, dim]: rows [n, P, dim] are the images' prefix rows; every other row of the buffer is NaN (never read)."""
    n, P, dim = rows.shape
    total, first, _ = embed_layout(n, tokens, group)
    x = torch.full((total + guard, dim), NAN)
    for t in range(P):
        x[first + t] = rows[:, t]
    return x


def head_operand(rows: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """float64 [n, dim]: the classifier's A operand of balanced rows, sign(row) * gamma (NaN rows stay NaN)."""
    s = torch.where(torch.isnan(rows), rows, torch.sign(rows))         # (torch.sign maps NaN to 0)
    return s.double() * gamma.double()[None, :]


def head_logits(h: torch.Tensor, head_w: torch.Tensor, head_b: torch.Tensor) -> torch.Tensor:
    """fp32 [n, C] = float(bf16(fl32(sum_k h_k W[c, k] + b[c]))) from a float64 A operand h.  +-inf weight entries are taken out of the
    float64 product and put back by rule (the sign pattern decides between +inf, -inf and NaN), so that the prediction does not lean
    on how a BLAS orders non-finite terms; a NaN row of h gives a NaN row."""
    wb = head_w.to(torch.bfloat16).double()
    fin = torch.isfinite(wb)
    acc = torch.nan_to_num(h, nan=0.0) @ torch.where(fin, wb, torch.zeros_like(wb)).T
    for c, k in (~fin).nonzero().tolist():
        acc[:, c] = acc[:, c] + h[:, k] * wb[c, k]                    # float64 inf arithmetic: inf + -inf = NaN
    acc[torch.isnan(h).any(1)] = NAN
    return (acc + head_b.to(torch.bfloat16).double()[None, :]).float().to(torch.bfloat16).float()


def dist_logits(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """0.5 * float(bf16(fl32(a + b))): an fp32 add of the CPU, then the bf16 rounding, then the exact halving."""
    return 0.5 * (a.float() + b.float()).to(torch.bfloat16).float()


def top1_rule(logits: torch.Tensor) -> torch.Tensor:
    """int64 [n]: lowest index of a NaN if the row has one, else lowest index of the maximum — written out, no argmax involved."""
    n, C = logits.shape
    idx = torch.arange(C).expand(n, C)
    nan = torch.isnan(logits)
    first_nan = torch.where(nan, idx, torch.full_like(idx, C)).min(1).values
    mx = torch.where(nan, torch.full_like(logits, -INF), logits).max(1, keepdim=True).values
    first_max = torch.where(logits == mx, idx, torch.full_like(idx, C)).min(1).values
    return torch.where(nan.any(1), first_nan, first_max)


def same_bits_or_nan(got: torch.Tensor, want: torch.Tensor):
    """Elements that differ: NaN where NaN is expected (whatever its sign and payload: the host's and the GPU's default NaNs differ),
    identical bits everywhere else."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return (gn != wn) | (~wn & (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)))


# top-1 scenarios at TOP1_C classes: name -> edit(head_w, head_b, n) on clones.  Tied classes get one duplicated weight row and a bias of
# 4096, far above every other logit (|logit| <= 3 * 3 / 8 * dim + 2 < 1500), so that their common value is the row's maximum.
def _tie(classes):
    def edit(hw, hb):
        for c in classes[1:]:
            hw[c] = hw[classes[0]]
        hb[list(classes)] = 4096.0
    return edit


def _all_equal(hw, hb):
    hw.zero_(); hb.zero_()


def _all_neg_inf(hw, hb):
    hw.zero_(); hb.fill_(-INF)


def _pos_inf_column(hw, hb):
    hb[321] = INF
    _tie((700, 701))(hw, hb)                                            # a finite tie above everything else but the +inf column


def _nan_above_and_below_inf(hw, hb):
    hb[130] = NAN; hb[321] = INF; hb[770] = NAN                         # lowest NaN index wins, wherever the maximum is


def _nan_behind_inf(hw, hb):
    hb[5] = INF; hb[900] = NAN; hb[964] = NAN                           # the maximum in an earlier lane and step than both NaNs (900, 964: one lane)


def _per_row_inf(hw, hb):
    hw[417, 3] = INF; hw[417, 10] = INF                                 # A[i, 3] and A[i, 10] are +-g: +inf, -inf or NaN, row by row
    hw[90, 3] = -INF                                                    # ... and a column that is -inf where the other is +inf or NaN


TOP1_SCENARIOS = {
    "other lanes of one step": _tie((131, 132, 168)),                  # c, c + 1, c + 37: steps 2, lanes 3, 4, 40
    "one lane at other steps": _tie((195, 259, 835)),                  # c, c + 64, c + 640: lane 3
    "both, lowest index in a late lane": _tie((190, 259, 323, 830, 961)),   # lane 62 holds the lowest index; lanes 3 and 1 the others
    "every logit equal": _all_equal,
    "every logit -inf": _all_neg_inf,
    "+inf column": _pos_inf_column,
    "NaN bias above and below +inf": _nan_above_and_below_inf,
    "NaN behind the maximum": _nan_behind_inf,
    "+inf weights, per-row signs": _per_row_inf,
}


def head_case_weights(dim: int, classes: int, prefix: int = 1, dist_head: bool = False, scenario: Optional[str] = None, seed: int = 0) -> Dict:
    """flat_vit on the head geometry (img 32, patch 16), its head — with a distillation head: both heads — edited by a TOP1_SCENARIOS
    entry (the sum of two tied, infinite or NaN logits is tied, infinite or NaN in the same classes)."""
    w = flat_vit(32, 16, dim, heads_of(dim), classes, prefix=prefix, dist_head=dist_head, seed=seed)
    if scenario is not None:
        for kw, kb in (("head_w", "head_b"), ("head_dist_w", "head_dist_b"))[: 2 if dist_head else 1]:
            hw, hb = w[kw].clone(), w[kb].clone()
            TOP1_SCENARIOS[scenario](hw, hb)
            w[kw], w[kb] = hw, hb
    return w


def dist_special(w: Dict) -> Dict:
    """The distillation head's chosen sums, on classes whose weight rows are zero in both heads (a and b are then the biases):
    class 0: 1 + 2^-8, a tie that goes DOWN to the even 1;  class 1 (if there): (1 + 2^-7) + 2^-8, a tie that goes UP to the even 1 + 2^-6;
    class 2: +inf + -inf = NaN;  class 3: 2^20 (1 + 2^-7) + (1 + 2^-7): the fp32 sum rounds before the bf16 rounding does."""
    w = dict(w)
    C = int(w["classes"])
    for k in ("head_w", "head_b", "head_dist_w", "head_dist_b"):
        w[k] = w[k].clone()
    pairs = [(1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8), (INF, -INF), (2.0 ** 20 * (1 + 2.0 ** -7), 1 + 2.0 ** -7)]
    for c, (a, b) in enumerate(pairs[:C]):
        w["head_w"][c] = 0; w["head_dist_w"][c] = 0
        w["head_b"][c] = a; w["head_dist_b"][c] = b
    return w


def dist_cancelling(w: Dict) -> Dict:
    """head_dist = -head: with equal CLS and DIST rows a = -b in every class, every mean is 0 and every class ties."""
    w = dict(w)
    w["head_dist_w"] = -w["head_w"]; w["head_dist_b"] = -w["head_b"]
    return w


def head_numerators(w: Dict, key: str = "head_w"):
    """Integer numerators of the head's exact operands: |A| = |gamma| in quarters, the finite weights in eighths: products in 2^-5."""
    ka = (w["lnf_g"].double() * 4.0)
    kw = torch.nan_to_num(w[key].to(torch.bfloat16).double(), nan=0.0, posinf=0.0, neginf=0.0) * 8.0
    assert bool((ka == ka.round()).all()) and bool((kw == kw.round()).all()), "operands off their grid"
    return ka.to(torch.int64)[None, :], kw.to(torch.int64)


def realistic_head_weight(classes: int, dim: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    wv = torch.randn(classes, dim, generator=g) * (0.02 + 0.03 * torch.rand(classes, 1, generator=g))
    wv[::17] *= 8.0
    return wv, (torch.randn(classes, generator=g) * 0.02).to(torch.bfloat16).float()


def labels_for(pred: torch.Tensor, classes: int, seed: int) -> torch.Tensor:
    """int64 labels that match `pred` in about half the rows; the others are another class or one of -1, C and 2^40, which never match."""
    g = torch.Generator().manual_seed(seed)
    n = pred.numel()
    other = torch.tensor([-1, classes, 2 ** 40])[torch.randint(0, 3, (n,), generator=g)]
    if classes > 1:
        shifted = (pred + 1 + torch.randint(0, classes - 1, (n,), generator=g)) % classes
        other = torch.where(torch.rand(n, generator=g) < 0.5, shifted, other)
    return torch.where(torch.rand(n, generator=g) < 0.5, pred, other).to(torch.int64)
