"""TEST INFRASTRUCTURE — cases, operands and restatements for the small kernels of csrc/misc.hip.h and the host code around them: the
score finish, the weight path (ingest, compaction, clone, re-quantisation) and the fp8 calibration.  Never imported by the product path.

Shared by tests/test_misc_kernel_statements_cpu.py (which proves the restatements on the CPU, against float64 and torch CPU, on the very
inputs the GPU tests use) and tests/test_misc_kernels_gpu.py (which holds the kernels to them).

Row layout (include/ssp2vit.h, ssp2_rows): images contiguous, or slabs of `group` images padded to a multiple of 128 rows.  `layout`
returns every image's first row; `row_owner` the image each row belongs to (-1: a pad row, or a row behind the last image).

Fused score finish.  The fc1 epilogue leaves slab[t][seg][j]: 128-row tile t, seg 0 = the rows of the image that owns the tile's FIRST
row, seg 1 = the rows of the image after it.  `finish_fused` states the finish from that definition and the owner map alone: image s
collects, tile by tile in row order, the entry whose image it is; norm = float32(sqrt(float64(sum))) (sqrtf is correctly rounded: the
build has no fast-math; rounding a float64 root to fp32 is innocuous: 53 >= 2 * 24 + 2); the group sum adds the norms in image order
in fp32; on the bf16 chain the norm and the group sum are rounded with torch's .to(torch.bfloat16).  `finish_fused_f64` is the same
in float64 with the two bf16 roundings only.

Stand-alone route (ssp2_act_l2_accum).  `act_l2_statement`: sum of squares of the first token half (ceil(tokens / 2) rows) plus that of
the second, the root, lane q of four adding images s0 + q, s0 + q + 4, ... in that order, the fold (p0 + p1) + (p2 + p3) — the
association csrc/misc.hip.h documents for score_colsum_halves_kernel.  Activations are integers |v| <= 8: exact in bf16, every sum of
squares exact in fp32 (577 * 64 < 2^24) in any order.

Weight ingest.  `rne_bits` is round-to-nearest-even on the integer bit pattern (NaN kept NaN); `special_values` builds fp32 operands
from bit patterns: ties with an even and an odd upper half, one fp32 ulp on either side of a tie, the largest finite fp32, subnormals,
zeros and infinities of both signs, NaNs.  `matrix_image` / `bias_image` place torch's own rounding in the zero-padded image.

Compaction.  `coded_ffn` gives FFN weights whose bf16 bit patterns encode their own (row, column): all finite, all distinct within a
tensor, so one misplaced element shows.  `pruned_images` slices them on the host.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

U = 2.0 ** -24
NAN = float("nan")


def ceil_to(v: int, m: int) -> int:
    return -(-v // m) * m


# ----------------------------------------------------------------------------------------------------------------- row layout
def layout(n: int, tokens: int, group: int) -> Tuple[int, List[int]]:
    """(rows of the token matrix, first row of every image) — ssp2_rows as the header defines it."""
    if group <= 0 or group >= n:
        return n * tokens, [s * tokens for s in range(n)]
    mpad = ceil_to(group * tokens, 128)
    first = [(s // group) * mpad + (s % group) * tokens for s in range(n)]
    return first[-1] + tokens, first


def row_owner(n: int, tokens: int, group: int) -> np.ndarray:
    """owner[r] for r < ceil256(rows): the image row r belongs to, -1 for none."""
    rows, first = layout(n, tokens, group)
    own = np.full(ceil_to(rows, 256), -1, dtype=np.int64)
    for s, r0 in enumerate(first):
        assert (own[r0:r0 + tokens] == -1).all()
        own[r0:r0 + tokens] = s
    return own


def slab_tiles(n: int, tokens: int, group: int) -> int:
    return 2 * (ceil_to(layout(n, tokens, group)[0], 256) // 256)


def sample_entries(n: int, tokens: int, group: int, wrong_segment: bool = False) -> List[List[Tuple[int, int]]]:
    """Per image: the (tile, segment) entries of the slab that hold its rows, in row order.  From the definition: a tile's segment 0
    belongs to the owner of the tile's first row, segment 1 to the next image.  `wrong_segment` plants the defect the tests must see:
    the image's LAST tile is read from the other segment."""
    assert tokens >= 128
    own = row_owner(n, tokens, group)
    _, first = layout(n, tokens, group)
    out = []
    for s, r0 in enumerate(first):
        ent = []
        for t in range(r0 // 128, (r0 + tokens - 1) // 128 + 1):
            head = int(own[128 * t])
            assert head in (s, s - 1), "a 128-row tile of >= 128-token images meets two images at the most"
            ent.append((t, 0 if head == s else 1))
        if wrong_segment:
            t, seg = ent[-1]
            ent[-1] = (t, 1 - seg)
        out.append(ent)
    return out


def group_of(n: int, group: int) -> int:
    return n if (group <= 0 or group > n) else group


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def sqrt_f32(t: torch.Tensor) -> torch.Tensor:
    """float32(sqrt(float64(t))) — the correctly rounded fp32 root."""
    return t.double().sqrt().float()


def finish_fused(slab: torch.Tensor, n: int, tokens: int, group: int, chain: int, wrong_segment: bool = False):
    """slab f32 [tiles, 2, ld] -> (out f32 [groups, ld], norms f32 [n, ld]) in the kernels' association (fp32, tile order, image order)."""
    ld = slab.shape[2]
    norms = torch.empty(n, ld, dtype=torch.float32)
    for s, ent in enumerate(sample_entries(n, tokens, group, wrong_segment)):
        acc = torch.zeros(ld, dtype=torch.float32)
        for t, seg in ent:
            acc = acc + slab[t, seg]
        nrm = sqrt_f32(acc)
        norms[s] = bf16_round(nrm) if chain else nrm
    grp = group_of(n, group)
    out = torch.empty(-(-n // grp), ld, dtype=torch.float32)
    for g in range(out.shape[0]):
        acc = torch.zeros(ld, dtype=torch.float32)
        for s in range(g * grp, min(n, (g + 1) * grp)):
            acc = acc + norms[s]
        out[g] = bf16_round(acc) if chain else acc
    return out, norms


def finish_fused_f64(slab: torch.Tensor, n: int, tokens: int, group: int, chain: int):
    """The same in float64 (the two bf16 roundings of the reference chain kept)."""
    s64 = slab.double()
    norms = torch.stack([sum(s64[t, seg] for t, seg in ent).sqrt() for ent in sample_entries(n, tokens, group)])
    if chain:
        norms = bf16_round(norms)
    grp = group_of(n, group)
    out = torch.stack([norms[g * grp:min(n, (g + 1) * grp)].sum(0) for g in range(-(-n // grp))])
    return (bf16_round(out) if chain else out), norms


def slab_from_activations(act: torch.Tensor, group: int) -> torch.Tensor:
    """act f64 [n, tokens, ld] -> the slab the fc1 epilogue would leave, float64, from the layout's definition: per 128-row tile the
    sum of squares of the rows of the first row's image (segment 0) and of the image after it (segment 1); pad rows count nowhere."""
    n, tokens, ld = act.shape
    own = row_owner(n, tokens, group)
    _, first = layout(n, tokens, group)
    rows = torch.zeros(own.shape[0], ld, dtype=torch.float64)
    for s, r0 in enumerate(first):
        rows[r0:r0 + tokens] = act[s]
    sq = rows * rows
    slab = torch.zeros(own.shape[0] // 128, 2, ld, dtype=torch.float64)
    for t in range(slab.shape[0]):
        o = own[128 * t:128 * t + 128]
        head = int(o[0])
        if head < 0:
            assert (o < 0).all(), "a tile that starts on a pad row holds pad rows only"
            continue
        slab[t, 0] = sq[128 * t:128 * t + 128][torch.from_numpy(o == head)].sum(0)
        slab[t, 1] = sq[128 * t:128 * t + 128][torch.from_numpy(o == head + 1)].sum(0)
        assert ((o == head) | (o == head + 1) | (o < 0)).all()
    return slab


# (tokens, n, group, ld): what each is for is said beside it
FUSED_CASES = [
    (128, 5, 0, 64),      # an image is exactly one tile: segment 1 is never used
    (129, 5, 0, 64),      # one row into the next tile
    (197, 6, 0, 320),     # contiguous ViT-B/16 geometry, a partial second 256-column block
    (197, 7, 3, 64),      # slabs with pad rows, n no multiple of the group: a short last slab
    (197, 4, 1, 64),      # one image per slab
    (257, 5, 2, 320),     # 257 tokens, slabs, wide
    (577, 3, 0, 64),      # an image over 5 to 6 tiles
    (577, 5, 2, 64),      # ... in slabs
    (197, 37, 18, 64),    # the 16-wide unrolled sum, its tail (2) and a one-image group
]


def exact_slab(n: int, tokens: int, group: int, ld: int, seed: int) -> torch.Tensor:
    """Every entry a distinct integer in [1, entries]: neighbouring segments and tiles differ, every per-image sum is exact in fp32."""
    tiles = slab_tiles(n, tokens, group)
    cnt = tiles * 2 * ld
    assert cnt * 4 < 100 * 1024 and 7 * cnt < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(cnt, generator=g) + 1).float().view(tiles, 2, ld)


def realistic_slab(n: int, tokens: int, group: int, ld: int, seed: int) -> torch.Tensor:
    """Positive partial sums over seven orders of magnitude."""
    tiles = slab_tiles(n, tokens, group)
    g = torch.Generator().manual_seed(seed)
    return torch.exp(torch.rand(tiles, 2, ld, generator=g, dtype=torch.float64) * 16.0 - 6.0).float()


def tiles_per_sample(n: int, tokens: int, group: int) -> int:
    return max(len(e) for e in sample_entries(n, tokens, group))


def bf16_ulps_apart(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 steps between two tensors of finite, non-negative bf16-representable values."""
    ia = a.float().to(torch.bfloat16).view(torch.int16).to(torch.int32)
    ib = b.float().to(torch.bfloat16).view(torch.int16).to(torch.int32)
    return (ia - ib).abs()


# ----------------------------------------------------------------------------------------------------------- stand-alone route
# (tokens, n, group, d, ld).  Token counts: every unroll tier of act_l2_norms_kernel (64, 32, 16 and 4 token rows per wave step) runs and
# runs zero times (1 token: the second half is empty); groups at n = 70: the 8-images-in-flight loop (a lane needs 29 images ahead of
# it), ragged last groups, one group of all; d / ld: the pad columns [d, ld) are scored like any other.
ACT_L2_CASES = [
    (1, 6, 4, 64, 64), (2, 6, 4, 64, 200), (7, 6, 4, 200, 200), (50, 6, 4, 200, 512), (129, 6, 4, 64, 512), (197, 6, 4, 200, 200),
    (257, 6, 4, 64, 64), (577, 6, 4, 200, 512),
    (7, 70, 1, 64, 64), (7, 70, 3, 200, 200), (7, 70, 29, 64, 512), (50, 70, 33, 200, 512), (7, 70, 64, 64, 200), (50, 70, 0, 200, 200),
]


def act_l2_input(tokens: int, n: int, ld: int, seed: int) -> torch.Tensor:
    """Integers |v| <= 8 in EVERY column, the pad columns [d, ld) too (fp32; exact in bf16)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n, tokens, ld), generator=g).float()


def act_l2_statement(act: torch.Tensor, group: int, chain: int):
    """act f32 [n, tokens, ld] of small integers -> out f32 [groups, ld] in the documented association."""
    n, tokens, ld = act.shape
    mid = (tokens + 1) >> 1
    sq = act.double() ** 2
    h0, h1 = sq[:, :mid].sum(1), sq[:, mid:].sum(1)
    assert float((h0 + h1).max()) < 2 ** 24
    nrm = sqrt_f32(h0.float() + h1.float())
    if chain:
        nrm = bf16_round(nrm)
    grp = group_of(n, group)
    out = torch.empty(-(-n // grp), ld, dtype=torch.float32)
    for g in range(out.shape[0]):
        s0, s1 = g * grp, min(n, (g + 1) * grp)
        p = []
        for q in range(4):
            acc = torch.zeros(ld, dtype=torch.float32)
            for s in range(s0 + q, s1, 4):
                acc = acc + nrm[s]
            p.append(acc)
        t = (p[0] + p[1]) + (p[2] + p[3])
        out[g] = bf16_round(t) if chain else t
    return out


def act_l2_f64(act: torch.Tensor, group: int) -> torch.Tensor:
    n = act.shape[0]
    nrm = (act.double() ** 2).sum(1).sqrt()
    grp = group_of(n, group)
    return torch.stack([nrm[g * grp:min(n, (g + 1) * grp)].sum(0) for g in range(-(-n // grp))])


# ------------------------------------------------------------------------------------------------------------------- ingest
def rne_bits(u: np.ndarray, truncate: bool = False) -> np.ndarray:
    """fp32 bit patterns (uint32) -> bf16 bit patterns (uint16), round to nearest, ties to even; a NaN stays a NaN (quiet bit set).
    `truncate` plants the defect the tests must see."""
    u = u.astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u >> 16) if truncate else ((u + 0x7fff + ((u >> 16) & 1)) >> 16)
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


SPECIAL_BITS = np.array([
    0x3f808000, 0x3f818000,            # exact ties: even upper half (rounds down), odd upper half (rounds up)
    0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,   # one fp32 ulp on either side of them
    0xbf808000, 0xbf818000, 0xbf807fff, 0xbf818001,   # ... negative
    0x7f7fffff, 0xff7fffff,            # the largest finite fp32: rounds to infinity
    0x7f7f7fff, 0x7f7f8000,            # just below the bf16 maximum's upper tie, and on it (rounds to infinity)
    0x00000001, 0x007fffff, 0x80000001, 0x00008000, 0x00018000, 0x00007fff,   # subnormals, their ties
    0x00000000, 0x80000000, 0x7f800000, 0xff800000,   # zeros and infinities
    0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xff812345,               # NaNs, quiet and signalling
], dtype=np.uint32)


def special_values(shape, seed: int) -> torch.Tensor:
    """fp32 tensor from bit patterns: a random finite upper half, the lower half drawn from {tie, tie - 1, tie + 1, 0, random}, and
    every entry of SPECIAL_BITS planted (spread over the tensor where it has room, in front where it has not)."""
    numel = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    exp = rng.integers(0x70, 0x90, numel).astype(np.uint32)              # biased exponents around 1: all finite
    hi = (rng.integers(0, 2, numel).astype(np.uint32) << 15) | (exp << 7) | rng.integers(0, 128, numel).astype(np.uint32)
    lows = np.array([0x8000, 0x7fff, 0x8001, 0x0000], dtype=np.uint32)
    pick = rng.integers(0, 5, numel)
    lo = np.where(pick < 4, lows[np.minimum(pick, 3)], rng.integers(0, 0x10000, numel).astype(np.uint32))
    u = ((hi << 16) | lo).astype(np.uint32)
    k = min(numel, SPECIAL_BITS.size)
    pos = rng.choice(numel, k, replace=False) if numel >= 4 * SPECIAL_BITS.size else np.arange(k)
    u[pos] = np.roll(SPECIAL_BITS, seed)[:k]
    return torch.from_numpy(u.view(np.int32).copy()).view(torch.float32).reshape(shape)


def f32_bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def matrix_image(src: torch.Tensor, rows_pad: int, ld: int, zero_pad: bool = True) -> torch.Tensor:
    """torch CPU's bf16 cast of src [rows, ...] (flattened to 2-D) in a zero [rows_pad, ld] image.  `zero_pad = False` plants the defect
    the tests must see (a pad element left at 1)."""
    m = src.reshape(src.shape[0], -1)
    img = torch.zeros(rows_pad, ld, dtype=torch.bfloat16)
    if not zero_pad:
        img[-1, -1] = 1.0
    img[:m.shape[0], :m.shape[1]] = m.to(torch.bfloat16)
    return img


def bias_image(src: torch.Tensor, rows_pad: int) -> torch.Tensor:
    img = torch.zeros(rows_pad, dtype=torch.float32)
    img[:src.numel()] = src.reshape(-1).to(torch.bfloat16).float()
    return img


def differs(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Element mask: NaN positions are compared as "is NaN", everything else by bits (so +0 and -0 differ)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[got.element_size()]
    if got.dtype == torch.uint8:
        return got != want
    gn, wn = got.isnan(), want.isnan()
    return (gn != wn) | (~gn & (got.contiguous().view(it) != want.contiguous().view(it)))


MATRIX_KINDS = ("patch_w", "qkv_w", "proj_w", "fc1_w", "fc2_w", "head_w", "head_dist_w")
BIAS_KINDS = ("patch_b", "qkv_b", "proj_b", "fc1_b", "fc2_b", "head_b", "head_dist_b")
LAYER_KINDS = ("ln1_g", "qkv_w", "qkv_b", "proj_w", "ln1_b", "ln2_g", "proj_b", "fc1_w", "fc1_b", "fc2_w", "ln2_b", "fc2_b")


def tensor_list(depth: int, dist: bool) -> List[Tuple[str, int]]:
    """(kind, layer) of every tensor of an engine, the kinds mixed: a bias or a vector sits between the matrices."""
    out = [("patch_w", 0), ("cls", 0), ("patch_b", 0), ("head_w", 0), ("pos", 0), ("head_b", 0), ("lnf_g", 0), ("lnf_b", 0)]
    if dist:
        out[3:3] = [("dist", 0), ("head_dist_w", 0), ("head_dist_b", 0)]
    for l in range(depth):
        out += [(k, l) for k in LAYER_KINDS]
    return out


def key_of(kind: str, layer: int) -> str:
    return kind if kind in ("patch_w", "patch_b", "cls", "pos", "lnf_g", "lnf_b", "head_w", "head_b", "dist", "head_dist_w", "head_dist_b") \
        else f"{kind}.{layer}"


def geometry(img=28, patch=14, dim=64, depth=2, classes=10, d_int=(203, 72), prefix=1, dist_head=False) -> Dict:
    return dict(img=img, patch=patch, dim=dim, heads=dim // 64, depth=depth, classes=classes, eps=1e-6, d_int=tuple(d_int),
                prefix=prefix, dist_head=dist_head, tokens=(img // patch) ** 2 + prefix)


def tensor_shapes(geo: Dict) -> Dict[str, tuple]:
    D, p = geo["dim"], geo["patch"]
    s = {"patch_w": (D, 3, p, p), "patch_b": (D,), "cls": (1, 1, D), "pos": (1, geo["tokens"], D), "lnf_g": (D,), "lnf_b": (D,),
         "head_w": (geo["classes"], D), "head_b": (geo["classes"],)}
    if geo["prefix"] == 2:
        s["dist"] = (1, 1, D)
    if geo["dist_head"]:
        s["head_dist_w"] = (geo["classes"], D); s["head_dist_b"] = (geo["classes"],)
    for l, di in enumerate(geo["d_int"]):
        s.update({f"ln1_g.{l}": (D,), f"ln1_b.{l}": (D,), f"qkv_w.{l}": (3 * D, D), f"qkv_b.{l}": (3 * D,), f"proj_w.{l}": (D, D),
                  f"proj_b.{l}": (D,), f"ln2_g.{l}": (D,), f"ln2_b.{l}": (D,), f"fc1_w.{l}": (di, D), f"fc1_b.{l}": (di,),
                  f"fc2_w.{l}": (D, di), f"fc2_b.{l}": (D,)})
    return s


def flat_weights(geo: Dict, fill) -> Dict:
    """The flat dictionary VitEngine takes, every tensor from fill(name, shape, index)."""
    w: Dict = {k: geo[k] for k in ("img", "patch", "dim", "heads", "depth", "classes", "eps")}
    if geo["prefix"] != 1:
        w["prefix_tokens"] = geo["prefix"]
    for i, (name, shape) in enumerate(tensor_shapes(geo).items()):
        w[name] = fill(name, shape, i)
    return w


def special_weights(geo: Dict, seed: int) -> Dict:
    return flat_weights(geo, lambda name, shape, i: special_values(shape, 1000 * seed + i))


def random_weights(geo: Dict, seed: int, std: float = 0.05) -> Dict:
    """Ordinary weights for the cases that run a forward: Gaussian matrices, small biases, LayerNorm near (1, 0)."""
    g = torch.Generator().manual_seed(seed)

    def fill(name, shape, i):
        base = name.split(".")[0]
        if base in ("ln1_g", "ln2_g", "lnf_g"):
            return 1.0 + 0.1 * torch.randn(shape, generator=g)
        if base.endswith("_w"):
            return std * torch.randn(shape, generator=g)
        if base in ("cls", "pos", "dist"):
            return 0.5 * torch.randn(shape, generator=g)
        return 0.02 * torch.randn(shape, generator=g)
    return flat_weights(geo, fill)


def expected_image(kind: str, src: torch.Tensor, shape: Dict[str, int]) -> torch.Tensor:
    """What the engine must hold for `src` loaded as `kind`, given the image's (rows_pad, ld)."""
    if kind in MATRIX_KINDS:
        return matrix_image(src, shape["rows_pad"], shape["ld"])
    if kind in BIAS_KINDS:
        return bias_image(src, shape["rows_pad"])
    return src.reshape(-1).clone()


def fresh_shape(kind: str, src: torch.Tensor) -> Dict[str, int]:
    """rows, cols, rows_pad, ld of a freshly created engine's storage for `src`: matrices [ceil256(rows), ceil64(cols)]."""
    if kind in MATRIX_KINDS:
        rows, cols = src.shape[0], src[0].numel()
        return dict(rows=rows, cols=cols, rows_pad=ceil_to(rows, 256), ld=ceil_to(cols, 64))
    if kind in BIAS_KINDS:
        return dict(rows=src.numel(), cols=1, rows_pad=ceil_to(src.numel(), 256), ld=1)
    return dict(rows=src.numel(), cols=1, rows_pad=src.numel(), ld=1)


# --------------------------------------------------------------------------------------------------------------- compaction
def _coded(rows: int, cols: int, base: int) -> torch.Tensor:
    """fp32 [rows, cols] whose bf16 pattern is base + row * cols + col: positive, finite, distinct."""
    bits = base + np.arange(rows * cols, dtype=np.int64)
    assert base > 0x0080 and int(bits[-1]) < 0x7f80
    return torch.from_numpy((bits.astype(np.uint32) << 16).view(np.int32).copy()).view(torch.float32).reshape(rows, cols)


def coded_ffn(geo: Dict, w: Dict, salt: int = 0) -> Dict:
    """`w` with every block's fc1 / fc2 weights and fc1 bias replaced by self-describing values (fc2's bias distinct too)."""
    w = dict(w)
    D = geo["dim"]
    for l, di in enumerate(geo["d_int"]):
        w[f"fc1_w.{l}"] = _coded(di, D, 0x1000 + 0x100 * l + salt)
        w[f"fc2_w.{l}"] = _coded(D, di, 0x4400 + 0x100 * l + salt)
        w[f"fc1_b.{l}"] = _coded(1, di, 0x3c00 + 0x100 * l + salt).reshape(di)
        w[f"fc2_b.{l}"] = _coded(1, D, 0x2e00 + 0x100 * l + salt).reshape(D)
    return w


def pruned_images(w: Dict, layer: int, keep, fc1_rows_pad: int, shift: int = 0) -> Dict[str, torch.Tensor]:
    """Host-sliced images of block `layer` after keeping neurons `keep`: fc1 rows (image [fc1_rows_pad, ceil64(dim)]), fc1 bias entries,
    fc2 columns at ld = ceil64(n_keep); pads zero; fc2's bias as it was.  `shift` plants the defect the tests must see (the keep list
    moved by one neuron)."""
    k = torch.as_tensor(list(keep), dtype=torch.long)
    if shift:
        k = (k + shift) % w[f"fc1_w.{layer}"].shape[0]
    fc1, b1, fc2, b2 = w[f"fc1_w.{layer}"], w[f"fc1_b.{layer}"], w[f"fc2_w.{layer}"], w[f"fc2_b.{layer}"]
    D = fc1.shape[1]
    return {"fc1_w": matrix_image(fc1[k], fc1_rows_pad, ceil_to(D, 64)), "fc1_b": bias_image(b1[k], fc1_rows_pad),
            "fc2_w": matrix_image(fc2[:, k], ceil_to(D, 256), ceil_to(len(k), 64)), "fc2_b": bias_image(b2, ceil_to(D, 256))}


def keep_lists(d_int: int, seed: int) -> Dict[str, List[int]]:
    """The keep lists of the compaction cases for a block of d_int > 65 neurons."""
    g = torch.Generator().manual_seed(seed)
    pick = lambda k: sorted(torch.randperm(d_int, generator=g)[:k].tolist())
    tail = sorted(set(pick(20)) | {d_int - 1})
    return {"all": list(range(d_int)), "one": [d_int // 3], "64": pick(64), "65": pick(65), "ends on the last": tail}
