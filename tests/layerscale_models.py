"""TEST INFRASTRUCTURE — CPU restatement of ViTs with LayerScale (never imported by the product path).

The oracle's modules (oracle/vit_modules.py) know no LayerScale.  timm's Block with ``init_values`` multiplies each residual branch by
a learned per-channel vector before the add::

    x = x + ls1(attn(norm1(x)));  x = x + ls2(mlp(norm2(x)));  LayerScale.forward(x) = x * gamma   (inplace=False)

Under CPU autocast the branch output is bf16 and gamma an fp32 parameter: ``x * gamma`` is one fp32 product, the residual add a
second fp32 operation.  ``LayerScaleTimmViT`` composes the oracle's timm-layout blocks with that module (an ``nn.Identity`` where a
branch has none), in the timm anatomy the reference duck-types over (``blocks[i].{norm1, attn, ls1, norm2, mlp, ls2}``), and is run
through ``oracle.ref_cpu`` like the oracle's own modules.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from oracle.vit_modules import TimmLayoutViT, load_flat_weights


class LayerScale(nn.Module):
    """timm.layers.LayerScale: ``x * gamma`` (``x.mul_(gamma)`` with inplace=True, which the loaders refuse)."""
    def __init__(self, dim: int, init_values: float = 1e-5, inplace: bool = False):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x.mul_(self.gamma) if self.inplace else x * self.gamma


def _ls_block_forward(self, x):
    x = x + self.ls1(self.attn(self.norm1(x)))
    return x + self.ls2(self.mlp(self.norm2(x)))


class LayerScaleTimmViT(TimmLayoutViT):
    """The oracle's timm-layout ViT whose blocks carry ``ls1`` / ``ls2`` (LayerScale where `layer_scale[i][branch]`, else Identity)."""
    def __init__(self, *, img, patch, dim, heads, inter, depth, classes, eps=1e-6, layer_scale=None):
        super().__init__(img=img, patch=patch, dim=dim, heads=heads, inter=inter, depth=depth, classes=classes, eps=eps)
        layer_scale = layer_scale if layer_scale is not None else [(True, True)] * depth
        for blk, (a, m) in zip(self.blocks, layer_scale):
            blk.ls1 = LayerScale(dim) if a else nn.Identity()
            blk.ls2 = LayerScale(dim) if m else nn.Identity()
            blk.forward = _ls_block_forward.__get__(blk)
        self.num_prefix_tokens = 1
        self.global_pool = "token"
        self.fc_norm = nn.Identity()
        self.no_embed_class = False
        self.reg_token = None

    def __deepcopy__(self, memo):           # the blocks' bound forwards must follow a copy to ITS blocks (copy mode of the depth search)
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        import copy
        for k, v in self.__dict__.items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        for blk in new.blocks:
            blk.forward = _ls_block_forward.__get__(blk)
        return new


def _cfg(w):
    return dict(img=int(w["img"]), patch=int(w["patch"]), dim=int(w["dim"]), heads=int(w["heads"]),
                inter=[int(w[f"fc1_w.{i}"].shape[0]) for i in range(int(w["depth"]))], depth=int(w["depth"]),
                classes=int(w["classes"]))


@torch.no_grad()
def build_layerscale(w) -> nn.Module:
    """A flat dictionary with ``ls1.i`` / ``ls2.i`` -> the eval-mode fp32 CPU module (timm anatomy)."""
    depth = int(w["depth"])
    has = [(f"ls1.{i}" in w, f"ls2.{i}" in w) for i in range(depth)]
    m = load_flat_weights(LayerScaleTimmViT(**_cfg(w), eps=float(w.get("eps", 1e-6)), layer_scale=has), w)
    for i, blk in enumerate(m.blocks):
        for name in ("ls1", "ls2"):
            if f"{name}.{i}" in w:
                getattr(blk, name).gamma.copy_(w[f"{name}.{i}"].reshape(-1))
    return m.eval()


# ------------------------------------------------------------------------------------------- golden cases (tests/golden/ls_*.npz)
# tag -> (VIT_CONFIGS name, batches, images per batch, prune count t per block, min_remaining, K blocks, weight scale, planner targets).
# tests/golden/make_golden_layerscale.py writes the reference's outputs for these inputs; the tests regenerate the inputs from the same
# seeds and check the stored checksums.
LS_GOLDEN_CASES = {
    "ls_test": ("vit_test_patch16_32_ls", 2, 8, 40, 16, 2, 0.1, (0.25, 0.375, 0.5)),
    "ls_s16": ("vit_small_patch16_224_ls_d2", 2, 16, 576, 512, 1, 0.03, (0.25, 0.375, 0.5)),
}


def _grid(shape, scale, g):
    """Values k * scale / 64, k uniform in [-127, 127], from an INTEGER generator: the same bits on every host."""
    return torch.randint(-127, 128, tuple(shape), generator=g).float() * (scale / 64.0)


def _gamma(dim, g):
    """LayerScale values from integer draws: (128 + m) / 128 * 2^e with m in [0, 127], e in [-10, 0] — magnitudes in [2^-10, 2), every one
    exactly representable — and every fourth draw negative."""
    m = torch.randint(0, 128, (dim,), generator=g).float()
    e = torch.randint(-10, 1, (dim,), generator=g).float()
    s = torch.randint(0, 4, (dim,), generator=g)
    mag = (128.0 + m) / 128.0 * torch.exp2(e)
    return torch.where(s == 0, -mag, mag)


def weak_neurons(tag: str, block: int) -> torch.Tensor:
    """The FFN neurons of a golden case whose fc1 row and bias are scaled by 1 / 4 (exact: a power of two): t of them per block, t the
    case's prune count (5 / 16 of 128, 3 / 8 of 1536), spread over the width and other ones in every block.  A neuron's pre-GELU
    activation, and so its stage-1 score, scales by exactly 1 / 4 with them: the cut at t falls into a gap far wider than any score
    tolerance, so the mask step's answer is decided (ssp2vit.mask_parity: `guaranteed`) and the masks can be asserted."""
    from ssp2vit.weights import VIT_CONFIGS
    d_int, t = VIT_CONFIGS[LS_GOLDEN_CASES[tag][0]][4], LS_GOLDEN_CASES[tag][3]
    num, den = (5, 16) if (d_int, t) == (128, 40) else (3, 8)
    j = torch.arange(d_int)
    weak = j[(j * 5 + block) % den < num]
    assert weak.numel() == t
    return weak


def golden_weights(tag: str):
    """The flat dictionary of a golden case: the shapes of synthetic_weights, every matrix, bias and embedding drawn by _grid (matrices at
    the case's std, biases at 0.02), LayerNorm gamma 1 / beta 0, LayerScale by _gamma; fc1 rows and biases of weak_neurons() x 1 / 4."""
    from ssp2vit.weights import synthetic_weights
    name, std = LS_GOLDEN_CASES[tag][0], LS_GOLDEN_CASES[tag][6]
    w = synthetic_weights(name, classes=10, seed=0, std=std, eps=1e-6)
    g = torch.Generator().manual_seed(0)
    for k, v in list(w.items()):
        if not isinstance(v, torch.Tensor) or k.startswith(("ln1_", "ln2_", "lnf_")):
            continue
        if k.startswith(("ls1.", "ls2.")):
            w[k] = _gamma(v.numel(), g)
        else:
            bias = k.endswith("_b") or "_b." in k
            w[k] = _grid(v.shape, 0.02 if bias else std, g)
    for l in range(int(w["depth"])):
        weak = weak_neurons(tag, l)
        w[f"fc1_w.{l}"][weak] *= 0.25
        w[f"fc1_b.{l}"][weak] *= 0.25
    return w


def golden_pixels(tag: str):
    name, nb, bs = LS_GOLDEN_CASES[tag][:3]
    from ssp2vit.weights import VIT_CONFIGS
    img = VIT_CONFIGS[name][0]
    g = torch.Generator().manual_seed(1)
    return [_grid((bs, 3, img, img), 64.0, g) / 64.0 for _ in range(nb)]


_GOLDEN = {}


def load_golden(tag: str):
    """-> (flat weights, batches with the stored labels, npz dict) of tests/golden/<tag>_timm.npz; computed once per process and shared
    (callers do not modify it); the regenerated inputs are checked against the stored checksums."""
    if tag in _GOLDEN:
        return _GOLDEN[tag]
    import os
    import numpy as np
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{tag}_timm.npz")))
    w = golden_weights(tag)
    pxs = golden_pixels(tag)
    assert float(z["weights_checksum"]) == sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor)), "weights changed"
    assert float(z["pixels_checksum"]) == sum(float(p.double().sum()) for p in pxs), "pixels changed"
    batches = [{"pixel_values": p, "labels": torch.from_numpy(z[f"labels.{i}"])} for i, p in enumerate(pxs)]
    _GOLDEN[tag] = (w, batches, z)
    return _GOLDEN[tag]


def bf16_from_bits(a) -> torch.Tensor:
    import numpy as np
    return torch.from_numpy(np.asarray(a).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
