"""TEST INFRASTRUCTURE — CPU restatement of ViTs with register tokens and class-free positions (never imported by the product path).

timm's ``VisionTransformer._pos_embed`` with ``P = 1 + R`` prefix tokens (``cls_token`` and ``reg_token`` [1, R, dim]), eval mode::

    no_embed_class=True   (pos_embed [1, patches, dim])       x = cat(cls, reg, patch_embed(px) + pos_embed)
    no_embed_class=False  (pos_embed [1, patches + P, dim])   x = cat(cls, reg, patch_embed(px)) + pos_embed

Under CPU autocast the patch embedding is bf16 and every parameter fp32: the sum and the concatenation are fp32.  The head reads
``norm(x)[:, 0]`` (``global_pool = 'token'``); the stage-1 hook on ``mlp.fc1`` sees all ``patches + P`` tokens.  ``RegTokenTimmViT``
composes the oracle's timm-layout blocks and the LayerScale restatement of tests/layerscale_models.py with that embedding, in the timm
anatomy the reference duck-types over, and is run through ``oracle.ref_cpu`` like the oracle's own modules.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from layerscale_models import LayerScaleTimmViT, _cfg, _gamma, _grid, bf16_from_bits  # noqa: F401
from oracle.vit_modules import load_flat_weights


class RegTokenTimmViT(LayerScaleTimmViT):
    def __init__(self, *, img, patch, dim, heads, inter, depth, classes, eps=1e-6, layer_scale=None, reg_tokens=0, no_embed_class=False):
        super().__init__(img=img, patch=patch, dim=dim, heads=heads, inter=inter, depth=depth, classes=classes, eps=eps,
                         layer_scale=layer_scale if layer_scale is not None else [(False, False)] * depth)
        patches = (img // patch) ** 2
        self.num_reg_tokens = int(reg_tokens)
        self.num_prefix_tokens = 1 + self.num_reg_tokens
        self.no_embed_class = bool(no_embed_class)
        self.reg_token = nn.Parameter(torch.zeros(1, self.num_reg_tokens, dim)) if self.num_reg_tokens else None
        self.pos_embed = nn.Parameter(torch.zeros(1, patches if self.no_embed_class else patches + self.num_prefix_tokens, dim))

    def _pos_embed(self, x):
        b = x.shape[0]
        to_cat = [self.cls_token.expand(b, -1, -1)]
        if self.reg_token is not None:
            to_cat.append(self.reg_token.expand(b, -1, -1))
        if self.no_embed_class:
            return torch.cat(to_cat + [x + self.pos_embed], dim=1)
        return torch.cat(to_cat + [x], dim=1) + self.pos_embed

    def forward(self, x):
        x = self._pos_embed(self.patch_embed(x))
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x)[:, 0])


@torch.no_grad()
def build_regtoken(w) -> nn.Module:
    """A flat dictionary with ``reg`` / ``no_embed_class`` (and ``ls1.i`` / ``ls2.i``) -> the eval-mode fp32 CPU module (timm anatomy)."""
    depth = int(w["depth"])
    has = [(f"ls1.{i}" in w, f"ls2.{i}" in w) for i in range(depth)]
    regs = int(w["reg"].shape[1]) if w.get("reg") is not None else 0
    m = load_flat_weights(RegTokenTimmViT(**_cfg(w), eps=float(w.get("eps", 1e-6)), layer_scale=has, reg_tokens=regs,
                                          no_embed_class=bool(w.get("no_embed_class", False))), w)
    if regs:
        m.reg_token.copy_(w["reg"].reshape(m.reg_token.shape))
    for i, blk in enumerate(m.blocks):
        for name in ("ls1", "ls2"):
            if f"{name}.{i}" in w:
                getattr(blk, name).gamma.copy_(w[f"{name}.{i}"].reshape(-1))
    return m.eval()


def embed_tokens(w, y: torch.Tensor) -> torch.Tensor:
    """The statement of the token layout on the host: y [n, patches, dim] = float(bf16 patch embedding) -> x [n, tokens, dim] fp32."""
    n, patches, dim = y.shape
    regs = int(w["reg"].shape[1]) if w.get("reg") is not None else 0
    P = 1 + regs
    pos = w["pos"].reshape(-1, dim)
    x = torch.empty(n, patches + P, dim)
    pre = torch.cat([w["cls"].reshape(1, dim)] + ([w["reg"].reshape(regs, dim)] if regs else []), 0)
    if w.get("no_embed_class"):
        x[:, :P] = pre
        x[:, P:] = y + pos
    else:
        x[:, :P] = pre + pos[:P]
        x[:, P:] = y + pos[P:]
    return x


# ------------------------------------------------------------------------------------------- golden cases (tests/golden/reg_*.npz)
# tag -> (VIT_CONFIGS name, batches, images per batch, prune count t per block, min_remaining, K blocks, weight scale, planner targets).
# tests/golden/make_golden_regtokens.py writes the reference's outputs for these inputs; the tests regenerate the inputs from the same
# seeds and check the stored checksums.
REG_GOLDEN_CASES = {
    "reg_test4": ("vit_test_patch16_32_reg4", 2, 8, 40, 16, 2, 0.1, (0.25, 0.375, 0.5)),
    "reg_test2pe": ("vit_test_patch16_32_reg2_pe", 2, 8, 40, 16, 2, 0.1, (0.25, 0.375, 0.5)),
    "reg_deit3_s16": ("deit3_small_patch16_224_d2", 2, 16, 576, 512, 1, 0.03, (0.25, 0.375, 0.5)),
    "reg_dinov2_s14": ("vit_small_patch14_reg4_dinov2_224_d2", 2, 8, 576, 512, 1, 0.03, (0.25, 0.375, 0.5)),
}


def weak_neurons(tag: str, block: int) -> torch.Tensor:
    """The FFN neurons of a golden case whose fc1 row and bias are scaled by 1 / 4 (exact): t of them per block (5 / 16 of 128, 3 / 8 of
    1536), spread over the width and other ones in every block — the cut at t falls into a gap far wider than any score tolerance, so
    the mask step's answer is decided (ssp2vit.mask_parity: `guaranteed`)."""
    from ssp2vit.weights import VIT_CONFIGS
    d_int, t = VIT_CONFIGS[REG_GOLDEN_CASES[tag][0]][4], REG_GOLDEN_CASES[tag][3]
    num, den = (5, 16) if (d_int, t) == (128, 40) else (3, 8)
    j = torch.arange(d_int)
    weak = j[(j * 5 + block) % den < num]
    assert weak.numel() == t
    return weak


def golden_weights(tag: str):
    """The flat dictionary of a golden case: the shapes of synthetic_weights, every matrix, bias, embedding and register token drawn by
    _grid from an integer generator (matrices at the case's std, biases at 0.02), LayerNorm gamma 1 / beta 0, LayerScale by _gamma; fc1
    rows and biases of weak_neurons() x 1 / 4."""
    from ssp2vit.weights import synthetic_weights
    name, std = REG_GOLDEN_CASES[tag][0], REG_GOLDEN_CASES[tag][6]
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
    name, nb, bs = REG_GOLDEN_CASES[tag][:3]
    from ssp2vit.weights import VIT_CONFIGS
    img = VIT_CONFIGS[name][0]
    g = torch.Generator().manual_seed(1)
    return [_grid((bs, 3, img, img), 64.0, g) / 64.0 for _ in range(nb)]


_GOLDEN = {}


def load_golden(tag: str):
    """-> (flat weights, batches with the stored labels, npz dict) of tests/golden/<tag>.npz; computed once per process and shared
    (callers do not modify it); the regenerated inputs are checked against the stored checksums."""
    if tag in _GOLDEN:
        return _GOLDEN[tag]
    import os
    import numpy as np
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{tag}.npz")))
    w = golden_weights(tag)
    pxs = golden_pixels(tag)
    assert float(z["weights_checksum"]) == sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor)), "weights changed"
    assert float(z["pixels_checksum"]) == sum(float(p.double().sum()) for p in pxs), "pixels changed"
    batches = [{"pixel_values": p, "labels": torch.from_numpy(z[f"labels.{i}"])} for i, p in enumerate(pxs)]
    _GOLDEN[tag] = (w, batches, z)
    return _GOLDEN[tag]
