"""TEST INFRASTRUCTURE — CPU restatement of distilled DeiT (never imported by the product path).

The oracle's modules (oracle/vit_modules.py) know one prefix token.  Distilled DeiT puts a distillation token behind CLS
(tokens = patches + 2, pos_embed covers both) and, in eval mode, returns (head(norm(x)[:, 0]) + head_dist(norm(x)[:, 1])) / 2;
HF's DeiTForImageClassification has the same two tokens and a head on CLS only.  The modules below compose the oracle's blocks
with that embedding and that head, in the two anatomies the reference duck-types over:

* ``DistilledTimmViT``  timm layout (`dist_token`, `head_dist`, `num_prefix_tokens = 2`), called as ``model(px)``;
* ``HFDistilledDeiT``   old-HF layout (`deit.encoder.layer[i]`, `deit.embeddings.distillation_token`, reached through
  ``base_model`` as the reference's `_get_encoder` does), teacher heads (`cls_classifier` + `distillation_classifier`) or a CLS
  ``classifier``; called as ``model(pixel_values=px)`` with ``.logits``.

Both are loaded from the flat dictionary of ``ssp2vit.weights`` and run under CPU autocast through ``oracle.ref_cpu`` like the
oracle's own modules.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn

from oracle.vit_modules import HFLayoutViT, TimmLayoutViT, load_flat_weights


class DistilledTimmViT(TimmLayoutViT):
    def __init__(self, *, img, patch, dim, heads, inter, depth, classes, eps=1e-6):
        super().__init__(img=img, patch=patch, dim=dim, heads=heads, inter=inter, depth=depth, classes=classes, eps=eps)
        self.pos_embed = nn.Parameter(torch.zeros(1, (img // patch) ** 2 + 2, dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.head_dist = nn.Linear(dim, classes)
        self.num_prefix_tokens = 2
        self.global_pool = "token"
        self.fc_norm = nn.Identity()
        self.no_embed_class = False
        self.reg_token = None

    def forward(self, x):
        x = self.patch_embed(x)
        b = x.shape[0]
        x = torch.cat((self.cls_token.expand(b, -1, -1), self.dist_token.expand(b, -1, -1), x), dim=1) + self.pos_embed
        for blk in self.blocks:
            x = blk(x)
        x = self.norm(x)
        return (self.head(x[:, 0]) + self.head_dist(x[:, 1])) / 2


class _DistEmbeddings(nn.Module):
    """HF embeddings with the distillation token behind CLS."""
    def __init__(self, emb, dim, n_tok):
        super().__init__()
        self.cls_token = emb.cls_token
        self.distillation_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.position_embeddings = nn.Parameter(torch.zeros(1, n_tok, dim))
        self.patch_embeddings = emb.patch_embeddings

    def forward(self, px):
        e = self.patch_embeddings(px)
        b = e.shape[0]
        e = torch.cat((self.cls_token.expand(b, -1, -1), self.distillation_token.expand(b, -1, -1), e), dim=1)
        return e + self.position_embeddings


class HFDistilledDeiT(nn.Module):
    """`deit` = the oracle's HF backbone with the distillation token; teacher heads or a CLS classifier."""
    def __init__(self, backbone: HFLayoutViT, classes: int, teacher: bool = True):
        super().__init__()
        self.config = backbone.config
        self.deit = backbone.vit
        self.teacher = teacher
        dim = backbone.classifier.in_features
        if teacher:
            self.cls_classifier = nn.Linear(dim, classes)
            self.distillation_classifier = nn.Linear(dim, classes)
        else:
            self.classifier = nn.Linear(dim, classes)

    @property
    def base_model(self):
        return self.deit

    def forward(self, pixel_values=None):
        seq = self.deit(pixel_values)
        if self.teacher:
            return SimpleNamespace(logits=(self.cls_classifier(seq[:, 0, :]) + self.distillation_classifier(seq[:, 1, :])) / 2)
        return SimpleNamespace(logits=self.classifier(seq[:, 0, :]))


def _cfg(w):
    return dict(img=int(w["img"]), patch=int(w["patch"]), dim=int(w["dim"]), heads=int(w["heads"]),
                inter=[int(w[f"fc1_w.{i}"].shape[0]) for i in range(int(w["depth"]))], depth=int(w["depth"]),
                classes=int(w["classes"]))


@torch.no_grad()
def build_distilled(w, layout: str = "timm", teacher: bool = True) -> nn.Module:
    """A distilled flat dictionary (prefix_tokens 2, dist, head_dist_*) -> the eval-mode fp32 CPU module of `layout` ("timm" /
    "hf"); teacher=False (hf only): DeiTForImageClassification's CLS head, head_w."""
    put = lambda p, t: p.copy_(t.reshape(p.shape))
    n_tok = (int(w["img"]) // int(w["patch"])) ** 2 + 2
    if layout == "timm":
        m = load_flat_weights(DistilledTimmViT(**_cfg(w), eps=float(w.get("eps", 1e-6))), w)
        put(m.dist_token, w["dist"])
        put(m.head_dist.weight, w["head_dist_w"]); put(m.head_dist.bias, w["head_dist_b"])
        return m.eval()
    if layout != "hf":
        raise ValueError(layout)
    hf = HFLayoutViT(**_cfg(w), eps=float(w.get("eps", 1e-12)))
    hf.vit.embeddings = _DistEmbeddings(hf.vit.embeddings, int(w["dim"]), n_tok)
    load_flat_weights(hf, w)
    put(hf.vit.embeddings.distillation_token, w["dist"])
    m = HFDistilledDeiT(hf, int(w["classes"]), teacher)
    if teacher:
        put(m.cls_classifier.weight, w["head_w"]); put(m.cls_classifier.bias, w["head_b"])
        put(m.distillation_classifier.weight, w["head_dist_w"]); put(m.distillation_classifier.bias, w["head_dist_b"])
    else:
        put(m.classifier.weight, w["head_w"]); put(m.classifier.bias, w["head_b"])
    return m.eval()


# ------------------------------------------------------------------------------------------- golden cases (tests/golden/deit_*.npz)
# tag -> (VIT_CONFIGS name, batches, images per batch, prune count t per block, min_remaining, K blocks, weight scale); the tiny model's
# scale is larger so that bypassing an attention block moves predictions (non-zero impacts).  tests/golden/make_golden_deit.py writes
# the reference's outputs for these inputs; the tests regenerate the inputs from the same seeds and check the stored checksums.
DEIT_GOLDEN_CASES = {
    "deit_test": ("deit_test_distilled_patch16_32", 2, 8, 40, 16, 2, 0.1),
    "deit_s16": ("deit_small_distilled_patch16_224_d2", 2, 16, 576, 512, 1, 0.03),
}


def _grid(shape, scale, g):
    """Values k * scale / 64, k uniform in [-127, 127], from an INTEGER generator: the same bits on every host (the float samplers'
    last bits differ between host CPUs), and bf16-representable up to the scale's exponent."""
    return torch.randint(-127, 128, tuple(shape), generator=g).float() * (scale / 64.0)


def golden_weights(tag: str, layout: str):
    """The distilled flat dictionary of a golden case: the shapes of synthetic_weights, every matrix, bias and embedding drawn by _grid
    (matrices at the case's std, biases at 0.02), LayerNorm gamma 1 / beta 0."""
    from ssp2vit.weights import synthetic_weights
    name, std = DEIT_GOLDEN_CASES[tag][0], DEIT_GOLDEN_CASES[tag][6]
    w = synthetic_weights(name, classes=10, seed=0, std=std, eps=1e-6 if layout == "timm" else 1e-12)
    g = torch.Generator().manual_seed(0)
    for k, v in list(w.items()):
        if isinstance(v, torch.Tensor) and not k.startswith(("ln1_", "ln2_", "lnf_")):
            bias = k.endswith("_b") or "_b." in k
            w[k] = _grid(v.shape, 0.02 if bias else std, g)
    return w


def golden_pixels(tag: str):
    name, nb, bs = DEIT_GOLDEN_CASES[tag][:3]
    img = 32 if name.endswith("patch16_32") else 224
    g = torch.Generator().manual_seed(1)
    return [_grid((bs, 3, img, img), 64.0, g) / 64.0 for _ in range(nb)]


def load_golden(tag: str, layout: str):
    """-> (flat weights, batches with the stored labels, npz dict) of tests/golden/<tag>_<layout>.npz; the regenerated inputs are checked
    against the stored checksums."""
    import os
    import numpy as np
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{tag}_{layout}.npz")))
    w = golden_weights(tag, layout)
    pxs = golden_pixels(tag)
    assert float(z["weights_checksum"]) == sum(float(v.double().sum()) for v in w.values() if isinstance(v, torch.Tensor)), "weights changed"
    assert float(z["pixels_checksum"]) == sum(float(p.double().sum()) for p in pxs), "pixels changed"       # (exact: integer draws)
    batches = [{"pixel_values": p, "labels": torch.from_numpy(z[f"labels.{i}"])} for i, p in enumerate(pxs)]
    return w, batches, z


def bf16_from_bits(a) -> torch.Tensor:
    import numpy as np
    return torch.from_numpy(np.asarray(a).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
