"""Flat ViT weight dictionary: the one format the HIP engine is loaded from.

Keys (all tensors fp32, CPU, contiguous; layer index ``i`` in ``0..depth-1``)::

    img patch dim heads depth classes eps            python scalars
    patch_w [dim,3,p,p]  patch_b [dim]               conv k=s=p   (a3 in SURVEY.md §8a)
    cls [1,1,dim]  pos [1,N,dim]
    ln1_g.i ln1_b.i [dim]
    qkv_w.i [3*dim,dim]  qkv_b.i [3*dim]             rows ordered [q|k|v][head][d_h]
    proj_w.i [dim,dim]   proj_b.i [dim]
    ln2_g.i ln2_b.i [dim]
    fc1_w.i [d_int_i,dim] fc1_b.i [d_int_i]
    fc2_w.i [dim,d_int_i] fc2_b.i [dim]
    lnf_g lnf_b [dim]    head_w [classes,dim]  head_b [classes]
    prefix_tokens                                    1 (CLS), or 2 (CLS + distillation token: distilled DeiT); default 1
    dist [1,1,dim]                                   the distillation token (prefix_tokens == 2)
    head_dist_w [classes,dim]  head_dist_b [classes] the distillation head: logits = (head(CLS) + head_dist(DIST)) / 2
    reg [1,R,dim]                                    register tokens between CLS and the patches (timm reg_token, R = 1..8):
                                                     prefix_tokens = 1 + R; kept fp32, never rounded; not together with dist
    no_embed_class                                   bool, default False.  True (timm no_embed_class: DeiT-III, DINOv2-reg): pos is
                                                     [1,patches,dim] and the prefix tokens get no position row
    ls1.i ls2.i [dim]                                LayerScale (timm Block.ls1 / ls2 gamma; absent = none): x += ls1 * attn(...),
                                                     x += ls2 * mlp(...); kept fp32, never rounded

N = patches + prefix_tokens: pos covers every token, unless ``no_embed_class`` (N = patches then).  A model with two prefix tokens
and no ``head_dist_w`` (HF ``DeiTForImageClassification``) reads its head on CLS only.  The head of a register model reads CLS.

``nn.Linear`` row-major ``[out,in]`` is kept as is: it is already the K-contiguous "B^T" layout
the MFMA GEMM wants.  Anatomy adapters (``from_module``) accept the same three layouts the
reference duck-types over (/root/reference/src/vit_pruning.py:27-67) plus the renamed layout of
transformers>=5.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

# name -> (img, patch, dim, heads, d_int, depth)
VIT_CONFIGS = {
    "vit_tiny_patch16_224": (224, 16, 192, 3, 768, 12),
    "vit_small_patch16_224": (224, 16, 384, 6, 1536, 12),
    "vit_base_patch16_224": (224, 16, 768, 12, 3072, 12),
    "vit_large_patch16_224": (224, 16, 1024, 16, 4096, 24),
    "vit_huge_patch14_224": (224, 14, 1280, 16, 5120, 32),
    # the reference's own smoke-test config (experiments/vit_pruning/test_stage2_attention_only.py:44-53)
    "vit_test_patch16_32": (32, 16, 64, 4, 128, 4),
    # two-block cuts of the large geometries (same kernels / tile shapes as the full models, test-sized)
    "vit_base_patch16_224_d3": (224, 16, 768, 12, 3072, 3),
    "vit_large_patch16_224_d2": (224, 16, 1024, 16, 4096, 2),
    "vit_huge_patch14_224_d2": (224, 14, 1280, 16, 5120, 2),
    "vit_small_patch16_224_d2": (224, 16, 384, 6, 1536, 2),
    # geometries beside BASELINE's: ViT-L/14 (257 tokens at d_h = 64), ViT-B/32 (50 tokens, 3072-wide patches), B/16 at 160 / 208 pixels
    "vit_large_patch14_224": (224, 14, 1024, 16, 4096, 24),
    "vit_base_patch32_224": (224, 32, 768, 12, 3072, 12),
    "vit_large_patch14_224_d2": (224, 14, 1024, 16, 4096, 2),
    "vit_base_patch32_224_d2": (224, 32, 768, 12, 3072, 2),
    "vit_base_patch16_160_d2": (160, 16, 768, 12, 3072, 2),
    "vit_base_patch16_208_d2": (208, 16, 768, 12, 3072, 2),
    "vit_base_patch16_240_d2": (240, 16, 768, 12, 3072, 2),
    # sequences over 288 tokens (the key-streaming attention: SSP2_ATTN_STREAM=1 / VitEngine(attn_stream=1) / --long-sequences):
    # the reference's SRP models at 384 pixels (577 tokens) and test cuts of them, /8 at 224 (785 tokens), /16 at 512 (1025 tokens)
    "vit_tiny_patch16_384": (384, 16, 192, 3, 768, 12),
    "vit_small_patch16_384": (384, 16, 384, 6, 1536, 12),
    "vit_base_patch16_384": (384, 16, 768, 12, 3072, 12),
    "vit_large_patch16_384": (384, 16, 1024, 16, 4096, 24),
    "vit_small_patch16_384_d3": (384, 16, 384, 6, 1536, 3),
    "vit_base_patch16_384_d2": (384, 16, 768, 12, 3072, 2),
    "vit_small_patch8_224_d2": (224, 8, 384, 6, 1536, 2),
    "vit_tiny_patch16_512_d2": (512, 16, 192, 3, 768, 2),
    # distilled DeiT (a distillation token behind CLS, logits = mean of the CLS and DIST heads: DISTILLED below) and test cuts of it;
    # the 32-pixel test config has 4 patches + 2 = 6 tokens at d_h = 16
    "deit_tiny_distilled_patch16_224": (224, 16, 192, 3, 768, 12),
    "deit_small_distilled_patch16_224": (224, 16, 384, 6, 1536, 12),
    "deit_base_distilled_patch16_224": (224, 16, 768, 12, 3072, 12),
    "deit_base_distilled_patch16_384": (384, 16, 768, 12, 3072, 12),
    "deit_small_distilled_patch16_224_d2": (224, 16, 384, 6, 1536, 2),
    "deit_base_distilled_patch16_384_d2": (384, 16, 768, 12, 3072, 2),
    "deit_test_distilled_patch16_32": (32, 16, 64, 4, 128, 4),
    # LayerScale on both residual branches (LAYER_SCALE below): the DINOv2 backbones with a linear head at 518 pixels (1370 tokens, d_h 64:
    # the key-streaming attention) and at 224 (257 tokens), and test cuts
    "vit_small_patch14_dinov2": (518, 14, 384, 6, 1536, 12),
    "vit_base_patch14_dinov2": (518, 14, 768, 12, 3072, 12),
    "vit_large_patch14_dinov2": (518, 14, 1024, 16, 4096, 24),
    "vit_small_patch14_dinov2_224": (224, 14, 384, 6, 1536, 12),
    "vit_base_patch14_dinov2_224": (224, 14, 768, 12, 3072, 12),
    "vit_large_patch14_dinov2_224": (224, 14, 1024, 16, 4096, 24),
    "vit_small_patch14_dinov2_d2": (518, 14, 384, 6, 1536, 2),
    "vit_small_patch16_224_ls_d2": (224, 16, 384, 6, 1536, 2),
    "vit_test_patch16_32_ls": (32, 16, 64, 4, 128, 4),
    # DeiT-III: class-free positions (NO_EMBED_CLASS below: pos has the patches' rows only) and LayerScale
    "deit3_small_patch16_224": (224, 16, 384, 6, 1536, 12),
    "deit3_base_patch16_224": (224, 16, 768, 12, 3072, 12),
    "deit3_large_patch16_224": (224, 16, 1024, 16, 4096, 24),
    "deit3_base_patch16_384": (384, 16, 768, 12, 3072, 12),
    "deit3_small_patch16_224_d2": (224, 16, 384, 6, 1536, 2),
    # DINOv2 with four register tokens between CLS and the patches (REG_TOKENS below), class-free positions and LayerScale: 1374 tokens
    # at 518 pixels (the key-streaming attention), 261 at 224; and test cuts.  vit_test_patch16_32_reg4 has 4 + 5 = 9 tokens at d_h 16;
    # vit_test_patch16_32_reg2_pe two registers with positions for every token (7 tokens), no LayerScale
    "vit_small_patch14_reg4_dinov2": (518, 14, 384, 6, 1536, 12),
    "vit_base_patch14_reg4_dinov2": (518, 14, 768, 12, 3072, 12),
    "vit_large_patch14_reg4_dinov2": (518, 14, 1024, 16, 4096, 24),
    "vit_small_patch14_reg4_dinov2_224": (224, 14, 384, 6, 1536, 12),
    "vit_base_patch14_reg4_dinov2_224": (224, 14, 768, 12, 3072, 12),
    "vit_large_patch14_reg4_dinov2_224": (224, 14, 1024, 16, 4096, 24),
    "vit_small_patch14_reg4_dinov2_224_d2": (224, 14, 384, 6, 1536, 2),
    "vit_small_patch14_reg4_dinov2_d2": (518, 14, 384, 6, 1536, 2),
    "vit_test_patch16_32_reg4": (32, 16, 64, 4, 128, 4),
    "vit_test_patch16_32_reg2_pe": (32, 16, 64, 4, 128, 4),
}
# VIT_CONFIGS entries with a distillation token and head (their entries stay (img, patch, dim, heads, d_int, depth))
DISTILLED = frozenset(k for k in VIT_CONFIGS if k.startswith("deit_") and "_distilled_" in k)


# VIT_CONFIGS entries whose blocks carry LayerScale (synthetic_weights draws ls1 / ls2 for them by default)
LAYER_SCALE = frozenset(k for k in VIT_CONFIGS if "_dinov2" in k or k.endswith(("_ls", "_ls_d2")) or k.startswith("deit3_")
                        or k == "vit_test_patch16_32_reg4")

# VIT_CONFIGS entries with register tokens between CLS and the patches: name -> how many ("_reg<R>" in the name)
REG_TOKENS = {k: int(k.split("_reg")[1][0]) for k in VIT_CONFIGS if "_reg" in k}

# VIT_CONFIGS entries with class-free positions (timm no_embed_class=True: pos has the patches' rows only)
NO_EMBED_CLASS = frozenset(k for k in VIT_CONFIGS if k.startswith("deit3_") or (k in REG_TOKENS and not k.endswith("_pe")))

MAX_REG_TOKENS = 8                                      # the engine's limit (ssp2_create_layout)


def prefix_tokens_of(name: str) -> int:
    """Tokens in front of the patches of a VIT_CONFIGS model: 2 for the distilled DeiTs, 1 + R with R register tokens, else 1."""
    return 2 if name in DISTILLED else 1 + REG_TOKENS.get(name, 0)


def n_tokens(w: Dict) -> int:
    return (int(w["img"]) // int(w["patch"])) ** 2 + int(w.get("prefix_tokens", 1))


def synthetic_weights(name: str = "vit_base_patch16_224", classes: int = 1000, seed: int = 0,
                      std: float = 0.02, eps: float = 1e-6, spread: Optional[float] = None,
                      bias_std: float = 0.0, layer_scale: Optional[bool] = None) -> Dict:
    """Seeded random-init weights of a named architecture (no checkpoints exist offline).

    trunc-normal(std) matrices, LN gamma=1 beta=0, zero (or N(0,bias_std)) biases.  ``spread`` scales
    fc1 rows by a log-uniform factor in [1/spread, spread] so stage-1 scores are well separated
    (SURVEY.md §8d).  ``layer_scale`` (default: the model is in LAYER_SCALE) adds ``ls1.i`` / ``ls2.i``: magnitudes log-uniform in
    [1e-3, 2], about a quarter of them negative — not the 1e-5 init value, so that a column-mapping error moves a result by far more
    than any tolerance.  They are drawn from a generator of their own: the other tensors are the same with and without them.
    Models in REG_TOKENS get ``reg`` (trunc-normal(std), from a generator of its own as well); models in NO_EMBED_CLASS get
    ``no_embed_class = True`` and a ``pos`` of the patches' rows only.
    """
    img, patch, dim, heads, inter, depth = VIT_CONFIGS[name]
    g = torch.Generator().manual_seed(seed)

    def tn(*shape, s=std):
        t = torch.empty(*shape)
        torch.nn.init.trunc_normal_(t, std=s, a=-2 * s, b=2 * s, generator=g)
        return t

    def bias(n):
        return torch.randn(n, generator=g) * bias_std if bias_std > 0 else torch.zeros(n)

    prefix = prefix_tokens_of(name)
    n_tok = (img // patch) ** 2 + prefix
    w: Dict = dict(img=img, patch=patch, dim=dim, heads=heads, depth=depth, classes=classes, eps=eps)
    if prefix != 1:
        w["prefix_tokens"] = prefix
    w["patch_w"] = tn(dim, 3, patch, patch)
    w["patch_b"] = bias(dim)
    w["cls"] = tn(1, 1, dim)
    w["pos"] = tn(1, n_tok - prefix if name in NO_EMBED_CLASS else n_tok, dim)
    for i in range(depth):
        w[f"ln1_g.{i}"] = torch.ones(dim); w[f"ln1_b.{i}"] = torch.zeros(dim)
        w[f"qkv_w.{i}"] = tn(3 * dim, dim); w[f"qkv_b.{i}"] = bias(3 * dim)
        w[f"proj_w.{i}"] = tn(dim, dim); w[f"proj_b.{i}"] = bias(dim)
        w[f"ln2_g.{i}"] = torch.ones(dim); w[f"ln2_b.{i}"] = torch.zeros(dim)
        fc1 = tn(inter, dim)
        if spread is not None and spread > 1.0:
            u = torch.rand(inter, generator=g) * 2 - 1
            fc1 = fc1 * torch.exp(u * math.log(spread)).unsqueeze(1)
        w[f"fc1_w.{i}"] = fc1; w[f"fc1_b.{i}"] = bias(inter)
        w[f"fc2_w.{i}"] = tn(dim, inter); w[f"fc2_b.{i}"] = bias(dim)
    w["lnf_g"] = torch.ones(dim); w["lnf_b"] = torch.zeros(dim)
    w["head_w"] = tn(classes, dim); w["head_b"] = bias(classes)
    if name in DISTILLED:
        w["dist"] = tn(1, 1, dim)
        w["head_dist_w"] = tn(classes, dim); w["head_dist_b"] = bias(classes)
    if name in NO_EMBED_CLASS:
        w["no_embed_class"] = True
    if name in REG_TOKENS:
        gr = torch.Generator().manual_seed(seed + 104729)
        reg = torch.empty(1, REG_TOKENS[name], dim)
        torch.nn.init.trunc_normal_(reg, std=std, a=-2 * std, b=2 * std, generator=gr)
        w["reg"] = reg
    if (name in LAYER_SCALE) if layer_scale is None else layer_scale:
        gl = torch.Generator().manual_seed(seed + 7919)
        lo, hi = math.log(1e-3), math.log(2.0)
        for i in range(depth):
            for k in ("ls1", "ls2"):
                mag = torch.exp(torch.rand(dim, generator=gl) * (hi - lo) + lo)
                w[f"{k}.{i}"] = torch.where(torch.rand(dim, generator=gl) < 0.25, -mag, mag)
    return w


def count_params(w: Dict) -> int:
    return sum(int(v.numel()) for v in w.values() if isinstance(v, torch.Tensor))


# ----------------------------------------------------------------------------- anatomy adapters
def _f32(t) -> torch.Tensor:
    """fp32 view / copy ON THE TENSOR'S OWN DEVICE: the engine reads device-resident weights in place
    (ssp2_load_tensor_dev), so a module that lives on the GPU never round-trips through the host."""
    return t.detach().to(torch.float32).contiguous()


def _bias_or_zeros(lin) -> torch.Tensor:
    """nn.Linear bias, or zeros when the layer was built with bias=False (timm's qkv_bias=False)."""
    return _f32(lin.bias) if getattr(lin, "bias", None) is not None else torch.zeros(lin.weight.shape[0], device=lin.weight.device)


def detect_layout(model) -> str:
    """'timm' | 'hf' (transformers<5: vit.encoder.layer) | 'hf5' (transformers>=5: vit.layers)."""
    if hasattr(model, "blocks") and hasattr(model, "patch_embed"):
        return "timm"
    base = getattr(model, "vit", None) or getattr(model, "base_model", None) or model
    enc = getattr(base, "encoder", base)
    if hasattr(enc, "layer"):
        return "hf"
    if hasattr(base, "layers") or hasattr(enc, "layers"):
        return "hf5"
    raise AttributeError("Unsupported ViT model structure: expected encoder.layer or blocks")


def score_site_for(layout: str) -> str:
    """Where the reference's stage-1 hook lands (vit_pruning.py:130 vs :135)."""
    return "pre_gelu" if layout == "timm" else "post_gelu"


def reg_tokens_of(w: Dict) -> int:
    """Register tokens of a flat dictionary (rows of `reg`, 0 without it)."""
    return int(w["reg"].shape[-2]) if w.get("reg") is not None else 0


def _timm_reg_tokens(model) -> int:
    """Register tokens of a timm-layout module: rows of `reg_token` [1, R, dim], checked against `num_reg_tokens`."""
    reg = getattr(model, "reg_token", None)
    nreg = getattr(model, "num_reg_tokens", None)
    if reg is None:
        if int(nreg or 0) > 0:
            raise ValueError(f"reg_token: num_reg_tokens={int(nreg)} but the model has no reg_token parameter")
        return 0
    if reg.dim() != 3 or int(reg.shape[0]) != 1 or int(reg.shape[1]) < 1:
        raise ValueError(f"reg_token: shape {tuple(reg.shape)} is not [1, R, dim]")
    r = int(reg.shape[1])
    if nreg is not None and int(nreg) != r:
        raise ValueError(f"reg_token: {r} rows but num_reg_tokens={int(nreg)}")
    if r > MAX_REG_TOKENS:
        raise ValueError(f"reg_token: {r} register tokens, the engine takes up to {MAX_REG_TOKENS}")
    return r


def _check_timm_token_layout(model) -> Tuple[int, int, bool]:
    """(prefix tokens, register tokens, no_embed_class) of a timm-layout module — CLS [+ dist_token], or CLS + up to 8 rows of
    `reg_token`, with positions for every token or class-free (`no_embed_class`) — after refusing, by the attribute's name, every
    layout the engine cannot represent and every set of attributes that does not agree with itself: registers or class-free
    positions beside a `dist_token` (timm's distilled class has neither), `num_reg_tokens` without a `reg_token`, `no_embed_class`
    on a `pos_embed` that is no square number of rows, a `num_prefix_tokens` that is not the count of the tokens found, a pooled
    head (`global_pool` other than 'token', a `fc_norm` that is not Identity)."""
    regs = _timm_reg_tokens(model)
    dist = getattr(model, "dist_token", None) is not None
    nec = bool(getattr(model, "no_embed_class", False))
    if regs and dist:
        raise ValueError("reg_token: register tokens beside a dist_token are not supported (timm's distilled models have none)")
    if nec and dist:
        raise ValueError("no_embed_class: class-free positions beside a dist_token are not supported (timm's distilled models have positions for every token)")
    if nec:
        rows = int(model.pos_embed.shape[1])
        side = int(round(math.sqrt(rows)))
        if side < 1 or side * side != rows:
            raise ValueError(f"no_embed_class: True, but pos_embed has {rows} rows, which is no square number of patches")
    pool = getattr(model, "global_pool", "token")
    if pool not in ("token", None):
        raise ValueError(f"global_pool={pool!r}: only the token head ('token': the head reads CLS [+ DIST]) is supported")
    fcn = getattr(model, "fc_norm", None)
    if fcn is not None and not isinstance(fcn, torch.nn.Identity):
        raise ValueError(f"fc_norm: a {type(fcn).__name__} in front of the head is not supported (only Identity)")
    prefix = 1 + regs + int(dist)
    npt = getattr(model, "num_prefix_tokens", None)
    if npt is not None and int(npt) != prefix:
        raise ValueError(f"num_prefix_tokens={int(npt)}: the model has CLS{' + dist_token' if dist else ''}"
                         f"{f' + {regs} register token(s)' if regs else ''} = {prefix} prefix token(s)")
    return prefix, regs, nec


def _timm_layer_scale(block, name: str, dim: int, where: str) -> Optional[torch.Tensor]:
    """gamma of a timm block's `ls1` / `ls2` (LayerScale: x * gamma, an fp32 product under autocast); None for an absent attribute or an
    nn.Identity (init_values=None).  Refused by name: `inplace=True` (x.mul_(gamma) rounds the product to the branch's bf16 — other
    arithmetic), HF's `lambda1` parameter, anything else without a gamma, a gamma that is not [dim]."""
    ls = getattr(block, name, None)
    if ls is None or isinstance(ls, torch.nn.Identity):
        return None
    if getattr(ls, "lambda1", None) is not None:
        raise ValueError(f"{where}.{name}.lambda1: HF-style LayerScale (Dinov2LayerScale) is not supported")
    gamma = getattr(ls, "gamma", None)
    if gamma is None:
        raise ValueError(f"{where}.{name}: a {type(ls).__name__} without a `gamma` parameter is not a LayerScale this build knows")
    if bool(getattr(ls, "inplace", False)):
        raise ValueError(f"{where}.{name}.inplace: an in-place LayerScale rounds gamma * x to bf16 under autocast (other arithmetic); not supported")
    if gamma.dim() != 1 or int(gamma.numel()) != dim:
        raise ValueError(f"{where}.{name}.gamma: shape {tuple(gamma.shape)} is not [{dim}]")
    return _f32(gamma)


def _refuse_hf_layer_scale(layer, where: str) -> None:
    """HF DINOv2 blocks (`layer_scale1.lambda1` / `layer_scale2.lambda1`): its classifier concatenates CLS with the mean patch token, which
    the engine's head does not compute — refused by name rather than pruned as another network."""
    for name in ("layer_scale1", "layer_scale2"):
        if getattr(layer, name, None) is not None:
            raise ValueError(f"{where}.{name}.lambda1: HF DINOv2 LayerScale is not supported (its head reads CLS and the mean patch token); "
                             "use the timm layout (blocks[i].ls1.gamma)")


def has_layer_scale(model) -> Tuple[Tuple[bool, bool], ...]:
    """Per block of a timm-layout module: (ls1 is a LayerScale, ls2 is one), read without copying a weight; () for the HF layouts."""
    if detect_layout(model) != "timm":
        return ()
    is_ls = lambda b, n: getattr(b, n, None) is not None and not isinstance(getattr(b, n), torch.nn.Identity)
    return tuple((is_ls(b, "ls1"), is_ls(b, "ls2")) for b in model.blocks)


def _hf_base(model):
    """The HF backbone (ViTModel / DeiTModel) of a classification model, or the model itself."""
    for name in ("vit", "deit"):
        b = getattr(model, name, None)
        if b is not None:
            return b
    b = getattr(model, "base_model", None)
    return b if b is not None and b is not model and hasattr(b, "embeddings") else model


def _hf_heads(model, w: Dict) -> None:
    """HF classifiers: `classifier` (ViT, DeiTForImageClassification: the CLS row) or the teacher model's `cls_classifier` +
    `distillation_classifier` (logits = their mean, DeiTForImageClassificationWithTeacher)."""
    if hasattr(model, "cls_classifier") and hasattr(model, "distillation_classifier"):
        w["head_w"], w["head_b"] = _f32(model.cls_classifier.weight), _bias_or_zeros(model.cls_classifier)
        w["head_dist_w"], w["head_dist_b"] = _f32(model.distillation_classifier.weight), _bias_or_zeros(model.distillation_classifier)
    elif isinstance(getattr(model, "classifier", None), torch.nn.Linear):
        w["head_w"], w["head_b"] = _f32(model.classifier.weight), _bias_or_zeros(model.classifier)
    else:
        raise AttributeError("classifier: the HF model has no Linear classification head — the search evaluates top-1")


def _hf_embeddings(emb, w: Dict) -> None:
    if getattr(emb, "register_tokens", None) is not None:
        raise ValueError("register_tokens: register tokens are not supported")
    w["cls"], w["pos"] = _f32(emb.cls_token), _f32(emb.position_embeddings)
    if getattr(emb, "distillation_token", None) is not None:
        w["dist"] = _f32(emb.distillation_token)
        w["prefix_tokens"] = 2


def _side_of(w: Dict) -> int:
    """Patches per side from the position embedding: patches + prefix tokens rows, or with `no_embed_class` the patches' rows only;
    a count that does not fit the dictionary's reading is refused rather than misread."""
    prefix = 0 if w.get("no_embed_class") else int(w.get("prefix_tokens", 1))
    n_tok = int(w["pos"].shape[1])
    side = int(round(math.sqrt(max(n_tok - prefix, 0))))
    if side < 1 or side * side + prefix != n_tok:
        raise ValueError(f"pos_embed: {n_tok} rows are not {prefix} prefix token(s) + a square number of patches "
                         + ("(no_embed_class: the patches' rows only)" if w.get("no_embed_class") else "(extra tokens are not supported)"))
    return side


def check_flat_layout(w: Dict) -> Tuple[int, int, bool]:
    """(prefix_tokens, register tokens, no_embed_class) of a flat dictionary, validated: `reg` is [1, R, dim] with R <= 8 and
    prefix_tokens = 1 + R, no `dist` / `head_dist_w` beside registers or class-free positions, and `pos` has `patches` rows
    (no_embed_class) or `patches + prefix_tokens` (patches from img / patch)."""
    regs, nec = reg_tokens_of(w), bool(w.get("no_embed_class", False))
    prefix = int(w.get("prefix_tokens", 1))
    if regs:
        if w["reg"].dim() != 3 or int(w["reg"].shape[0]) != 1 or int(w["reg"].shape[2]) != int(w["dim"]):
            raise ValueError(f"reg: shape {tuple(w['reg'].shape)} is not [1, R, {int(w['dim'])}]")
        if regs > MAX_REG_TOKENS:
            raise ValueError(f"reg: {regs} register tokens, the engine takes up to {MAX_REG_TOKENS}")
        if prefix != 1 + regs:
            raise ValueError(f"prefix_tokens={prefix}: CLS + {regs} register token(s) are {1 + regs}")
    if (regs or nec) and (w.get("dist") is not None or "head_dist_w" in w or (not regs and prefix == 2)):
        raise ValueError("dist: a distillation token or head beside register tokens (reg) or class-free positions (no_embed_class) is not supported")
    patches = (int(w["img"]) // int(w["patch"])) ** 2
    rows = int(w["pos"].shape[1])
    if rows != (patches if nec else patches + prefix):
        raise ValueError(f"no_embed_class={nec}: pos has {rows} rows, expected {patches if nec else patches + prefix} "
                         f"({patches} patches{'' if nec else f' + {prefix} prefix token(s)'})")
    return prefix, regs, nec


def token_layout(model) -> tuple:
    """(prefix_tokens, dist_head) of a live module, read from its attributes without copying a weight (the engine cache keys on it)."""
    if detect_layout(model) == "timm":
        dist = getattr(model, "dist_token", None) is not None
        return (2 if dist else 1, int(dist and getattr(model, "head_dist", None) is not None))
    emb = getattr(_hf_base(model), "embeddings", None)
    dist = getattr(emb, "distillation_token", None) is not None
    return (2 if dist else 1, int(dist and hasattr(model, "distillation_classifier")))


def position_layout(model) -> tuple:
    """(register tokens, no_embed_class) of a live module, read from its attributes without copying a weight: the part of the token
    layout `token_layout` does not carry (the engine cache keys on both)."""
    if detect_layout(model) != "timm":
        return (0, False)
    reg = getattr(model, "reg_token", None)
    return (int(reg.shape[1]) if reg is not None and reg.dim() == 3 else 0, bool(getattr(model, "no_embed_class", False)))


def from_module(model) -> Dict:
    """Extract the flat dictionary from a live module (weights are copied, the module is untouched).  Distilled DeiT (timm
    `dist_token` + `head_dist`; HF `distillation_token` + `cls_classifier` / `distillation_classifier`, or a CLS-only `classifier`)
    gives prefix_tokens = 2; layouts the engine cannot represent raise ValueError naming the attribute."""
    layout = detect_layout(model)
    w: Dict = {}
    if layout == "timm":
        prefix, regs, nec = _check_timm_token_layout(model)
        pe = model.patch_embed.proj
        blocks = list(model.blocks)
        w["patch_w"], w["patch_b"] = _f32(pe.weight), _f32(pe.bias)
        w["cls"], w["pos"] = _f32(model.cls_token), _f32(model.pos_embed)
        if regs:
            w["reg"], w["prefix_tokens"] = _f32(model.reg_token), prefix
            if int(w["reg"].shape[2]) != int(w["cls"].shape[-1]):
                raise ValueError(f"reg_token: shape {tuple(w['reg'].shape)} is not [1, R, {int(w['cls'].shape[-1])}]")
        if nec:
            w["no_embed_class"] = True
        if prefix == 2 and not regs:
            w["dist"], w["prefix_tokens"] = _f32(model.dist_token), 2
            if getattr(model, "head_dist", None) is not None:
                w["head_dist_w"], w["head_dist_b"] = _f32(model.head_dist.weight), _bias_or_zeros(model.head_dist)
        for i, b in enumerate(blocks):
            w[f"ln1_g.{i}"], w[f"ln1_b.{i}"] = _f32(b.norm1.weight), _f32(b.norm1.bias)
            attn = getattr(b, "attn", None)
            if attn is not None and hasattr(attn, "qkv"):
                w[f"qkv_w.{i}"], w[f"qkv_b.{i}"] = _f32(attn.qkv.weight), _bias_or_zeros(attn.qkv)
                w[f"proj_w.{i}"], w[f"proj_b.{i}"] = _f32(attn.proj.weight), _bias_or_zeros(attn.proj)
            else:  # attention already replaced by a bypass (a6): zero weights + skip flag
                w[f"attn_absent.{i}"] = True
            w[f"ln2_g.{i}"], w[f"ln2_b.{i}"] = _f32(b.norm2.weight), _f32(b.norm2.bias)
            w[f"fc1_w.{i}"], w[f"fc1_b.{i}"] = _f32(b.mlp.fc1.weight), _f32(b.mlp.fc1.bias)
            w[f"fc2_w.{i}"], w[f"fc2_b.{i}"] = _f32(b.mlp.fc2.weight), _f32(b.mlp.fc2.bias)
            for name in ("ls1", "ls2"):
                gamma = _timm_layer_scale(b, name, int(b.norm1.weight.shape[0]), f"blocks[{i}]")
                if gamma is not None:
                    w[f"{name}.{i}"] = gamma
        w["lnf_g"], w["lnf_b"] = _f32(model.norm.weight), _f32(model.norm.bias)
        w["head_w"], w["head_b"] = _f32(model.head.weight), _bias_or_zeros(model.head)
        eps = float(model.norm.eps)
        # the head count lives on the attention modules; block 0 may already be a bypass (the heuristic prunes it
        # first), so take it from the first block that still has one, then from a config object
        heads = next((int(b.attn.num_heads) for b in blocks if hasattr(getattr(b, "attn", None), "num_heads")), None)
        if heads is None:
            heads = getattr(getattr(model, "config", None), "num_attention_heads", None)
            heads = None if heads is None else int(heads)
    elif layout == "hf":
        vit = _hf_base(model)
        emb = vit.embeddings
        pe = emb.patch_embeddings.projection
        layers = list(vit.encoder.layer)
        w["patch_w"], w["patch_b"] = _f32(pe.weight), _f32(pe.bias)
        _hf_embeddings(emb, w)
        for i, l in enumerate(layers):
            _refuse_hf_layer_scale(l, f"encoder.layer[{i}]")
            w[f"ln1_g.{i}"], w[f"ln1_b.{i}"] = _f32(l.layernorm_before.weight), _f32(l.layernorm_before.bias)
            att = getattr(l, "attention", None)
            sa = getattr(att, "attention", None)
            if sa is not None and hasattr(sa, "query"):
                w[f"qkv_w.{i}"] = torch.cat([_f32(sa.query.weight), _f32(sa.key.weight), _f32(sa.value.weight)], 0)
                w[f"qkv_b.{i}"] = torch.cat([_bias_or_zeros(sa.query), _bias_or_zeros(sa.key), _bias_or_zeros(sa.value)], 0)
                w[f"proj_w.{i}"], w[f"proj_b.{i}"] = _f32(att.output.dense.weight), _f32(att.output.dense.bias)
            else:
                w[f"attn_absent.{i}"] = True
            w[f"ln2_g.{i}"], w[f"ln2_b.{i}"] = _f32(l.layernorm_after.weight), _f32(l.layernorm_after.bias)
            w[f"fc1_w.{i}"], w[f"fc1_b.{i}"] = _f32(l.intermediate.dense.weight), _f32(l.intermediate.dense.bias)
            w[f"fc2_w.{i}"], w[f"fc2_b.{i}"] = _f32(l.output.dense.weight), _f32(l.output.dense.bias)
        w["lnf_g"], w["lnf_b"] = _f32(vit.layernorm.weight), _f32(vit.layernorm.bias)
        _hf_heads(model, w)
        eps = float(vit.layernorm.eps)
        heads = int(getattr(model.config, "num_attention_heads"))
    else:  # hf5: vit.layers[i].{layernorm_before, attention.{q,k,v,o}_proj, layernorm_after, mlp.fc1/fc2}
        vit = _hf_base(model)
        emb = vit.embeddings
        pe = emb.patch_embeddings.projection
        layers = list(getattr(vit, "layers", None) or vit.encoder.layers)
        w["patch_w"], w["patch_b"] = _f32(pe.weight), _f32(pe.bias)
        _hf_embeddings(emb, w)
        for i, l in enumerate(layers):
            _refuse_hf_layer_scale(l, f"layers[{i}]")
            w[f"ln1_g.{i}"], w[f"ln1_b.{i}"] = _f32(l.layernorm_before.weight), _f32(l.layernorm_before.bias)
            a = l.attention
            if hasattr(a, "q_proj"):
                w[f"qkv_w.{i}"] = torch.cat([_f32(a.q_proj.weight), _f32(a.k_proj.weight), _f32(a.v_proj.weight)], 0)
                w[f"qkv_b.{i}"] = torch.cat([_bias_or_zeros(a.q_proj), _bias_or_zeros(a.k_proj), _bias_or_zeros(a.v_proj)], 0)
                w[f"proj_w.{i}"], w[f"proj_b.{i}"] = _f32(a.o_proj.weight), _bias_or_zeros(a.o_proj)
            else:
                w[f"attn_absent.{i}"] = True
            w[f"ln2_g.{i}"], w[f"ln2_b.{i}"] = _f32(l.layernorm_after.weight), _f32(l.layernorm_after.bias)
            w[f"fc1_w.{i}"], w[f"fc1_b.{i}"] = _f32(l.mlp.fc1.weight), _f32(l.mlp.fc1.bias)
            w[f"fc2_w.{i}"], w[f"fc2_b.{i}"] = _f32(l.mlp.fc2.weight), _f32(l.mlp.fc2.bias)
        w["lnf_g"], w["lnf_b"] = _f32(vit.layernorm.weight), _f32(vit.layernorm.bias)
        _hf_heads(model, w)
        eps = float(vit.layernorm.eps)
        heads = int(getattr(model.config, "num_attention_heads"))

    dim = int(w["patch_w"].shape[0])
    patch = int(w["patch_w"].shape[-1])
    side = _side_of(w)
    depth = sum(1 for k in w if k.startswith("ln1_g."))
    if heads is None:
        if depth and all(w.get(f"attn_absent.{i}") for i in range(depth)):
            heads = max(1, dim // 64)       # no attention left anywhere: the value is never used by a kernel
        else:
            raise AttributeError("cannot determine the number of attention heads: no block exposes attn.num_heads and "
                                 "the model has no config.num_attention_heads")
    for i in range(depth):  # bypassed attention: supply zero weights, the engine skips the block anyway
        if w.get(f"attn_absent.{i}"):
            dv = w["patch_w"].device
            w[f"qkv_w.{i}"] = torch.zeros(3 * dim, dim, device=dv); w[f"qkv_b.{i}"] = torch.zeros(3 * dim, device=dv)
            w[f"proj_w.{i}"] = torch.zeros(dim, dim, device=dv); w[f"proj_b.{i}"] = torch.zeros(dim, device=dv)
    w.update(img=side * patch, patch=patch, dim=dim, heads=heads, depth=depth,
             classes=int(w["head_w"].shape[0]), eps=eps, layout=layout)
    return w


# ----------------------------------------------------------------------------- local checkpoints (CLI --weights)
_KNOWN_HEADS = {192: 3, 384: 6, 768: 12, 1024: 16, 1280: 16}       # ViT-Ti / S / B / L / H: the published geometries


def from_state_dict(sd: Dict[str, torch.Tensor], config: Optional[Dict] = None, meta: Optional[Dict] = None) -> Dict:
    """Flat dictionary from a checkpoint's state dict in any of the three key layouts `from_module` reads from live
    modules: timm (`blocks.N.attn.qkv.weight`, ...), transformers < 5 (`vit.encoder.layer.N.attention.attention.query...`)
    and transformers >= 5 (`vit.layers.N.attention.q_proj...`; also under `vit.encoder.layers`).  `config` = the HF
    config.json (heads, layer_norm_eps); `meta` = this build's pruning_meta.json (bypassed attention blocks).  FFN widths
    come from the tensor shapes, so a width-pruned checkpoint loads as it is.  The reference loads its models with
    `from_pretrained` / `timm.create_model` + `load_state_dict` (adaptation-for-Pures-framework/auto_2ssp.py:636-667);
    neither library's model code is needed here."""
    config, meta = dict(config or {}), dict(meta or {})
    f = lambda k: sd[k].detach().to(torch.float32).contiguous()
    has = lambda k: k in sd
    opt = lambda k, n: f(k) if has(k) else torch.zeros(n)
    w: Dict = {}
    absent = set(int(i) for i in meta.get("attention_removed_blocks", []))
    for k in sd:                                                         # HF DINOv2 LayerScale, under any prefix: refused by name (see from_module)
        if k.endswith((".layer_scale1.lambda1", ".layer_scale2.lambda1")):
            raise ValueError(f"{k}: HF DINOv2 LayerScale (layer_scale1.lambda1 / layer_scale2.lambda1) is not supported (its head reads CLS "
                             "and the mean patch token); use the timm layout (blocks.N.ls1.gamma)")
    if has("patch_embed.proj.weight"):                                   # ---- timm
        layout = "timm"
        if has("fc_norm.weight"):
            raise ValueError("fc_norm: a LayerNorm in front of the head (fc_norm: pooled head) not supported")
        if has("reg_token") and has("dist_token"):
            raise ValueError("reg_token: register tokens beside a dist_token are not supported (timm's distilled models have none)")
        w["patch_w"], w["patch_b"] = f("patch_embed.proj.weight"), f("patch_embed.proj.bias")
        w["cls"], w["pos"] = f("cls_token"), f("pos_embed")
        dim = int(w["patch_w"].shape[0])
        if has("dist_token"):                                            # distilled DeiT: CLS + DIST, two heads averaged
            w["dist"], w["prefix_tokens"] = f("dist_token"), 2
        if has("reg_token"):                                             # register tokens: CLS + R rows
            reg = f("reg_token")
            if reg.dim() != 3 or int(reg.shape[0]) != 1 or int(reg.shape[2]) != dim or int(reg.shape[1]) < 1:
                raise ValueError(f"reg_token: shape {tuple(reg.shape)} is not [1, R, {dim}]")
            if int(reg.shape[1]) > MAX_REG_TOKENS:
                raise ValueError(f"reg_token: {int(reg.shape[1])} register tokens, the engine takes up to {MAX_REG_TOKENS}")
            w["reg"], w["prefix_tokens"] = reg, 1 + int(reg.shape[1])
        if _infer_no_embed_class(w, config, meta):
            w["no_embed_class"] = True
        i = 0
        while has(f"blocks.{i}.norm1.weight"):
            p = f"blocks.{i}."
            w[f"ln1_g.{i}"], w[f"ln1_b.{i}"] = f(p + "norm1.weight"), f(p + "norm1.bias")
            if has(p + "attn.qkv.weight"):
                w[f"qkv_w.{i}"], w[f"qkv_b.{i}"] = f(p + "attn.qkv.weight"), opt(p + "attn.qkv.bias", 3 * dim)
                w[f"proj_w.{i}"], w[f"proj_b.{i}"] = f(p + "attn.proj.weight"), opt(p + "attn.proj.bias", dim)
            else:
                absent.add(i)
            w[f"ln2_g.{i}"], w[f"ln2_b.{i}"] = f(p + "norm2.weight"), f(p + "norm2.bias")
            w[f"fc1_w.{i}"], w[f"fc1_b.{i}"] = f(p + "mlp.fc1.weight"), f(p + "mlp.fc1.bias")
            w[f"fc2_w.{i}"], w[f"fc2_b.{i}"] = f(p + "mlp.fc2.weight"), f(p + "mlp.fc2.bias")
            for name in ("ls1", "ls2"):                                  # LayerScale (a state dict cannot say `inplace`: that is a module attribute)
                if has(p + name + ".gamma"):
                    gamma = f(p + name + ".gamma")
                    if gamma.dim() != 1 or int(gamma.numel()) != dim:
                        raise ValueError(f"{p}{name}.gamma: shape {tuple(gamma.shape)} is not [{dim}]")
                    w[f"{name}.{i}"] = gamma
            i += 1
        w["lnf_g"], w["lnf_b"] = f("norm.weight"), f("norm.bias")
        if not has("head.weight"):
            raise AttributeError("Unsupported ViT checkpoint: no classification head (head.weight) — the search evaluates top-1")
        w["head_w"], w["head_b"] = f("head.weight"), opt("head.bias", int(sd["head.weight"].shape[0]))
        if has("head_dist.weight"):
            if not has("dist_token"):
                raise ValueError("head_dist: a distillation head without a dist_token")
            w["head_dist_w"], w["head_dist_b"] = f("head_dist.weight"), opt("head_dist.bias", int(sd["head_dist.weight"].shape[0]))
        eps = float(config.get("layer_norm_eps", meta.get("layer_norm_eps", 1e-6)))
    else:
        pre = next((p for p in ("vit.", "deit.") if any(k.startswith(p) for k in sd)), "")
        emb = pre + "embeddings."
        if not has(emb + "patch_embeddings.projection.weight"):
            raise AttributeError("Unsupported ViT checkpoint: neither timm (patch_embed.proj) nor HF (embeddings.patch_embeddings) keys")
        if has(emb + "register_tokens"):
            raise ValueError("register_tokens: register tokens are not supported")
        w["patch_w"], w["patch_b"] = f(emb + "patch_embeddings.projection.weight"), f(emb + "patch_embeddings.projection.bias")
        w["cls"], w["pos"] = f(emb + "cls_token"), f(emb + "position_embeddings")
        if has(emb + "distillation_token"):                              # DeiT: CLS + DIST
            w["dist"], w["prefix_tokens"] = f(emb + "distillation_token"), 2
        dim = int(w["patch_w"].shape[0])
        if has(pre + "encoder.layer.0.layernorm_before.weight"):        # ---- transformers < 5
            layout, base = "hf", pre + "encoder.layer."
        else:                                                           # ---- transformers >= 5
            layout = "hf5"
            base = pre + ("layers." if has(pre + "layers.0.layernorm_before.weight") else "encoder.layers.")
        i = 0
        while has(f"{base}{i}.layernorm_before.weight"):
            p = f"{base}{i}."
            w[f"ln1_g.{i}"], w[f"ln1_b.{i}"] = f(p + "layernorm_before.weight"), f(p + "layernorm_before.bias")
            if layout == "hf":
                q, k_, v, o = (p + "attention.attention.query", p + "attention.attention.key", p + "attention.attention.value",
                               p + "attention.output.dense")
                fc1, fc2 = p + "intermediate.dense", p + "output.dense"
            else:
                q, k_, v, o = p + "attention.q_proj", p + "attention.k_proj", p + "attention.v_proj", p + "attention.o_proj"
                fc1, fc2 = p + "mlp.fc1", p + "mlp.fc2"
            if has(q + ".weight"):
                w[f"qkv_w.{i}"] = torch.cat([f(q + ".weight"), f(k_ + ".weight"), f(v + ".weight")], 0)
                w[f"qkv_b.{i}"] = torch.cat([opt(q + ".bias", dim), opt(k_ + ".bias", dim), opt(v + ".bias", dim)], 0)
                w[f"proj_w.{i}"], w[f"proj_b.{i}"] = f(o + ".weight"), opt(o + ".bias", dim)
            else:
                absent.add(i)
            w[f"ln2_g.{i}"], w[f"ln2_b.{i}"] = f(p + "layernorm_after.weight"), f(p + "layernorm_after.bias")
            w[f"fc1_w.{i}"], w[f"fc1_b.{i}"] = f(fc1 + ".weight"), f(fc1 + ".bias")
            w[f"fc2_w.{i}"], w[f"fc2_b.{i}"] = f(fc2 + ".weight"), f(fc2 + ".bias")
            i += 1
        w["lnf_g"], w["lnf_b"] = f(pre + "layernorm.weight"), f(pre + "layernorm.bias")
        if has("cls_classifier.weight") and has("distillation_classifier.weight"):      # DeiTForImageClassificationWithTeacher
            w["head_w"], w["head_b"] = f("cls_classifier.weight"), opt("cls_classifier.bias", int(sd["cls_classifier.weight"].shape[0]))
            w["head_dist_w"] = f("distillation_classifier.weight")
            w["head_dist_b"] = opt("distillation_classifier.bias", int(sd["distillation_classifier.weight"].shape[0]))
        elif not has("classifier.weight"):
            raise AttributeError("Unsupported ViT checkpoint: no classification head (classifier.weight; a bare ViTModel?) — the search evaluates top-1")
        else:
            w["head_w"], w["head_b"] = f("classifier.weight"), opt("classifier.bias", int(sd["classifier.weight"].shape[0]))
        if "head_dist_w" in w and "dist" not in w:
            raise ValueError("distillation_classifier: a distillation head without a distillation_token")
        eps = float(config.get("layer_norm_eps", meta.get("layer_norm_eps", 1e-12)))
    depth = i
    if depth == 0:
        raise AttributeError("Unsupported ViT checkpoint: no encoder blocks found")
    heads = config.get("num_attention_heads", meta.get("num_attention_heads"))
    if heads is None:
        heads = _KNOWN_HEADS.get(dim)
    if heads is None:
        raise AttributeError(f"cannot determine the number of attention heads for hidden size {dim}: give config.json "
                             "(num_attention_heads) or --heads")
    for b in range(depth):
        if b in absent:
            w[f"attn_absent.{b}"] = True
            w[f"qkv_w.{b}"] = torch.zeros(3 * dim, dim); w[f"qkv_b.{b}"] = torch.zeros(3 * dim)
            w[f"proj_w.{b}"] = torch.zeros(dim, dim); w[f"proj_b.{b}"] = torch.zeros(dim)
    patch = int(w["patch_w"].shape[-1])
    side = _side_of(w)
    w.update(img=side * patch, patch=patch, dim=dim, heads=int(heads), depth=depth, classes=int(w["head_w"].shape[0]),
             eps=eps, layout=layout)
    # A checkpoint this build exported says where it came from (pruning_meta.json): an HF-origin model re-saved in the timm key
    # layout keeps its hook site (post-GELU, reference src/vit_pruning.py:130 vs :135) and its LayerNorm eps across the round trip
    if meta.get("score_site") in ("pre_gelu", "post_gelu"):
        w["score_site"] = meta["score_site"]
    if meta.get("origin_layout"):
        w["origin_layout"] = meta["origin_layout"]
    return w


def _infer_no_embed_class(w: Dict, config: Dict, meta: Dict) -> bool:
    """A timm state dict cannot say `no_embed_class`; the row count of pos_embed can: class-free when `rows` is a square number of
    patches, with the prefix rows when `rows - prefix` is one.  Where both hold (toy sizes: 9 rows with four registers, 25 with
    eight) `no_embed_class` or the image size (`img_size` / `image_size`) of `config` / `meta` decides; without them the dictionary
    is refused, naming both readings.  A distillation token rules the class-free reading out."""
    prefix = int(w.get("prefix_tokens", 1))
    rows = int(w["pos"].shape[1])
    patch = int(w["patch_w"].shape[-1])
    sq = lambda n: n >= 1 and int(round(math.sqrt(n))) ** 2 == n
    free, full = sq(rows) and "dist" not in w, sq(rows - prefix)
    for src in (config, meta):
        if src.get("no_embed_class") is not None:
            want = bool(src["no_embed_class"])
            if not (free if want else full):
                raise ValueError(f"pos_embed: {rows} rows do not fit no_embed_class={want} with {prefix} prefix token(s)")
            return want
    for src in (config, meta):
        img = src.get("img_size", src.get("image_size"))
        if isinstance(img, (list, tuple)):
            img = img[0]
        if img is not None:
            patches = (int(img) // patch) ** 2
            if rows == patches and free:
                return True
            if rows == patches + prefix and full:
                return False
            raise ValueError(f"pos_embed: {rows} rows fit neither {patches} patches (no_embed_class) nor {patches} + {prefix} prefix "
                             f"token(s) at an image size of {int(img)}")
    if free and full:
        raise ValueError(f"pos_embed: {rows} rows read both as {rows} patches without the prefix tokens' rows (no_embed_class) and as "
                         f"{rows - prefix} patches + {prefix} prefix token(s); give config img_size / image_size or no_embed_class")
    return free and not full         # (neither: _side_of refuses the count by name)


def load_checkpoint(path: str, heads: Optional[int] = None) -> Dict:
    """CLI `--weights`: a LOCAL checkpoint -> the flat dictionary.  Accepted: a `.safetensors` file, a `.pth` / `.pt` /
    `.bin` state dict (loaded with `weights_only=True`: nothing in the file is executed), or a directory holding
    `model.safetensors` / `pytorch_model.bin` / `timm_model.pth` with an optional `config.json` and this build's
    `pruning_meta.json` — i.e. an HF `save_pretrained` directory, or what `ssp2vit.export` writes.  No network access."""
    import json
    import os
    config, meta = {}, {}
    file = path
    if os.path.isdir(path):
        for name in ("model.safetensors", "pytorch_model.bin", "timm_model.pth"):
            if os.path.exists(os.path.join(path, name)):
                file = os.path.join(path, name)
                break
        else:
            raise FileNotFoundError(f"{path}: no model.safetensors / pytorch_model.bin / timm_model.pth inside")
        for name, dst in (("config.json", config), ("pruning_meta.json", meta)):
            p = os.path.join(path, name)
            if os.path.exists(p):
                with open(p, encoding="utf-8") as fh:
                    dst.update(json.load(fh))
    if file.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(file)
    else:
        sd = torch.load(file, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
            sd = sd["state_dict"]
    if heads is not None:
        config["num_attention_heads"] = int(heads)
    return from_state_dict(sd, config, meta)
