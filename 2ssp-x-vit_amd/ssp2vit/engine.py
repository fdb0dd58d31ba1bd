"""VitEngine: thin object wrapper over the C ABI.  PyTorch is used here only as plumbing — device buffers,
the current HIP stream, and (elsewhere) torch.distributed; every arithmetic step of the hot path runs in
libssp2vit's HIP kernels.  There is no CPU path: constructing an engine without a GPU raises."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, weights as _weights
from ._lib import EXT_OPTIONS, K_CLASS, OPTIONS, SCORE_CHAIN, SCORE_SITE, T_KINDS, Ssp2Error, TokenLayout, VitDesc, VitExt, check


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def ssp2_rows(n: int, tokens: int, group: int = 0) -> int:
    """Token-matrix rows of n images in the slab layout of `group` images per slab (csrc/engine.hip make_rowmap / total_rows)."""
    if group <= 0 or group >= n:
        return n * tokens
    mpad = -(-group * tokens // _lib.SLAB_ALIGN) * _lib.SLAB_ALIGN
    full, rest = divmod(n, group)
    return full * mpad + rest * tokens if rest else (full - 1) * mpad + group * tokens


class VitEngine:
    def _check(self, rc: int) -> None:
        check(rc, self.lib)

    def __init__(self, weights: Optional[Dict], device: str | torch.device = "cuda:0", max_images: int = 64, *,
                 precision: str = "bf16", lib_variant: Optional[str] = None, attn_stream: Optional[int] = None,
                 stream_fp8: Optional[bool] = None, _twin_of: Optional["VitEngine"] = None, _d_int: Optional[Sequence[int]] = None):
        """`lib_variant`: a named build of the library instead of the product one — "lab" carries the opt-in kernel forms the product
        does not instantiate (options ln_fusion / defer_resid / group256; ssp2vit/_lib.py VARIANT_FLAGS).
        `attn_stream`: SSP2_OPT_ATTN_STREAM in force when the engine is created (None: the environment's SSP2_ATTN_STREAM, default 0).
        0 = resident attention kernels only (d_h = 64 up to 288 tokens); 1 = longer d_h = 64 sequences (384-pixel /16: 577 tokens,
        224-pixel /8: 785) on the key-streaming kernel; 2 = every d_h = 64 attention streams (cross-checks).  A twin inherits it.
        `stream_fp8`: SSP2_OPT_STREAM_FP8, set before the precision is (None: the environment's SSP2_STREAM_FP8, default off).  True lets
        an engine on the key-streaming attention run precision="fp8": its attention writes e4m3 for the e4m3 out-projection, as the
        persistent kernels do (set_option("fp8_proj", 0) keeps both on bf16).  A twin inherits it.
        Token layout: `weights["prefix_tokens"]` (default 1; 2 = CLS + distillation token, DeiT) and a distillation head when the
        dictionary has `head_dist_w` (logits = mean of the CLS and DIST heads) go to ssp2_create_ext; a twin inherits them too.
        Register tokens (`weights["reg"]`, [1, R, dim] with prefix_tokens = 1 + R, R <= 8) and class-free positions
        (`weights["no_embed_class"]`: `pos` has the patches' rows only, the prefix tokens get no position row) go to ssp2_create_layout
        and ssp2_set_reg_tokens; the head reads CLS; a twin and a derived engine inherit the layout.
        LayerScale: `weights["ls1.i"]` / `weights["ls2.i"]` (fp32 [dim]: timm Block.ls1 / ls2 gamma) scale block i's attention / MLP
        branch before the residual add (ssp2_set_layer_scale); a block without the key runs the plain residual epilogue.  The lab
        build's options ln_fusion / defer_resid are not extended to such a branch: it takes the product kernel form."""
        if precision not in ("bf16", "fp8"):
            raise ValueError(f"precision must be 'bf16' or 'fp8', got {precision!r}")
        if attn_stream is not None and (isinstance(attn_stream, bool) or attn_stream not in (0, 1, 2)):
            raise ValueError(f"attn_stream must be None, 0, 1 or 2, got {attn_stream!r}")
        if stream_fp8 is not None and not isinstance(stream_fp8, bool):
            raise ValueError(f"stream_fp8 must be None, False or True, got {stream_fp8!r}")
        self.precision = precision
        if _twin_of is not None:          # same architecture, other FFN widths, weights cloned on the device
            src = _twin_of
            attn_stream = src.attn_stream
            stream_fp8 = bool(src.stream_fp8)
            weights = dict(depth=src.depth, dim=src.dim, classes=src.classes, img=src.img, patch=src.patch, heads=src.heads,
                           eps=src.eps, prefix_tokens=src.prefix_tokens, dist_head=src.dist_head, _layer_scale=src.layer_scale,
                           _reg_tokens=src.reg_tokens, no_embed_class=src.no_embed_class,
                           **{f"fc1_w.{i}": torch.empty(int(d), 0) for i, d in enumerate(_d_int)})
            device = src.device
        if not torch.cuda.is_available():
            raise Ssp2Error("ssp2vit needs an MI355X (HIP device): there is no CPU fallback in the product path")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise Ssp2Error(f"ssp2vit runs on HIP devices only, got device={device!r}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib_variant = lib_variant if _twin_of is None else _twin_of.lib_variant
        self.lib = _lib.load(variant=self.lib_variant)
        self.depth = int(weights["depth"])
        self.dim = int(weights["dim"])
        self.classes = int(weights["classes"])
        self.img = int(weights["img"])
        self.patch, self.heads, self.eps = int(weights["patch"]), int(weights["heads"]), float(weights.get("eps", 1e-6))
        self.prefix_tokens = int(weights.get("prefix_tokens", 1))
        self.dist_head = int(weights.get("dist_head", "head_dist_w" in weights))
        self.reg_tokens, self.no_embed_class = self._position_layout_of(weights)
        if self.reg_tokens and self.prefix_tokens != 1 + self.reg_tokens:
            raise ValueError(f"prefix_tokens={self.prefix_tokens}: CLS + {self.reg_tokens} register token(s) (reg) are {1 + self.reg_tokens}")
        if _twin_of is None and (self.reg_tokens or self.no_embed_class):
            _weights.check_flat_layout(weights)                  # pos rows against img / patch, no distillation token beside registers
        self.d_int = [int(weights[f"fc1_w.{i}"].shape[0]) for i in range(self.depth)]
        self.layer_scale = self._layer_scale_of(weights, self.depth, self.dim)      # per block: (ls1 present, ls2 present)
        self.score_ld = max((d + 63) // 64 * 64 for d in self.d_int)
        self.max_images = int(max_images)
        self.absent = [bool(weights.get(f"attn_absent.{i}", False)) for i in range(self.depth)]
        arr = (C.c_int32 * self.depth)(*self.d_int)
        desc = VitDesc(self.img, int(weights["patch"]), self.dim, int(weights["heads"]), self.depth, self.classes,
                       float(weights.get("eps", 1e-6)), self.max_images, arr)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            opts = (C.c_int32 * _lib.OPT_COUNT)(*([-1] * _lib.OPT_COUNT))
            if attn_stream is not None:
                opts[OPTIONS["attn_stream"]] = int(attn_stream)
            if self.reg_tokens or self.no_embed_class:
                lay = TokenLayout(self.prefix_tokens, self.dist_head, self.reg_tokens, 0 if self.no_embed_class else 1)
                self._check(self.lib.ssp2_create_layout(C.byref(desc), opts, C.byref(lay), C.byref(h)))
            elif self.prefix_tokens == 1 and not self.dist_head:
                self._check(self.lib.ssp2_create_opts(C.byref(desc), opts, C.byref(h)))
            else:
                ext = VitExt(self.prefix_tokens, self.dist_head)
                self._check(self.lib.ssp2_create_ext(C.byref(desc), opts, C.byref(ext), C.byref(h)))
            self.h = h
            self.tokens = self.lib.ssp2_tokens(self.h)
            self.attn_stream = self.get_option("attn_stream")
            if stream_fp8 is not None:
                self.set_option("stream_fp8", int(stream_fp8))
            self.stream_fp8 = self.get_option("stream_fp8")
            if _twin_of is None:
                self._load(weights)
                if precision == "fp8":
                    self._bind_stream()
                    self._check(self.lib.ssp2_set_precision(self.h, 1))
            else:
                self._bind_stream()
                self._check(self.lib.ssp2_clone_weights(self.h, _twin_of.h))
                self.absent = list(_twin_of.absent)

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _layer_scale_of(w: Dict, depth: int, dim: int) -> Tuple[Tuple[bool, bool], ...]:
        """Which residual branches of `w` carry a LayerScale (`ls1.i` / `ls2.i`); a gamma that is not [dim] is refused by name."""
        if "_layer_scale" in w:
            return tuple(w["_layer_scale"])
        for i in range(depth):
            for k in (f"ls1.{i}", f"ls2.{i}"):
                if k in w and int(w[k].numel()) != dim:
                    raise ValueError(f"{k}: a LayerScale gamma of {int(w[k].numel())} values on a hidden size of {dim}")
        return tuple((f"ls1.{i}" in w, f"ls2.{i}" in w) for i in range(depth))

    @staticmethod
    def _position_layout_of(w: Dict) -> Tuple[int, bool]:
        """(register tokens, class-free positions) of `w`: rows of `reg` ([1, R, dim]) and `no_embed_class`."""
        if "_reg_tokens" in w:
            return int(w["_reg_tokens"]), bool(w.get("no_embed_class", False))
        reg = w.get("reg")
        if reg is not None and (reg.dim() != 3 or int(reg.shape[0]) != 1 or int(reg.shape[2]) != int(w["dim"])):
            raise ValueError(f"reg: shape {tuple(reg.shape)} is not [1, R, {int(w['dim'])}]")
        return (int(reg.shape[1]) if reg is not None else 0), bool(w.get("no_embed_class", False))

    def _load(self, w: Dict) -> None:
        """fp32 tensors in nn.Linear layout -> the engine's bf16 / padded weight image.  The rounding and the padding run
        in a kernel; a tensor that already lives on this GPU (a module moved to the device, as the reference keeps it)
        is read in place, a host tensor costs one copy of its fp32 bytes."""
        self._bind_stream()
        keep, batch = [], []                                     # device tensors: alive until the stream has consumed them; (kind, layer, tensor)

        def put(kind: str, layer: int, t: torch.Tensor):
            t = t.detach()
            if t.device == self.device:
                t = t.to(torch.float32).contiguous()
                keep.append(t)
                batch.append((T_KINDS.index(kind), layer, t))
            else:
                t = t.to("cpu", torch.float32).contiguous()
                self._check(self.lib.ssp2_load_tensor(self.h, T_KINDS.index(kind), layer,
                                                C.cast(t.data_ptr(), C.POINTER(C.c_float)), t.numel()))
        for k in ("patch_w", "patch_b", "cls", "pos", "lnf_g", "lnf_b", "head_w", "head_b"):
            put(k, 0, w[k])
        if self.prefix_tokens == 2 and not self.reg_tokens:
            put("dist", 0, w["dist"])
        if self.dist_head:
            put("head_dist_w", 0, w["head_dist_w"]); put("head_dist_b", 0, w["head_dist_b"])
        for i in range(self.depth):
            for k in ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_g", "ln2_b",
                      "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
                put(k, i, w[f"{k}.{i}"])
        if batch:
            # a live module's ~150 tensors in ceil(count / 64) launches (ssp2_load_tensors_dev, ABI 5) instead of one launch each: 1.5 ms of
            # launches for 0.1 ms of traffic inside the caller's prune bracket (scripts/api_profile.py)
            m = len(batch)
            kinds = (C.c_int * m)(*[b[0] for b in batch])
            layers = (C.c_int * m)(*[b[1] for b in batch])
            ptrs = (C.c_void_p * m)(*[b[2].data_ptr() for b in batch])
            numels = (C.c_size_t * m)(*[b[2].numel() for b in batch])
            self._check(self.lib.ssp2_load_tensors_dev(self.h, m, kinds, layers, ptrs, numels))
        if self.reg_tokens:                                      # register tokens: fp32 as they are, one small copy (no tensor kind: the kinds' order is pinned)
            t = w["reg"].detach()
            on_dev = t.device == self.device
            t = (t if on_dev else t.to("cpu")).to(torch.float32).contiguous().view(-1)
            keep.append(t)
            self._check(self.lib.ssp2_set_reg_tokens(self.h, _ptr(t), self.reg_tokens, int(on_dev)))
        # LayerScale: fp32 as it is, one small copy per branch (no tensor kind of the batched ingest: the kinds' order is pinned)
        for i, has in enumerate(self.layer_scale):
            for br in (0, 1):
                if has[br]:
                    t = w[f"ls{br + 1}.{i}"].detach()
                    on_dev = t.device == self.device
                    t = (t if on_dev else t.to("cpu")).to(torch.float32).contiguous().view(-1)
                    keep.append(t)
                    self._check(self.lib.ssp2_set_layer_scale(self.h, i, br, _ptr(t), int(on_dev)))
        if keep:
            torch.cuda.current_stream(self.device).synchronize()

    def geometry_key(self):
        """What two engines must share for one to take over the other's handle (workspace, weight storage): see `reload`."""
        return (str(self.device), self.precision, self.lib_variant, self.img, self.patch, self.dim, self.heads, self.depth, self.classes,
                float(self.eps), tuple(int(d) for d in self.d_int), self.prefix_tokens, self.dist_head, self.layer_scale,
                self.reg_tokens, self.no_embed_class)

    def reload(self, weights: Dict) -> "VitEngine":
        """Another model of the SAME geometry into this engine: every tensor is ingested again (device-to-device rounding kernels), the
        attention flags are reset to the new model's — handle, weight storage and the (already touched) activation workspace stay.
        What vit_pruning's engine pool does when a sweep builds a fresh module per target: a fresh engine costs its build (2.6 ms for
        the 13 GB layer-major workspace of ViT-B/16) plus ~3 ms of first use of fresh memory, per prune (profiles/r05_m_api_profile.txt)."""
        if self.precision != "bf16":
            raise Ssp2Error("reload: bf16 engines only (an fp8 engine carries quantised weight images and calibrated scales)")
        if [int(weights[f"fc1_w.{i}"].shape[0]) for i in range(self.depth)] != [int(d) for d in self.d_int]:
            raise Ssp2Error("reload: FFN widths differ")
        if (int(weights.get("prefix_tokens", 1)), int(weights.get("dist_head", "head_dist_w" in weights))) != (self.prefix_tokens, self.dist_head):
            raise Ssp2Error("reload: token layouts differ (prefix tokens / distillation head)")
        if self._position_layout_of(weights) != (self.reg_tokens, self.no_embed_class):
            raise Ssp2Error("reload: token layouts differ (register tokens / class-free positions)")
        if self.reg_tokens or self.no_embed_class:
            _weights.check_flat_layout(weights)
        if self._layer_scale_of(weights, self.depth, self.dim) != self.layer_scale:
            raise Ssp2Error("reload: LayerScale differs (which residual branches carry a gamma)")
        with torch.cuda.device(self.device):
            self._load(weights)
            for l in range(self.depth):
                gone = bool(weights.get(f"attn_absent.{l}", False))
                self._check((self.lib.ssp2_drop_attention if gone else self.lib.ssp2_restore_attention)(self.h, l))
                self.absent[l] = gone
        return self

    def close(self) -> None:
        if getattr(self, "h", None):
            if getattr(self, "precision", "bf16") == "fp8":
                try:                                              # an fp8 engine that clipped attention outputs says so when it goes away
                    n = self.fp8_saturation()
                    if n > 0:
                        import warnings
                        warnings.warn(f"ssp2vit fp8 engine: {n} wave(s) clipped attention outputs at the e4m3 range of their hand-off scale "
                                      "(|o| > 28 uncalibrated); use calibrate_fp8(...), set_option('fp8_proj', 0) or precision='bf16' for this "
                                      "checkpoint", RuntimeWarning, stacklevel=2)
                except Exception:
                    pass
            self.lib.ssp2_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ applying a prune on the device (f2)
    def prune_ffn(self, layer: int, keep: Sequence[int]) -> None:
        """Keep only the FFN neurons `keep` (ascending) of block `layer`: fc1 rows / bias and fc2 columns are gathered
        in HBM (reference src/vit_pruning.py:297-311 on the module).  No re-upload of weights."""
        arr = (C.c_int32 * len(keep))(*[int(k) for k in keep])
        with torch.cuda.device(self.device):
            self._check(self.lib.ssp2_prune_ffn(self.h, int(layer), arr, len(keep)))
        self.d_int[layer] = len(keep)

    def apply_ffn_masks(self, masks: Sequence[Sequence[int]]) -> None:
        """masks[l][j] == 1 -> prune neuron j of block l (the `ffn_prune_masks` of prune_vit_mlp_width)."""
        for l, m in enumerate(masks):
            keep = [j for j, bit in enumerate(m) if not bit]
            if len(keep) != self.d_int[l]:
                self.prune_ffn(l, keep)

    def drop_attention(self, layers: Sequence[int]) -> None:
        for l in layers:
            self._check(self.lib.ssp2_drop_attention(self.h, int(l)))
            self.absent[int(l)] = True

    def set_cu_limit(self, n_cu: int) -> None:
        """Cap the grids of this engine's persistent kernels at n_cu workgroups (0 = all CUs)."""
        self._check(self.lib.ssp2_set_cu_limit(self.h, int(n_cu)))

    def set_option(self, name: str, value: int) -> None:
        """Run-time switch of this engine (include/ssp2vit.h SSP2_OPT_*: "zigzag", "attn_persist", "ln_fusion", "big_tiles",
        "fc1_big_tiles", "group256", ...; and the extended ones of _lib.EXT_OPTIONS: "stream_fp8").  None of them changes a result
        bit of a bf16 engine; they exist for the tests and A/B scripts that prove it."""
        self._check(self.lib.ssp2_set_option(self.h, self._option_index(name), int(value)))
        if name == "stream_fp8":
            self.stream_fp8 = int(value)

    @staticmethod
    def _option_index(name: str) -> int:
        return OPTIONS[name] if name in OPTIONS else EXT_OPTIONS[name]

    def get_option(self, name: str) -> int:
        v = self.lib.ssp2_get_option(self.h, self._option_index(name))
        if v < 0:
            self._check(v)
        return int(v)

    def calibrate_fp8(self, pixels: torch.Tensor, headroom: float = 4.0) -> List[float]:
        """fp8 mode: measure the attention outputs of `pixels` (one or more chunks of <= max_images images, each launch >= 4096 token
        rows) with the out-projection on bf16 and set every block's hand-off scale to the largest power of two that keeps
        max|o| x headroom inside the e4m3 range (ssp2_fp8_calibrate_*).  Explicit and deterministic: only these images count.
        Returns the scales in force afterwards, one per block (16.0 = the uncalibrated default)."""
        if self.precision != "fp8":
            raise Ssp2Error("calibrate_fp8 needs precision='fp8'")
        self._bind_stream()
        self._check(self.lib.ssp2_fp8_calibrate_begin(self.h))
        try:
            for s0 in range(0, pixels.shape[0], self.max_images):      # EVERY block through the full path (forward_logits ends in the CLS-only tail)
                chunk = pixels[s0:s0 + self.max_images]
                x = self.embed(chunk)
                self.layers(x, chunk.shape[0], 0, self.depth)
        finally:
            self._check(self.lib.ssp2_fp8_calibrate_end(self.h, float(headroom)))
        top = self.fp8_fc2_top_codes()
        if top > 0:
            import warnings
            warnings.warn(f"ssp2vit fp8 calibration: {top} FFN activation value(s) of the calibration images sit on the e4m3 top code (|GELU output| >= 448): "
                          "the fc1 -> fc2 hand-off of this checkpoint clips in fp8 mode; use precision='bf16'", RuntimeWarning, stacklevel=2)
        return [float(self.lib.ssp2_fp8_attn_scale(self.h, l)) for l in range(self.depth)]

    def fp8_fc2_top_codes(self) -> int:
        """fp8 mode: how many e4m3 bytes of the fc1 -> fc2 hand-off the LAST calibration pass (calibrate_fp8) found on the top code +-448 — GELU
        outputs at or beyond the e4m3 range, which the saturating cast clips (SSP2_Q_FP8_FC2_TOP_CODES).  0: that hand-off is safe on those images."""
        v = self.lib.ssp2_query(self.h, 9)
        if v < 0:
            self._check(v)
        return int(v)

    def fp8_saturation(self, reset: bool = False) -> int:
        """fp8 mode: how many waves have CLIPPED a value when the attention output was handed to the out-projection as e4m3(o x 16)
        (|o| > 28) since the engine was built / the counter was reset.  0 for a model whose attention outputs stay in range; > 0
        says this checkpoint wants `set_option("fp8_proj", 0)` or bf16.  Waits for the stream."""
        v = self.lib.ssp2_query(self.h, 8 if reset else 7)            # SSP2_Q_FP8_SATURATED_RESET / SSP2_Q_FP8_SATURATED
        if v < 0:
            self._check(v)
        return int(v)

    def pruned_twin(self, d_int: Sequence[int], max_images: int = 64) -> "VitEngine":
        """A second engine of the same architecture with FFN widths `d_int`, every other weight cloned device to
        device: the container `apply_into` fills.  Built once (outside a timed region); a prune then costs gathers only."""
        return VitEngine(None, max_images=max_images, _twin_of=self, _d_int=list(d_int))

    def apply_into(self, twin: "VitEngine", masks: Sequence[Sequence[int]], drop_blocks: Sequence[int]) -> "VitEngine":
        """Stage-1 + stage-2 APPLY (reference src/vit_pruning.py:297-311 and :499-504) into `twin`, leaving this dense
        engine untouched: kept FFN neurons of every block are gathered in HBM, the chosen blocks lose their attention.
        Asynchronous on the current stream.  masks[l][j] == 1 -> neuron j of block l is pruned."""
        self.apply_ffn_into(twin, masks)
        return self.apply_attention_into(twin, drop_blocks)

    def apply_ffn_into(self, twin: "VitEngine", masks: Sequence[Sequence[int]]) -> "VitEngine":
        """The width half of `apply_into` (a8): the gathers are ENQUEUED on the current stream and do not depend on the depth search, so
        a caller that has the masks before the search has finished can queue them behind it and spare the GPU the host's latency
        at the end of the prune (bench.py does)."""
        twin._bind_stream()
        for l, m in enumerate(masks):
            keep = m if isinstance(m, torch.Tensor) else torch.as_tensor(m)
            keep = torch.nonzero(keep == 0).view(-1).to(torch.int32).contiguous()
            self._check(self.lib.ssp2_prune_ffn_into(twin.h, self.h, l, C.cast(keep.data_ptr(), C.POINTER(C.c_int32)), keep.numel()))
        return twin

    def apply_attention_into(self, twin: "VitEngine", drop_blocks: Sequence[int]) -> "VitEngine":
        """The depth half (a9): host-side flags only, no device work."""
        drop = set(int(b) for b in drop_blocks)
        for l in range(self.depth):
            if l in drop or self.absent[l]:
                self._check(self.lib.ssp2_drop_attention(twin.h, l)); twin.absent[l] = True
            else:
                self._check(self.lib.ssp2_restore_attention(twin.h, l)); twin.absent[l] = False
        return twin

    # ------------------------------------------------------------------ plumbing
    def _bind_stream(self) -> None:
        self._check(self.lib.ssp2_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _skip_array(self, attn_skip: Optional[Sequence[int]]):
        flags = [1 if a else 0 for a in self.absent]
        if attn_skip is not None:
            for i in attn_skip:
                flags[int(i)] = 1
        if not any(flags):
            return None
        return (C.c_uint8 * self.depth)(*flags)

    def rows(self, n: int, group: int = 0) -> int:
        return int(self.lib.ssp2_rows(self.h, n, int(group)))

    def new_x(self, n: int, group: int = 0) -> torch.Tensor:
        return torch.empty(self.rows(n, group), self.dim, dtype=torch.float32, device=self.device)

    def new_scores(self, groups: int = 1) -> torch.Tensor:
        return torch.zeros(groups, self.depth, self.score_ld, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ the four device entry points
    batch_lists = True          # embed / forward_scores take a LIST of batches: each lands in its rows of x, nothing is concatenated
    prefix_scoring = True       # layers(score_images=...) / tail(group=...): the search's baseline can carry the stage-1 hook (core.prune_pass)

    def embed(self, pixels, x: Optional[torch.Tensor] = None, group: int = 0) -> torch.Tensor:
        if isinstance(pixels, (list, tuple)):
            # several dataloader batches -> one token matrix, each batch embedded straight into its rows (round 2 built one
            # pixel tensor with torch.cat first: 308 MB copied per 512-image stage-1 launch).  Slab layout (group > 0): batch
            # b is slab b and must hold `group` images, except the last; contiguous layout: batches back to back.
            n = sum(int(p.shape[0]) for p in pixels)
            x = self.new_x(n, group) if x is None else x
            if group > 0 and group < n:
                mpad = -(-group * self.tokens // _lib.SLAB_ALIGN) * _lib.SLAB_ALIGN
                pad = mpad - group * self.tokens
                if pad:                                    # pad rows between slabs: finite values (they flow through LN / GEMMs)
                    x[: (len(pixels) - 1) * mpad].view(len(pixels) - 1, mpad, self.dim)[:, group * self.tokens:, :].zero_()
                for b, p in enumerate(pixels):
                    if int(p.shape[0]) != group and b != len(pixels) - 1:
                        raise ValueError("slab layout: every batch but the last must hold `group` images")
                    self.embed(p, x=x[b * mpad:], group=0)
            else:
                row = 0
                for p in pixels:
                    self.embed(p, x=x[row:], group=0)
                    row += int(p.shape[0]) * self.tokens
            return x
        if pixels.dim() != 4 or pixels.shape[1] != 3 or pixels.shape[2] != self.img or pixels.shape[3] != self.img:
            raise ValueError(f"pixel_values must be [n,3,{self.img},{self.img}], got {tuple(pixels.shape)}")
        px = pixels.to(self.device, torch.float32, non_blocking=True).contiguous()
        n = px.shape[0]
        x = self.new_x(n, group) if x is None else x
        self._bind_stream()
        self._check(self.lib.ssp2_embed(self.h, _ptr(px), n, _ptr(x), int(group)))
        return x

    def layers(self, x: torch.Tensor, n: int, l_begin: int = 0, l_end: Optional[int] = None,
               attn_skip: Optional[Sequence[int]] = None, score_site: str = "none", score_chain: str = "fp32",
               batch_scores: Optional[torch.Tensor] = None, score_group: int = 0, scores_only: bool = False,
               x_in: Optional[torch.Tensor] = None, score_images: Optional[int] = None) -> Optional[torch.Tensor]:
        """Returns f32 [groups, depth, score_ld] when scoring (groups = ceil(n / score_group), 1 if score_group=0).
        `scores_only`: x is scratch afterwards — the last block stops behind its hooked activation (SSP2_SCORE_ONLY).
        `x_in`: the stream entering block l_begin is read from there and left untouched (ssp2_layers_from); x receives the result.
        `score_images`: only the leading images of the launch are hooked (whole slabs; ssp2_layers_prefix) — the search's baseline
        doubling as the stage-1 pass; groups = ceil(score_images / score_group)."""
        l_end = self.depth if l_end is None else l_end
        site = SCORE_SITE[score_site] | (0x10 if (scores_only and SCORE_SITE[score_site]) else 0)
        ns = n if score_images is None else int(score_images)
        grp = ns if (score_group <= 0 or score_group > ns) else score_group
        if site and batch_scores is None:
            batch_scores = self.new_scores((ns + grp - 1) // grp)
        self._bind_stream()
        if x_in is not None and (x_in.shape[0] < x.shape[0] or x_in.shape[1:] != x.shape[1:] or x_in.dtype != x.dtype or not x_in.is_contiguous()):
            raise ValueError("x_in must be a contiguous stream of the shape of x")
        self._check(self.lib.ssp2_layers_prefix(self.h, _ptr(x_in), _ptr(x), n, l_begin, l_end, self._skip_array(attn_skip), site,
                                          SCORE_CHAIN[score_chain], int(score_group), ns, _ptr(batch_scores if site else None), self.score_ld))
        return batch_scores if site else None

    def _logits_pred(self, n: int, want_logits: bool, want_pred: bool, logits: Optional[torch.Tensor], pred: Optional[torch.Tensor]):
        """The head's outputs: the caller's own buffers (logits f32 [>= n, classes] densely packed, pred int32 [>= n]: the kernels write
        n rows at a row stride of `classes`) or fresh ones when asked for."""
        if logits is not None and (logits.device != self.device or logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[0] < n
                                   or logits.shape[1] != self.classes or not logits.is_contiguous()):
            raise ValueError(f"logits must be a contiguous f32 device tensor of [>= {n}, {self.classes}]")
        if pred is not None and (pred.device != self.device or pred.dtype != torch.int32 or pred.dim() != 1 or pred.numel() < n
                                 or not pred.is_contiguous()):
            raise ValueError(f"pred must be a contiguous int32 device tensor of >= {n} entries")
        if logits is None and want_logits:
            logits = torch.empty(n, self.classes, dtype=torch.float32, device=self.device)
        if pred is None and want_pred:
            pred = torch.empty(n, dtype=torch.int32, device=self.device)
        return logits, pred

    def head(self, x: torch.Tensor, n: int, labels: Optional[torch.Tensor] = None,
             correct: Optional[torch.Tensor] = None, want_logits: bool = False, want_pred: bool = False, group: int = 0, *,
             logits: Optional[torch.Tensor] = None, pred: Optional[torch.Tensor] = None):
        """Final norm + classifier (+ top-1) on the prefix rows of x.  `logits` / `pred`: buffers of the caller's to write into (rows
        behind n are left alone); returned as given."""
        logits, pred = self._logits_pred(n, want_logits, want_pred, logits, pred)
        if labels is not None:
            labels = labels.to(self.device, torch.int64, non_blocking=True).contiguous()
            if correct is None:
                correct = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._bind_stream()
        self._check(self.lib.ssp2_head(self.h, _ptr(x), n, int(group), _ptr(logits), _ptr(pred), _ptr(labels),
                                 _ptr(correct if labels is not None else None)))
        return logits, pred, correct

    def tail(self, x: torch.Tensor, n: int, attn_skip: Optional[Sequence[int]] = None,
             labels: Optional[torch.Tensor] = None, correct: Optional[torch.Tensor] = None, want_logits: bool = False,
             want_pred: bool = False, slots: int = 1, group: int = 0, *, logits: Optional[torch.Tensor] = None,
             pred: Optional[torch.Tensor] = None):
        """Last encoder block + head on the CLS rows only (x must hold the residual stream ENTERING the last block;
        it is not modified).  Same results, bit for bit, as layers(x, depth-1, depth) + head(x).
        `slots` > 1: x holds that many streams of n images side by side (ssp2_tail_slots); labels [n] are shared, `correct`
        must have `slots` entries (slot s is counted in correct[s]), logits / pred cover slots * n images.
        `group` > 0: the streams are in the slab layout of `rows(slots * n, group)` (ssp2_tail_group).
        `logits` / `pred`: buffers of the caller's, as in `head`."""
        logits, pred = self._logits_pred(n * int(slots), want_logits, want_pred, logits, pred)
        if labels is not None:
            labels = labels.to(self.device, torch.int64, non_blocking=True).contiguous()
            if correct is None:
                correct = torch.zeros(int(slots), dtype=torch.int64, device=self.device)
            if correct.numel() < int(slots) or not correct.is_contiguous():
                raise ValueError("`correct` needs one contiguous int64 entry per slot")
        skip_last = bool(self.absent[self.depth - 1]) or (attn_skip is not None and (self.depth - 1) in [int(i) for i in attn_skip])
        self._bind_stream()
        self._check(self.lib.ssp2_tail_group(self.h, _ptr(x), n, int(slots), int(group), int(skip_last), _ptr(logits), _ptr(pred), _ptr(labels),
                                       _ptr(correct if labels is not None else None)))
        return logits, pred, correct

    def act_l2_accum(self, act: torch.Tensor, score_chain: str = "fp32") -> torch.Tensor:
        """Standalone hook-body kernel: act [n, tokens, d] (bf16 or f32, contiguous, d % 8 == 0) -> f32 [d]."""
        if act.dim() != 3 or not act.is_contiguous() or act.device.type != "cuda":
            raise ValueError("act must be a contiguous [n, tokens, d] device tensor")
        n, t, d = act.shape
        dtype = {torch.bfloat16: 0, torch.float32: 1}[act.dtype]
        ws = torch.empty(2, n, d, dtype=torch.float32, device=act.device)
        out = torch.empty(d, dtype=torch.float32, device=act.device)
        self._check(self.lib.ssp2_act_l2_accum(C.c_void_p(torch.cuda.current_stream(act.device).cuda_stream), _ptr(act), dtype,
                                         n, t, d, d, SCORE_CHAIN[score_chain], 0, _ptr(ws), _ptr(out), d))
        return out

    def score_finish(self, slab: torch.Tensor, n: int, tokens: int, group: int = 0, score_chain: str = "fp32", *,
                     norms: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The forward's fused score finish on a slab of the caller's (ssp2_score_finish): slab f32 [tiles, 2, ld] -> (out f32
        [ceil(n / group), out_stride] of which columns [0, ld) are written, norms f32 [n, ld]).  `norms` / `out`: the caller's buffers."""
        if slab.dim() != 3 or slab.shape[1] != 2 or slab.dtype != torch.float32 or not slab.is_contiguous() or slab.device.type != "cuda":
            raise ValueError("slab must be a contiguous f32 [tiles, 2, ld] device tensor")
        ld = int(slab.shape[2])
        rows = ssp2_rows(int(n), int(tokens), int(group))
        if int(slab.shape[0]) < 2 * (-(-rows // 256)):
            raise ValueError(f"slab holds {int(slab.shape[0])} tiles, the layout has {2 * (-(-rows // 256))}")
        grp = n if (group <= 0 or group > n) else group
        if norms is None:
            norms = torch.empty(n, ld, dtype=torch.float32, device=slab.device)
        if out is None:
            out = torch.empty(-(-n // grp), ld, dtype=torch.float32, device=slab.device)
        for name, t, r in (("norms", norms, n), ("out", out, -(-n // grp))):
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < r or t.shape[1] < ld or not t.is_contiguous() or t.device != slab.device:
                raise ValueError(f"{name} must be a contiguous f32 [>= {r}, >= {ld}] tensor on the slab's device")
        if int(norms.shape[1]) != ld:
            raise ValueError(f"norms must be [n, {ld}] densely packed")
        self._check(self.lib.ssp2_score_finish(C.c_void_p(torch.cuda.current_stream(slab.device).cuda_stream), _ptr(slab), int(n), int(tokens),
                                               int(group), ld, SCORE_CHAIN[score_chain], _ptr(norms), _ptr(out), int(out.shape[1])))
        return out, norms

    def peek_shape(self, kind: str, layer: int = 0) -> Dict[str, int]:
        """rows, cols, rows_pad, ld, ld8 of what the engine holds for tensor `kind` of block `layer` (ssp2_peek_tensor, SSP2_PEEK_SHAPE)."""
        buf = (C.c_int32 * 5)()
        self._check(self.lib.ssp2_peek_tensor(self.h, T_KINDS.index(kind), int(layer), _lib.PEEK["shape"], buf, 20))
        return dict(zip(("rows", "cols", "rows_pad", "ld", "ld8"), (int(v) for v in buf)))

    def peek_tensor(self, kind: str, layer: int = 0, image: str = "image") -> torch.Tensor:
        """What the engine holds, read back to the CPU (ssp2_peek_tensor; synchronises): image "image" -> a matrix's bf16 [rows_pad, ld],
        a bias's f32 [rows_pad], a vector's f32 [rows]; "e4m3" -> uint8 [rows_pad, ld8] and "scale" -> f32 [rows_pad] of a matrix in
        fp8 mode."""
        s = self.peek_shape(kind, layer)
        is_mat = kind.endswith("_w")
        if image == "image":
            t = torch.empty(s["rows_pad"], s["ld"], dtype=torch.bfloat16) if is_mat else torch.empty(s["rows_pad"], dtype=torch.float32)
        elif image == "e4m3":
            t = torch.empty(s["rows_pad"], s["ld8"], dtype=torch.uint8) if s["ld8"] else torch.empty(1, dtype=torch.uint8)   # (none: the library says so)
        elif image == "scale":
            t = torch.empty(s["rows_pad"], dtype=torch.float32)
        else:
            raise ValueError(f"image must be 'image', 'e4m3' or 'scale', got {image!r}")
        with torch.cuda.device(self.device):
            self._check(self.lib.ssp2_peek_tensor(self.h, T_KINDS.index(kind), int(layer), _lib.PEEK[image], C.c_void_p(t.data_ptr()),
                                                  t.numel() * t.element_size()))
        return t

    def linear(self, a: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], epilogue: str = "bf16",
               x: Optional[torch.Tensor] = None, kernel: str = "auto", *, gamma: Optional[torch.Tensor] = None,
               xin: Optional[torch.Tensor] = None, rev: int = 0) -> torch.Tensor:
        """One projection of the forward on its own (ssp2_linear_bf16): a bf16 [M, K], weight [N, K] (any float dtype,
        rounded to bf16 like autocast does), bias [N] or None.  epilogue "bf16" / "gelu" -> bf16 [M, N];
        "resid" -> x (f32 [M, N]) updated in place and returned.
        gamma (f32 [N], "resid" only): the branch's LayerScale — x = xin + fl32(gamma * bf16(...)) (ssp2_linear_ls_bf16), xin (default
        x) read at x's row stride, rev the walk direction of the 256 x 256 kernel's tiles."""
        epi = {"bf16": 0, "resid": 1, "gelu": 2}[epilogue]
        if gamma is None and (xin is not None or rev):
            raise ValueError("xin / rev belong to the LayerScale form (gamma=...)")
        if gamma is not None and epi != 1:
            raise ValueError("gamma: LayerScale goes with the resid epilogue only")
        M, K = a.shape
        N = weight.shape[0]
        npad = (N + 255) // 256 * 256
        wp = torch.zeros(npad, K, dtype=torch.bfloat16, device=self.device)
        wp[:N].copy_(weight.to(self.device, torch.bfloat16))
        bp = torch.zeros(npad, dtype=torch.float32, device=self.device)
        if bias is not None:
            bp[:N].copy_(bias.to(self.device, torch.bfloat16).float())
        a = a.to(self.device, torch.bfloat16).contiguous()
        out = None if epi == 1 else torch.empty(M, N, dtype=torch.bfloat16, device=self.device)
        if gamma is not None:
            # the LayerScale form takes x (and xin, at the same row stride) as row-major f32 [>= M, >= N]: ldx = x's row stride
            for name, t in (("x", x), ("xin", xin)):
                if (t is None and name == "x") or (t is not None and (t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 2
                                                                      or t.stride(1) != 1 or t.shape[0] < M or t.shape[1] < N)):
                    raise ValueError(f"the LayerScale form needs {name} as a row-major f32 device tensor of >= [{M}, {N}]")
            if xin is not None and xin.stride(0) != x.stride(0):
                raise ValueError("xin must have x's row stride (the kernel reads both at ldx)")
            gp = self._gamma_vec(gamma, N)
            self._check(self.lib.ssp2_linear_ls_bf16(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), _ptr(a), K, _ptr(wp), K,
                                                     _ptr(bp), _ptr(gp), M, N, K, _ptr(x), _ptr(xin), x.stride(0),
                                                     {"auto": 0, "small": 1, "big": 2}[kernel], int(rev)))
            return x
        if epi == 1 and (x is None or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[1] != N or x.shape[0] < M):
            raise ValueError("resid epilogue needs a contiguous f32 x [>= M, N]")
        self._check(self.lib.ssp2_linear_bf16(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), epi, _ptr(a), K,
                                        _ptr(wp), K, _ptr(bp), M, N, K, _ptr(out), N, _ptr(x if epi == 1 else None), N,
                                        {"auto": 0, "small": 1, "big": 2}[kernel]))
        return x if epi == 1 else out

    def linear_ex(self, a: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], epilogue: str = "bf16", *,
                  rows: Optional[int] = None, kernel: str = "auto", out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None,
                  x: Optional[torch.Tensor] = None, xin: Optional[torch.Tensor] = None, rev: int = 0, score_site: int = 0,
                  tokens: int = 0, group: int = 0, n_img: int = 0, slab_ld: Optional[int] = None):
        """`linear` on the caller's own buffers, with every form the forward's bf16 launches take (ssp2_linear_bf16_ex).  a: bf16
        row-major device tensor [>= rows, >= K] (rows = a.shape[0] by default), read at its row stride.  weight [N, K]: a bf16
        row-major device tensor is read WHERE IT IS at its row stride — the storage behind it must reach ceil256(N) rows, rows N..
        being zero (the kernels read whole column tiles); anything else is rounded to bf16 and padded like `linear` does.  bias [N] or
        None.  out / out2 (bf16) and x / xin (f32) are row-major device tensors of >= [rows, N], written / read at their row strides
        (out2 at out's, xin at x's).  epilogue "bf16" / "gelu" -> out (allocated [rows, N] when None); "gelu" with out2: the
        pre-GELU bf16 copy as well (128 x 128 kernel); "resid" -> x = xin (default x) + bf16(...), returned.  score_site 1 / 2
        ("gelu"; tokens, group, n_img: the row layout of ssp2_rows) returns (out, slab f32 [2 * ceil(rows / 256), 2, slab_ld]),
        slab_ld defaulting to N, pre-filled with NaN: entry t covers rows 128 t .. 128 t + 127.  rev: the walk direction of the tiles."""
        epi = {"bf16": 0, "resid": 1, "gelu": 2}[epilogue]
        N, K = weight.shape
        M = a.shape[0] if rows is None else int(rows)
        npad = (N + 255) // 256 * 256
        if (out2 is not None or score_site) and epi != 2:
            raise ValueError("out2 / score_site go with the gelu epilogue only")
        if (xin is not None and epi != 1) or (x is not None and epi != 1) or (out is not None and epi == 1):
            raise ValueError("x / xin go with the resid epilogue, out with the others")

        def dev2d(name, t, dtype, r, c):
            if t.device.type != "cuda" or t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < r or t.shape[1] < c:
                raise ValueError(f"{name} must be a row-major {dtype} device tensor of >= [{r}, {c}]")
        dev2d("a", a, torch.bfloat16, M, K)
        if weight.device.type == "cuda" and weight.dtype == torch.bfloat16 and weight.dim() == 2 and weight.stride(1) == 1:
            wp, ldw = weight, weight.stride(0)
            if weight.storage_offset() + (npad - 1) * ldw + K > weight.untyped_storage().nbytes() // 2:
                raise ValueError(f"the storage behind weight must hold ceil256(N) = {npad} rows (rows past N zero)")
        else:
            wp = torch.zeros(npad, K, dtype=torch.bfloat16, device=self.device)
            wp[:N].copy_(weight.to(self.device, torch.bfloat16))
            ldw = K
        bp = torch.zeros(npad, dtype=torch.float32, device=self.device)
        if bias is not None:
            bp[:N].copy_(bias.to(self.device, torch.bfloat16).float())
        slab = None
        ldo = ldx = 0
        if epi == 1:
            if x is None:
                raise ValueError("resid epilogue needs x")
            for name, t in (("x", x), ("xin", xin)):
                if t is not None:
                    dev2d(name, t, torch.float32, M, N)
            if xin is not None and xin.stride(0) != x.stride(0):
                raise ValueError("xin must have x's row stride (the kernel reads both at ldx)")
            ldx = x.stride(0)
        else:
            if out is None:
                out = torch.empty(M, N, dtype=torch.bfloat16, device=self.device)
            for name, t in (("out", out), ("out2", out2)):
                if t is not None:
                    dev2d(name, t, torch.bfloat16, M, N)
            if out2 is not None and out2.stride(0) != out.stride(0):
                raise ValueError("out2 must have out's row stride (the kernel writes both at ldo)")
            ldo = out.stride(0)
            if score_site:
                slab_ld = N if slab_ld is None else int(slab_ld)
                slab = torch.full((2 * ((M + 255) // 256), 2, slab_ld), float("nan"), dtype=torch.float32, device=self.device)
        self._check(self.lib.ssp2_linear_bf16_ex(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), epi, _ptr(a), a.stride(0),
                                                 _ptr(wp), ldw, _ptr(bp), M, N, K, _ptr(out) if epi != 1 else None, ldo,
                                                 _ptr(out2) if epi == 2 else None, _ptr(x) if epi == 1 else None,
                                                 _ptr(xin) if epi == 1 else None, ldx, int(score_site), int(tokens), int(group),
                                                 int(n_img), _ptr(slab), slab_ld or 0, {"auto": 0, "small": 1, "big": 2}[kernel], int(rev)))
        if epi == 1:
            return x
        return (out, slab) if score_site else out

    def _gamma_vec(self, gamma: torch.Tensor, N: int) -> torch.Tensor:
        """A LayerScale operand of the operator entries: fp32 [N] on the device, padded to 256 like a bias, values untouched."""
        if gamma.numel() != N:
            raise ValueError(f"gamma: {gamma.numel()} values for {N} output columns")
        gp = torch.zeros((N + 255) // 256 * 256, dtype=torch.float32, device=self.device)
        gp[:N].copy_(gamma.detach().reshape(-1).to(self.device, torch.float32))
        return gp

    def quantise_e4m3(self, w: torch.Tensor, *, rows_pad: Optional[int] = None, ld8: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The fp8 mode's weight quantiser on its own (ssp2_quantise_rows_e4m3, what ssp2_set_precision runs): w [rows, cols] (any float
        dtype, rounded to bf16).  Returns (uint8 [rows_pad, ld8] e4m3 bytes, f32 [rows_pad] row scales amax / 448); rows_pad defaults to
        ceil256(rows), ld8 to ceil128(cols) — the engine's weight images.  Pad rows and columns are zero bytes, pad scales 1."""
        rows, cols = w.shape
        rows_pad = (rows + 255) // 256 * 256 if rows_pad is None else int(rows_pad)
        ld8 = (cols + 127) // 128 * 128 if ld8 is None else int(ld8)
        wb = w.to(self.device, torch.bfloat16).contiguous()
        w8 = torch.empty(rows_pad, ld8, dtype=torch.uint8, device=self.device)
        sc = torch.empty(rows_pad, dtype=torch.float32, device=self.device)
        self._check(self.lib.ssp2_quantise_rows_e4m3(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), _ptr(wb), cols, rows,
                                                     cols, rows_pad, _ptr(w8), ld8, _ptr(sc)))
        return w8, sc

    def linear_e4m3(self, a8: torch.Tensor, w8: torch.Tensor, wscale: torch.Tensor, bias: Optional[torch.Tensor], epilogue: str = "bf16", *,
                    rows: Optional[int] = None, ascale: Optional[torch.Tensor] = None, ascale_const: float = 0.0,
                    out: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None, xin: Optional[torch.Tensor] = None,
                    score_site: int = 0, tokens: int = 0, group: int = 0, n_img: int = 0, slab_ld: Optional[int] = None,
                    rev: int = 0, gamma: Optional[torch.Tensor] = None):
        """One fp8 projection of the forward on its own (ssp2_linear_e4m3): a8 uint8 e4m3 [>= rows, lda] (rows = a8.shape[0] by default,
        lda = its row stride), w8 uint8 [N, K] e4m3 with K the contraction length (K % 128 == 0), wscale f32 [N], bias [N] or None (rounded
        to bf16); W, wscale and bias are padded to 256 rows like `linear` does.  Activation scale per row from ascale (f32 [>= rows]),
        or ascale_const, or 1.  epilogue "bf16" -> out bf16 [rows, >= N]; "resid" -> x (f32 [>= rows, ld]) = xin (default x) +
        bf16(...), returned; "gelu" -> out uint8 [rows, >= N] e4m3 bytes, and with score_site 1 / 2 (tokens, group, n_img: the row
        layout of ssp2_rows) the tuple (out, slab f32 [2 * ceil(rows / 256), 2, slab_ld]), slab_ld defaulting to N: entry t
        covers rows 128 t .. 128 t + 127 (zeros past the last row).  rev: the walk direction of the tiles (the forward alternates them).
        gamma (f32 [N], "resid" only): the branch's LayerScale, x = xin + fl32(gamma * bf16(...)) (ssp2_linear_ls_e4m3)."""
        epi = {"bf16": 0, "resid": 1, "gelu": 2}[epilogue]
        if gamma is not None and epi != 1:
            raise ValueError("gamma: LayerScale goes with the resid epilogue only")
        N, K = w8.shape
        M = a8.shape[0] if rows is None else int(rows)
        for name, t in (("a8", a8), ("w8", w8), ("out", out if epi == 2 else None)):
            if t is not None and (t.device.type != "cuda" or t.dim() != 2 or t.dtype != torch.uint8 or t.stride(1) != 1):
                raise ValueError(f"{name} must be a row-major 2-D uint8 (e4m3) device tensor")
        if a8.shape[0] < M or a8.shape[1] < K:
            raise ValueError(f"a8 [{tuple(a8.shape)}] smaller than [{M}, {K}]")
        # the kernel reads M rows of a8 at its row stride, and per-row scales at a stride of 1
        if ascale is not None and (ascale.device.type != "cuda" or ascale.dtype != torch.float32 or ascale.dim() != 1
                                   or ascale.stride(0) != 1 or ascale.numel() < M):
            raise ValueError(f"ascale must be a dense f32 device vector of >= {M} entries")
        if wscale.numel() != N:
            raise ValueError("wscale must hold one scale per weight row")
        npad = (N + 255) // 256 * 256
        wp = torch.zeros(npad, K, dtype=torch.uint8, device=self.device)
        wp[:N].copy_(w8)
        sp = torch.ones(npad, dtype=torch.float32, device=self.device)
        sp[:N].copy_(wscale.reshape(-1))
        bp = torch.zeros(npad, dtype=torch.float32, device=self.device)
        if bias is not None:
            bp[:N].copy_(bias.to(self.device, torch.bfloat16).float())
        slab = None
        if epi == 1:
            for name, t in (("x", x), ("xin", xin)):
                if t is not None and (t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1
                                      or t.shape[0] < M or t.shape[1] < N):
                    raise ValueError(f"resid epilogue needs {name} as a row-major f32 device tensor of >= [{M}, {N}]")
            if x is None or (xin is not None and xin.stride(0) != x.stride(0)):
                raise ValueError("resid epilogue needs x, and xin at x's row stride (the kernel reads both at ldx)")
            ldo, ldx = 0, x.stride(0)
        else:
            if out is None:
                out = torch.empty(M, N, dtype=torch.uint8 if epi == 2 else torch.bfloat16, device=self.device)
            if out.device.type != "cuda" or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < M or out.shape[1] < N \
                    or out.dtype != (torch.uint8 if epi == 2 else torch.bfloat16):
                raise ValueError(f"out must be a row-major {'uint8' if epi == 2 else 'bf16'} device tensor of >= [{M}, {N}]")
            ldo, ldx = out.stride(0), 0
            if score_site:
                slab_ld = N if slab_ld is None else int(slab_ld)
                slab = torch.full((2 * ((M + 255) // 256), 2, slab_ld), float("nan"), dtype=torch.float32, device=self.device)
        if gamma is not None:
            gp = self._gamma_vec(gamma, N)
            self._check(self.lib.ssp2_linear_ls_e4m3(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), _ptr(a8), a8.stride(0),
                                                     _ptr(ascale), float(ascale_const), _ptr(wp), K, _ptr(sp), _ptr(bp), _ptr(gp), M, N, K,
                                                     _ptr(x), _ptr(xin), ldx, int(rev)))
            return x
        self._check(self.lib.ssp2_linear_e4m3(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), epi, _ptr(a8), a8.stride(0),
                                              _ptr(ascale), float(ascale_const), _ptr(wp), K, _ptr(sp), _ptr(bp), M, N, K,
                                              _ptr(out) if epi != 1 else None, ldo, _ptr(x) if epi == 1 else None,
                                              _ptr(xin) if epi == 1 else None, ldx, int(score_site), int(tokens), int(group), int(n_img),
                                              _ptr(slab), slab_ld or 0, int(rev)))
        if epi == 1:
            return x
        return (out, slab) if score_site else out

    def attention(self, qkv: torch.Tensor, n: int, tokens: int, heads: int, d_h: int, *, group: int = 0,
                  out: Optional[torch.Tensor] = None, out8: Optional[torch.Tensor] = None, out8_scale: float = 16.0,
                  sat: Optional[torch.Tensor] = None, q_cls: Optional[torch.Tensor] = None, persist: Optional[bool] = None,
                  live: Optional[bool] = None, rev: int = 0, stream: bool = False) -> torch.Tensor:
        """Multi-head attention of the forward on its own (ssp2_attention_bf16), on caller-owned buffers: qkv bf16
        [>= rows, 3 * heads * d_h] densely packed, with rows = ssp2_rows(n, group).  Writes out (bf16 [>= rows, ldo], allocated when None) or,
        with out8 (uint8 [>= rows, ldo8]), the fp8 mode's e4m3(o * out8_scale) bytes, counting clipping waves into sat (int32
        [1]).  q_cls (bf16 [>= n, dim], densely packed): the CLS-only form, out [>= n, ldo].  persist / live override SSP2_OPT_ATTN_PERSIST /
        SSP2_OPT_ATTN_LIVE (None: on); rev: walk direction of the persistent kernels.  stream=True: the key-streaming kernel instead
        (ssp2_attention_stream_bf16, see attention_stream; bf16 output only).  Returns the tensor written."""
        if stream:
            if out8 is not None or sat is not None or persist is not None or live is not None:
                raise ValueError("the key-streaming attention writes bf16 only and has no persist / live switches")
            return self.attention_stream(qkv, n, tokens, heads, d_h, group=group, out=out, q_cls=q_cls)
        dim = heads * d_h
        named = (("qkv", qkv, torch.bfloat16), ("out", out, torch.bfloat16), ("out8", out8, torch.uint8), ("q_cls", q_cls, torch.bfloat16))
        for name, t, dt in named:
            if t is not None and (t.device.type != "cuda" or t.dim() != 2 or t.dtype != dt or t.stride(1) != 1 or t.stride(0) < t.shape[1]):
                raise ValueError(f"{name} must be a row-major 2-D {dt} device tensor")
        if sat is not None and (sat.device.type != "cuda" or sat.dtype != torch.int32 or sat.numel() < 1):
            raise ValueError("sat must be an int32 device tensor")
        need = n if q_cls is not None else ssp2_rows(n, tokens, group)
        # the kernels read qkv rows at a stride of 3 * dim and the compact CLS queries at a stride of dim: no other layout is accepted
        if qkv.shape[1] != 3 * dim or qkv.stride(0) != 3 * dim or (q_cls is not None and (q_cls.shape[1] != dim or q_cls.stride(0) != dim)):
            raise ValueError(f"qkv must be [rows, {3 * dim}] and q_cls [n, {dim}], densely packed (the kernels' row strides)")
        if qkv.shape[0] < ssp2_rows(n, tokens, group) or (q_cls is not None and q_cls.shape[0] < n):
            raise ValueError(f"qkv [{tuple(qkv.shape)}] / q_cls too small for n={n} tokens={tokens} heads={heads} d_h={d_h} group={group}")
        if out is None and out8 is None:
            out = torch.empty(need, dim, dtype=torch.bfloat16, device=qkv.device)
        for t in (out, out8):
            if t is not None and (t.shape[0] < need or t.shape[1] < dim):
                raise ValueError(f"output [{tuple(t.shape)}] smaller than [{need}, {dim}]")
        flag = {None: -1, False: 0, True: 1}
        self._check(self.lib.ssp2_attention_bf16(C.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream), _ptr(qkv), n, tokens, heads, d_h,
                                           group, _ptr(q_cls), _ptr(out), out.stride(0) if out is not None else 0, _ptr(out8),
                                           out8.stride(0) if out8 is not None else 0, float(out8_scale), _ptr(sat), flag[persist], flag[live], int(rev)))
        return out8 if out8 is not None else out

    def attention_stream(self, qkv: torch.Tensor, n: int, tokens: int, heads: int, d_h: int, *, group: int = 0,
                         out: Optional[torch.Tensor] = None, q_cls: Optional[torch.Tensor] = None, out8: Optional[torch.Tensor] = None,
                         out8_scale: float = 16.0, sat: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The key-streaming attention on its own (ssp2_attention_stream_bf16): the layouts of `attention`, d_h = 64, 1..8192 tokens.
        With out8 (uint8 [>= rows, ldo8], ldo8 a multiple of 16; full form only) the fp8 mode's e4m3(o * out8_scale) bytes instead of
        the bf16 output (ssp2_attention_stream_e4m3), out8_scale a power of two, clipping waves counted into sat (int32 [1])."""
        dim = heads * d_h
        if out8 is not None:
            if out is not None or q_cls is not None:
                raise ValueError("out8 replaces the bf16 output of the full form: no out, no q_cls")
            if qkv.device.type != "cuda" or qkv.dim() != 2 or qkv.dtype != torch.bfloat16 or qkv.stride(1) != 1:
                raise ValueError("qkv must be a row-major 2-D bf16 device tensor")
            if out8.device.type != "cuda" or out8.dim() != 2 or out8.dtype != torch.uint8 or out8.stride(1) != 1 or out8.stride(0) < out8.shape[1]:
                raise ValueError("out8 must be a row-major 2-D uint8 device tensor")
            if sat is not None and (sat.device.type != "cuda" or sat.dtype != torch.int32 or sat.numel() < 1):
                raise ValueError("sat must be an int32 device tensor")
            need = ssp2_rows(n, tokens, group)
            if qkv.shape[1] != 3 * dim or qkv.stride(0) != 3 * dim or qkv.shape[0] < need:
                raise ValueError(f"qkv [{tuple(qkv.shape)}] must be [>= {need}, {3 * dim}], densely packed (the kernels' row stride)")
            if out8.shape[0] < need or out8.shape[1] < dim:
                raise ValueError(f"output [{tuple(out8.shape)}] smaller than [{need}, {dim}]")
            self._check(self.lib.ssp2_attention_stream_e4m3(C.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream), _ptr(qkv), n, tokens,
                                                            heads, d_h, group, _ptr(out8), out8.stride(0), float(out8_scale), _ptr(sat)))
            return out8
        if sat is not None:
            raise ValueError("sat counts the clipping waves of the e4m3 output: it needs out8")
        for name, t in (("qkv", qkv), ("out", out), ("q_cls", q_cls)):
            if t is not None and (t.device.type != "cuda" or t.dim() != 2 or t.dtype != torch.bfloat16 or t.stride(1) != 1 or t.stride(0) < t.shape[1]):
                raise ValueError(f"{name} must be a row-major 2-D bf16 device tensor")
        need = n if q_cls is not None else ssp2_rows(n, tokens, group)
        if qkv.shape[1] != 3 * dim or qkv.stride(0) != 3 * dim or (q_cls is not None and (q_cls.shape[1] != dim or q_cls.stride(0) != dim)):
            raise ValueError(f"qkv must be [rows, {3 * dim}] and q_cls [n, {dim}], densely packed (the kernels' row strides)")
        if qkv.shape[0] < ssp2_rows(n, tokens, group) or (q_cls is not None and q_cls.shape[0] < n):
            raise ValueError(f"qkv [{tuple(qkv.shape)}] / q_cls too small for n={n} tokens={tokens} heads={heads} d_h={d_h} group={group}")
        if out is None:
            out = torch.empty(need, dim, dtype=torch.bfloat16, device=qkv.device)
        if out.shape[0] < need or out.shape[1] < dim:
            raise ValueError(f"output [{tuple(out.shape)}] smaller than [{need}, {dim}]")
        self._check(self.lib.ssp2_attention_stream_bf16(C.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream), _ptr(qkv), n, tokens,
                                                        heads, d_h, group, _ptr(q_cls), _ptr(out), out.stride(0)))
        return out

    def attention_prefix(self, qkv: torch.Tensor, n: int, tokens: int, heads: int, d_h: int, q: torch.Tensor, n_prefix: int, *,
                         group: int = 0, out: Optional[torch.Tensor] = None, stream: bool = False) -> torch.Tensor:
        """The evaluation tail's prefix-query attention on its own (ssp2_attention_prefix_bf16): n_prefix (1 or 2) queries per image,
        q bf16 [n_prefix * n, dim] prefix-major (row t * n + i = prefix query t of image i), densely packed; qkv as in `attention`.
        Returns out bf16 [n_prefix * n, ldo] in the same order.  stream=True: the key-streaming kernel (d_h = 64)."""
        dim = heads * d_h
        for name, t in (("qkv", qkv), ("q", q), ("out", out)):
            if t is not None and (t.device.type != "cuda" or t.dim() != 2 or t.dtype != torch.bfloat16 or t.stride(1) != 1 or t.stride(0) < t.shape[1]):
                raise ValueError(f"{name} must be a row-major 2-D bf16 device tensor")
        if qkv.shape[1] != 3 * dim or qkv.stride(0) != 3 * dim or q.shape[1] != dim or q.stride(0) != dim:
            raise ValueError(f"qkv must be [rows, {3 * dim}] and q [n_prefix * n, {dim}], densely packed (the kernels' row strides)")
        if qkv.shape[0] < ssp2_rows(n, tokens, group) or q.shape[0] < n_prefix * n:
            raise ValueError(f"qkv [{tuple(qkv.shape)}] / q [{tuple(q.shape)}] too small for n={n} tokens={tokens} n_prefix={n_prefix} group={group}")
        if out is None:
            out = torch.empty(n_prefix * n, dim, dtype=torch.bfloat16, device=qkv.device)
        if out.shape[0] < n_prefix * n or out.shape[1] < dim:
            raise ValueError(f"output [{tuple(out.shape)}] smaller than [{n_prefix * n}, {dim}]")
        self._check(self.lib.ssp2_attention_prefix_bf16(C.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream), _ptr(qkv), n, tokens,
                                                        heads, d_h, group, _ptr(q), _ptr(out), out.stride(0), int(n_prefix), int(bool(stream))))
        return out

    def layernorm(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, *, rows: Optional[int] = None,
                  in_stride: Optional[int] = None, gather: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                  ascale: Optional[torch.Tensor] = None, rev: int = 0) -> torch.Tensor:
        """LayerNorm of the forward on its own (ssp2_layernorm), on caller-owned buffers: row r of x (f32) at r * in_stride
        (default: x's row stride), or, gather = (tokens, group), the CLS row of image r in that layout.  D = gamma.numel().
        out bf16 [>= rows, ld] (allocated when None) or uint8 [>= rows, ld] — the fp8 mode's per-row-scaled e4m3 bytes, with
        the row scales (f32 [rows]) in ascale.  rev: walk direction (taken from 4096 rows on, as in the forward)."""
        D = gamma.numel()
        for name, t in (("x", x), ("gamma", gamma), ("beta", beta)):
            if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous f32 device tensor")
        if beta.numel() != D:
            raise ValueError("gamma / beta sizes differ")
        if rows is None:
            rows = x.shape[0]
        if gather is not None:
            if x.dim() != 2 or x.shape[1] != D:                # the gather reads the CLS row of image r at row_of(r) * D
                raise ValueError(f"the gathered form needs x as a [rows, {D}] token matrix")
            if x.numel() < ssp2_rows(rows, gather[0], gather[1]) * D:
                raise ValueError("x smaller than the gathered layout")
            in_stride = 0
        else:
            in_stride = x.stride(0) if in_stride is None else int(in_stride)
            if x.numel() < (rows - 1) * in_stride + D:
                raise ValueError("x smaller than rows * in_stride")
        if out is None:
            out = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device)
        fp8 = out.dtype == torch.uint8
        if (out.device.type != "cuda" or out.dim() != 2 or out.dtype not in (torch.bfloat16, torch.uint8) or out.stride(1) != 1
                or out.shape[0] < rows or out.shape[1] < D):
            raise ValueError(f"out must be a row-major bf16 / uint8 device tensor of >= [{rows}, {D}]")
        if fp8 and (ascale is None or ascale.device.type != "cuda" or ascale.dtype != torch.float32 or ascale.numel() < rows):
            raise ValueError("the e4m3 form needs ascale, f32 [rows] on the device")
        gt, gg = gather if gather is not None else (0, 0)
        self._check(self.lib.ssp2_layernorm(C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream), _ptr(x), in_stride, rows, D,
                                      _ptr(gamma), _ptr(beta), float(eps), gt, gg, None if fp8 else _ptr(out), out.stride(0),
                                      _ptr(out) if fp8 else None, _ptr(ascale) if fp8 else None, int(rev)))
        return out

    # ------------------------------------------------------------------ compositions used by the host API
    def forward_scores(self, pixels: torch.Tensor, score_site: str, score_chain: str = "fp32",
                       group: int = 0) -> torch.Tensor:
        """One forward over `pixels` (one or several dataloader batches of `group` images each, concatenated).
        Returns f32 [n_groups, depth, score_ld]; entry [g, l] = sum over group g's samples of the per-sample
        token-L2 of block l's FFN activation (reference hook body, src/vit_pruning.py:151-152)."""
        n = sum(int(p.shape[0]) for p in pixels) if isinstance(pixels, (list, tuple)) else pixels.shape[0]
        if n > self.max_images:
            raise Ssp2Error(f"chunk of {n} images exceeds engine capacity {self.max_images}")
        x = self.embed(pixels, group=group)             # slab layout: one 128-row-aligned slab per batch
        return self.layers(x, n, 0, self.depth, None, score_site, score_chain, None, group, scores_only=True)

    def forward_logits(self, pixels: torch.Tensor, attn_skip: Optional[Sequence[int]] = None) -> torch.Tensor:
        outs = []
        for s in range(0, pixels.shape[0], self.max_images):
            chunk = pixels[s:s + self.max_images]
            x = self.embed(chunk)
            self.layers(x, chunk.shape[0], 0, self.depth - 1, attn_skip)
            outs.append(self.tail(x, chunk.shape[0], attn_skip, want_logits=True)[0])
        return torch.cat(outs, 0)

    def profile(self, klass: str):
        """HIP events around every launch of one kernel class ("gemm_fc1", ...) or of every class ("all"); after the block:
        .total_ms / .launches / .flops, and with "all" also .by_class[name] = dict(ms, launches, flops, bytes)."""
        eng = self

        class _Ctx:
            def __enter__(self_inner):
                eng._bind_stream()
                eng._check(eng.lib.ssp2_profile_begin(eng.h, len(K_CLASS) if klass == "all" else K_CLASS[klass]))
                return self_inner

            def __exit__(self_inner, *exc):
                ms, cnt, fl = C.c_double(), C.c_int64(), C.c_double()
                if klass == "all":
                    self_inner.by_class = {}
                    for name, k in K_CLASS.items():
                        by = C.c_double()
                        eng._check(eng.lib.ssp2_profile_query(eng.h, k, C.byref(ms), C.byref(cnt), C.byref(fl), C.byref(by)))
                        if cnt.value:
                            self_inner.by_class[name] = {"ms": ms.value, "launches": cnt.value, "flops": fl.value, "bytes": by.value}
                eng._check(eng.lib.ssp2_profile_end(eng.h, C.byref(ms), C.byref(cnt), C.byref(fl)))
                self_inner.total_ms, self_inner.launches, self_inner.flops = ms.value, cnt.value, fl.value
                return False
        return _Ctx()
