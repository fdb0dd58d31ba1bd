"""Long sequences (more than 288 tokens) on the key-streaming attention: the parts that need no GPU — the C ABI, the argument checks of
ssp2_attention_stream_bf16 (all made before the device is touched), the new model geometries, the CLI switch and VitEngine's argument
check."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

from conftest import PKG


def _lib():
    from ssp2vit import _lib
    return _lib, _lib.load()


def test_abi_7_and_the_streaming_entries_are_exported():
    L, lib = _lib()
    assert L.ABI_VERSION == 7 and lib.ssp2_abi_version() == 7
    for name in ("ssp2_create_opts", "ssp2_attention_stream_bf16"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert L.OPTIONS["attn_stream"] == 13 and L.OPT_COUNT == 14 and max(L.OPTIONS.values()) == L.OPT_COUNT - 1
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "ssp2vit.h")).read()
    assert "#define SSP2_ABI_VERSION 7" in hdr and f"#define SSP2_ATTN_STREAM_MAX_TOKENS {L.ATTN_STREAM_MAX_TOKENS}" in hdr


def test_stream_operator_refuses_bad_arguments_before_touching_the_device():
    L, lib = _lib()
    fake = C.c_void_p(0x1000)           # never dereferenced: every refusal happens before the first HIP call
    T_MAX = L.ATTN_STREAM_MAX_TOKENS

    def call(qkv=fake, n=2, tokens=577, heads=3, d_h=64, group=0, q_cls=None, out=fake, ldo=192):
        return lib.ssp2_attention_stream_bf16(None, qkv, n, tokens, heads, d_h, group, q_cls, out, ldo)

    bad = {
        "d_h 80": dict(d_h=80), "d_h 16": dict(d_h=16), "d_h 0": dict(d_h=0),
        "tokens 0": dict(tokens=0), "tokens -1": dict(tokens=-1), "tokens above the maximum": dict(tokens=T_MAX + 1),
        "ldo below dim": dict(ldo=191), "ldo not a multiple of 8": dict(ldo=196), "null qkv": dict(qkv=None), "null out": dict(out=None),
        "group < 0": dict(group=-1), "n 0": dict(n=0), "heads 0": dict(heads=0),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what                                   # SSP2_EINVAL
        assert lib.ssp2_last_error()
    # the resident operator keeps its contract: 289 tokens are still refused there
    assert lib.ssp2_attention_bf16(None, fake, 1, 289, 1, 64, 0, None, fake, 64, None, 0, 16.0, None, -1, -1, 0) == -1


def test_create_opts_refuses_bad_overrides_before_touching_the_device():
    L, lib = _lib()
    d_int = (C.c_int32 * 2)(1536, 1536)
    desc = L.VitDesc(384, 16, 384, 6, 2, 10, 1e-6, 4, d_int)
    h = C.c_void_p()
    for idx, val in ((L.OPTIONS["attn_stream"], 3), (L.OPTIONS["attn_stream"], -2), (L.OPTIONS["zigzag"], -5)):
        opt = (C.c_int32 * L.OPT_COUNT)(*([-1] * L.OPT_COUNT))
        opt[idx] = val
        assert lib.ssp2_create_opts(C.byref(desc), opt, C.byref(h)) == -1, (idx, val)
        assert not h.value


def test_long_sequence_geometries():
    from ssp2vit.weights import VIT_CONFIGS, n_tokens, synthetic_weights
    want = {"vit_tiny_patch16_384": 577, "vit_small_patch16_384": 577, "vit_base_patch16_384": 577, "vit_large_patch16_384": 577,
            "vit_small_patch16_384_d3": 577, "vit_base_patch16_384_d2": 577, "vit_small_patch8_224_d2": 785, "vit_tiny_patch16_512_d2": 1025}
    for name, tokens in want.items():
        img, patch, dim, heads, _, _ = VIT_CONFIGS[name]
        assert (img // patch) ** 2 + 1 == tokens and dim // heads == 64, name
    w = synthetic_weights("vit_small_patch8_224_d2", classes=10)
    assert n_tokens(w) == 785 and tuple(w["pos"].shape)[-2] == 785
    # the names that were there keep their geometry
    assert VIT_CONFIGS["vit_base_patch16_224"] == (224, 16, 768, 12, 3072, 12)


def test_long_sequences_flag_parses():
    spec = importlib.util.spec_from_file_location("auto_2ssp_amd_ls", os.path.join(PKG, "auto_2ssp.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    p = cli.build_argparser()
    assert p.parse_args(["--model", "vit_tiny_patch16_384", "--target", "0.3", "--long-sequences"]).long_sequences is True
    assert p.parse_args(["--target", "0.3"]).long_sequences is False


def test_vit_engine_validates_attn_stream_before_the_device_check():
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    w = synthetic_weights("vit_test_patch16_32", classes=10)
    for bad in (3, -1, "1", 1.5, True):
        with pytest.raises(ValueError, match="attn_stream"):
            VitEngine(w, device="cuda:0", max_images=2, attn_stream=bad)


def test_engine_cache_key_follows_the_setting(monkeypatch):
    from ssp2vit import vit_pruning as vp
    monkeypatch.setattr(vp, "DEFAULT_ATTN_STREAM", None)
    monkeypatch.delenv("SSP2_ATTN_STREAM", raising=False)
    assert vp.attn_stream_setting() == 0
    monkeypatch.setenv("SSP2_ATTN_STREAM", "1")
    assert vp.attn_stream_setting() == 1
    assert vp.attn_stream_setting(2) == 2
    monkeypatch.setattr(vp, "DEFAULT_ATTN_STREAM", 0)
    assert vp.attn_stream_setting() == 0
