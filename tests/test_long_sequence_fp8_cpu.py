"""fp8 on the key-streaming attention (SSP2_OPT_STREAM_FP8, ssp2_attention_stream_e4m3): the parts that need no GPU — the option's
index in the binding and the header, the new entry's argument checks (all made before the device is touched), VitEngine's argument
check, the CLI switch and the engine-building setting."""
import ctypes as C
import importlib.util
import os
import re

import pytest

from conftest import PKG


def _lib():
    from ssp2vit import _lib
    return _lib, _lib.load()


def _header():
    return open(os.path.join(os.path.dirname(PKG), "include", "ssp2vit.h")).read()


def test_option_index_agrees_with_the_header_and_the_create_table_keeps_its_length():
    """SSP2_OPT_STREAM_FP8 is an EXTENDED option: it sits behind SSP2_OPT_COUNT, which stays the length of ssp2_create_opts' opt[] array
    (a caller built against the earlier header passes that many entries), and ssp2_set_option / ssp2_get_option take [0, SSP2_OPT_END)."""
    L, lib = _lib()
    hdr = _header()
    assert L.ABI_VERSION == 7 and lib.ssp2_abi_version() == 7 and "#define SSP2_ABI_VERSION 7" in hdr
    m = re.search(r"enum \{ (SSP2_OPT_ZIGZAG = 0,.*?) \};", hdr, re.S)
    names = [t.split("=")[0].strip() for t in m.group(1).replace("\n", " ").split(",")]
    assert names[-1] == "SSP2_OPT_COUNT" and names.index("SSP2_OPT_COUNT") == L.OPT_COUNT
    for key, idx in L.OPTIONS.items():
        assert names[idx] == "SSP2_OPT_" + key.upper(), key
    assert "enum { SSP2_OPT_STREAM_FP8 = SSP2_OPT_COUNT, SSP2_OPT_END };" in hdr
    assert L.EXT_OPTIONS == {"stream_fp8": L.OPT_COUNT} and L.OPT_END == L.OPT_COUNT + 1
    assert not set(L.EXT_OPTIONS) & set(L.OPTIONS)
    assert "SSP2_STREAM_FP8" in hdr and "unless SSP2_OPT_STREAM_FP8" in hdr
    for name in ("ssp2_attention_stream_e4m3",):
        assert name in L.SYMBOLS and hasattr(lib, name) and f"int {name}(" in hdr


def test_stream_e4m3_operator_refuses_bad_arguments_before_touching_the_device():
    L, lib = _lib()
    fake = C.c_void_p(0x1000)           # never dereferenced: every refusal happens before the first HIP call
    T_MAX = L.ATTN_STREAM_MAX_TOKENS

    def call(qkv=fake, n=2, tokens=577, heads=3, d_h=64, group=0, out8=fake, ldo8=192, scale=16.0, sat=None):
        return lib.ssp2_attention_stream_e4m3(None, qkv, n, tokens, heads, d_h, group, out8, ldo8, scale, sat)

    bad = {
        "d_h 80": dict(d_h=80), "d_h 16": dict(d_h=16), "d_h 0": dict(d_h=0),
        "tokens 0": dict(tokens=0), "tokens -1": dict(tokens=-1), "tokens above the maximum": dict(tokens=T_MAX + 1),
        "ldo8 below dim": dict(ldo8=176), "ldo8 not a multiple of 16": dict(ldo8=200), "out8 not 16-byte aligned": dict(out8=C.c_void_p(0x1008)),
        "scale 3": dict(scale=3.0), "scale 0": dict(scale=0.0), "scale -16": dict(scale=-16.0), "scale inf": dict(scale=float("inf")),
        "scale nan": dict(scale=float("nan")), "null qkv": dict(qkv=None), "null out8": dict(out8=None),
        "group < 0": dict(group=-1), "n 0": dict(n=0), "heads 0": dict(heads=0),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what                                   # SSP2_EINVAL
        assert lib.ssp2_last_error()


def test_vit_engine_validates_stream_fp8_before_the_device_check():
    from ssp2vit.engine import VitEngine
    from ssp2vit.weights import synthetic_weights
    w = synthetic_weights("vit_test_patch16_32", classes=10)
    for bad in (1, 0, 2, "1", 1.0, "yes"):
        with pytest.raises(ValueError, match="stream_fp8"):
            VitEngine(w, device="cuda:0", max_images=2, stream_fp8=bad)


def test_long_sequences_with_fp8_parses_and_selects_the_option():
    spec = importlib.util.spec_from_file_location("auto_2ssp_amd_ls8", os.path.join(PKG, "auto_2ssp.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    a = cli.build_argparser().parse_args(["--model", "vit_base_patch16_384", "--target", "0.3", "--long-sequences", "--precision", "fp8"])
    assert a.long_sequences is True and a.precision == "fp8"
    src = open(os.path.join(PKG, "auto_2ssp.py")).read()
    assert "vp.DEFAULT_STREAM_FP8 = True if (args.long_sequences and args.precision == \"fp8\") else None" in src


def test_stream_fp8_setting_follows_argument_default_and_environment(monkeypatch):
    from ssp2vit import vit_pruning as vp
    monkeypatch.setattr(vp, "DEFAULT_STREAM_FP8", None)
    monkeypatch.delenv("SSP2_STREAM_FP8", raising=False)
    assert vp.stream_fp8_setting() is False
    monkeypatch.setenv("SSP2_STREAM_FP8", "1")
    assert vp.stream_fp8_setting() is True and vp.stream_fp8_setting(False) is False
    monkeypatch.setenv("SSP2_STREAM_FP8", "0")
    assert vp.stream_fp8_setting() is False and vp.stream_fp8_setting(True) is True
    monkeypatch.setattr(vp, "DEFAULT_STREAM_FP8", True)
    assert vp.stream_fp8_setting() is True
