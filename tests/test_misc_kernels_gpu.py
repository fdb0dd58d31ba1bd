"""The small kernels of csrc/misc.hip.h and the host code around them — score finish, weight path, fp8 calibration — against the
restatements of tests/misc_kernel_cases.py (proved on the CPU by tests/test_misc_kernel_statements_cpu.py).  Statements and bounds were
written before the first GPU run; u = 2^-24.

Every __global__ of csrc/misc.hip.h in the product build, and the direct test that holds it to something that is not the code under test:
  im2col_patch_kernel            test_embed_head_numerics_gpu.py  test_patch_embedding_exact_operands_bit_for_bit (patch_lds = 0)
  cls_row_kernel                 test_embed_head_numerics_gpu.py  test_patch_embedding_exact_operands_bit_for_bit (prefix rows)
  gather_cls_rows_kernel         test_embed_head_numerics_gpu.py  test_tail_slots_count_per_slot_against_shared_labels (slab layout)
  layernorm_bf16_kernel          test_operator_numerics_gpu.py    test_layernorm_vs_float64_widths_rows_eps_and_forms, ..._cls_gather_...
  score_norms_from_slab_kernel   here  test_fused_finish_exact_slabs_bit_for_bit, test_fused_finish_realistic_slabs_against_float64
  score_colsum_kernel            here  the same two
  act_l2_norms_kernel            here  test_act_l2_accum_bit_for_bit_and_against_float64 (bf16 and f32 instantiations)
  score_colsum_halves_kernel     here  the same
  argmax_top1_kernel             test_embed_head_numerics_gpu.py  test_head_logits_and_top1_bit_for_bit, test_top1_ties_infinities_and_nans
  dist_head_top1_kernel          test_embed_head_numerics_gpu.py  test_distillation_head_mean_and_top1_bit_for_bit, ..._ties_...
  gather_matrix_kernel           here  test_prune_in_place_*, test_prune_into_a_twin_*, test_second_prune_*, test_narrow_block_*
  gather_vector_kernel           here  the same
  convert_pad_bf16_kernel        here  test_ingest_every_route_bit_for_bit [host], [dev]
  round_bias_kernel              here  the same
  ingest_batch_kernel            here  test_ingest_every_route_bit_for_bit [batch] (71 entries: two launches)
  quant_rows_e4m3_kernel         test_fp8_gemm_numerics_gpu.py    test_quantiser_bit_for_bit; here test_fp8_images_after_a_prune_* (the engine's use)
  e4m3_top_code_count_kernel     here  test_fp8_calibration_counts_top_codes_of_the_images_only
  absmax_bf16_kernel             here  test_fp8_calibration_scale_ignores_stale_pad_rows
(xcc_probe_kernel is launched by the lab build only.)

Fused finish.  Exact slabs (distinct integers, every per-image sum exact in fp32): norms and group sums bit for bit, NaN-filled
buffers, every entry of [groups, ld] finite afterwards and every column at or past ld untouched.  Realistic slabs (positive, seven
orders of magnitude): rtol (tiles per image + group + 2) u against float64 — a sequential fp32 sum of positive terms is within
(count - 1) u of the exact one, the root halves its operand's relative error and adds one rounding; on the bf16 chain at most 1 bf16
ulp per element (the CPU test shows the fp32 statement itself stays inside both on these inputs).
Stand-alone route through the C entry: bit for bit in the documented association and rtol (group + 4) u against float64 — the sum of
squares is exact, the root one rounding, lanes and fold at most (ceil(group / 4) - 1) + 2 more.
Weight path: everything bit for bit (NaN positions as "is NaN"), whole images, pads included.
fp8 calibration: the slab layout's pad rows hold stale attention outputs and fc1 of LayerNorm of zero rows; neither may count.
A contiguous launch reaches the e4m3 path (where calibration records) from 256 rows on, 52 of these 5-token images: the contiguous
side of both calibration tests therefore runs the 21 images repeated to 58 — the same set of images, so the same max |o|, and
2 x 58 x 5 top codes.

After the first GPU run no statement and no bound had to change.  Fused finish, fp32 chain: worst error 3.44 u against bounds of
5 .. 23 u; bf16 chain: no element off the float64 statement.  The two calibration tests FAILED against the calibration kernels as
they were (every row of [0, M) counted): 582 top codes = 2 x 291 rows instead of 210 = 2 x 21 x 5, and scales [1.0, 1.0] (max |o| ~ 100
out of the stale rows) instead of [64.0, 64.0]; absmax_bf16_kernel and e4m3_top_code_count_kernel now take the RowMap and the image
count and skip rows that are no image's (row_is_image), and both tests pass.
Planted defects, all in bounds, built once into a library of their own, run against this module once and reverted:
  slab0 = 0 in score_norms_from_slab_kernel (slab offset ignored)   both fused tests at every slab-layout case (3, 4, 5, 7, 8); the contiguous ones pass
  fold ((p0 + p1) + p2) + p3 in score_colsum_halves_kernel          test_act_l2_accum_* at every case with a group of 4 or more and non-integer norms
  truncation in round_bias_kernel                                   test_ingest_* [host] and [dev]; [batch] (its own kernel) passes
  rows past n_keep copied, not zeroed, by gather_matrix_kernel      every prune test but keep = all
"""
import ctypes as C
import time

import pytest
import torch

import misc_kernel_cases as MK

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = MK.U
EINVAL, ESTATE = -1, -4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    t0 = time.time()
    yield
    print(f"\n[misc kernels] module time {time.time() - t0:.1f} s")


def _engine(w, n=4, **kw):
    from ssp2vit.engine import VitEngine
    return VitEngine(w, device=DEV, max_images=n, **kw)


@pytest.fixture(scope="module")
def op():
    """An engine for the stand-alone wrappers (they need no weights of its)."""
    geo = MK.geometry()
    e = _engine(MK.random_weights(geo, seed=1))
    yield e
    e.close()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _same(got, want, what):
    bad = MK.differs(got, want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[:4].tolist()}"


def _nan(*shape):
    return torch.full(shape, MK.NAN, dtype=torch.float32, device=DEV)


# ----------------------------------------------------------------------------------------------------------- fused score finish
def _finish(op, slab, n, tokens, group, chain, extra=8):
    ld = slab.shape[2]
    groups = -(-n // MK.group_of(n, group))
    norms, out = _nan(n, ld), _nan(groups, ld + extra)
    o, nr = op.score_finish(slab.to(DEV), n, tokens, group, "bf16_ref" if chain else "fp32", norms=norms, out=out)
    assert o is out and nr is norms
    out, norms = out.cpu(), norms.cpu()
    assert bool(out[:, ld:].isnan().all()), "columns at and past ld are the caller's"
    assert bool(out[:, :ld].isfinite().all()) and bool(norms.isfinite().all())
    return out[:, :ld].contiguous(), norms


@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("i", range(len(MK.FUSED_CASES)))
def test_fused_finish_exact_slabs_bit_for_bit(op, i, chain):
    tokens, n, group, ld = MK.FUSED_CASES[i]
    slab = MK.exact_slab(n, tokens, group, ld, seed=i)
    want_out, want_norms = MK.finish_fused(slab, n, tokens, group, chain)
    out, norms = _finish(op, slab, n, tokens, group, chain)
    _same(norms, want_norms, f"norms {MK.FUSED_CASES[i]} chain {chain}")
    _same(out, want_out, f"group sums {MK.FUSED_CASES[i]} chain {chain}")


@pytest.mark.parametrize("i", range(len(MK.FUSED_CASES)))
def test_fused_finish_realistic_slabs_against_float64(op, i):
    tokens, n, group, ld = MK.FUSED_CASES[i]
    slab = MK.realistic_slab(n, tokens, group, ld, seed=100 + i)
    rtol = (MK.tiles_per_sample(n, tokens, group) + MK.group_of(n, group) + 2) * U
    out, norms = _finish(op, slab, n, tokens, group, 0)
    out64, norms64 = MK.finish_fused_f64(slab, n, tokens, group, 0)
    e_out, e_nrm = float(((out.double() - out64).abs() / out64).max()), float(((norms.double() - norms64).abs() / norms64).max())
    out1, norms1 = _finish(op, slab, n, tokens, group, 1)
    out64b, norms64b = MK.finish_fused_f64(slab, n, tokens, group, 1)
    d_out, d_nrm = MK.bf16_ulps_apart(out1, out64b), MK.bf16_ulps_apart(norms1, norms64b)
    print(f"\n[fused finish {MK.FUSED_CASES[i]}] fp32 chain: worst relative error {e_out / U:.2f} u (sums) {e_nrm / U:.2f} u (norms), bound "
          f"{rtol / U:.0f} u; bf16 chain: {int((d_out > 0).sum())} of {d_out.numel()} sums, {int((d_nrm > 0).sum())} of {d_nrm.numel()} norms off float64")
    assert e_out <= rtol and e_nrm <= rtol
    assert torch.equal(out1.to(torch.bfloat16).float(), out1) and torch.equal(norms1.to(torch.bfloat16).float(), norms1)
    assert int(d_out.max()) <= 1 and int(d_nrm.max()) <= 1


def test_score_finish_checks_every_argument_before_the_device(op):
    lib = op.lib
    n, tokens, ld = 3, 197, 64
    slab = torch.ones(MK.slab_tiles(n, tokens, 0), 2, ld, device=DEV)
    norms, out = _nan(n, ld), _nan(1, ld)

    def call(slab_=slab, n_=n, tokens_=tokens, group=0, ld_=ld, chain=0, norms_=norms, out_=out, stride=ld):
        return lib.ssp2_score_finish(_stream(), _p(slab_) if slab_ is not None else None, n_, tokens_, group, ld_, chain,
                                     _p(norms_) if norms_ is not None else None, _p(out_) if out_ is not None else None, stride)
    for what, kw in [("tokens < 128", dict(tokens_=127)), ("ld < 1", dict(ld_=0)), ("out_stride < ld", dict(stride=ld - 1)), ("null slab", dict(slab_=None)),
                     ("null norms", dict(norms_=None)), ("null out", dict(out_=None)), ("n = 0", dict(n_=0)), ("group < 0", dict(group=-1)), ("chain", dict(chain=2))]:
        assert call(**kw) == EINVAL, what
        assert lib.ssp2_last_error()
    torch.cuda.synchronize()
    assert bool(norms.isnan().all()) and bool(out.isnan().all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(out.isfinite().all())


# ----------------------------------------------------------------------------------------------------------- stand-alone route
def _act_l2(lib, act, d, chain, group, extra=8):
    n, tokens, ld = act.shape
    groups = -(-n // MK.group_of(n, group))
    ws, out = _nan(2, n, ld), _nan(groups, ld + extra)
    rc = lib.ssp2_act_l2_accum(_stream(), _p(act), 0 if act.dtype == torch.bfloat16 else 1, n, tokens, d, ld, chain, group, _p(ws), _p(out), ld + extra)
    assert rc == 0, lib.ssp2_last_error()
    out = out.cpu()
    assert bool(out[:, ld:].isnan().all()), "columns between ld and out_stride are the caller's"
    return out[:, :ld].contiguous()


@pytest.mark.parametrize("i", range(len(MK.ACT_L2_CASES)))
def test_act_l2_accum_bit_for_bit_and_against_float64(op, i):
    tokens, n, group, d, ld = MK.ACT_L2_CASES[i]
    act = MK.act_l2_input(tokens, n, ld, seed=i)
    want64 = MK.act_l2_f64(act, group)
    rtol = (MK.group_of(n, group) + 4) * U
    for chain in (0, 1):
        want = MK.act_l2_statement(act, group, chain)
        for dtype in (torch.bfloat16, torch.float32):
            what = f"{MK.ACT_L2_CASES[i]} chain {chain} {dtype}"
            out = _act_l2(op.lib, act.to(DEV, dtype).contiguous(), d, chain, group)
            _same(out, want, what)                       # columns [d, ld) included: the pad columns carry values of their own
            if not chain:
                assert float(((out.double() - want64).abs() / want64.clamp_min(1e-300)).max()) <= rtol, what


def test_act_l2_accum_refuses_an_out_stride_below_ld(op):
    n, tokens, d, ld = 5, 7, 64, 64
    act = MK.act_l2_input(tokens, n, ld, seed=99).to(DEV, torch.bfloat16)
    ws, out = _nan(2, n, ld), _nan(3, ld)
    rc = op.lib.ssp2_act_l2_accum(_stream(), _p(act), 0, n, tokens, d, ld, 0, 2, _p(ws), _p(out), ld - 8)
    assert rc == EINVAL and b"out_stride" in op.lib.ssp2_last_error()
    torch.cuda.synchronize()
    assert bool(ws.isnan().all()) and bool(out.isnan().all()), "nothing was launched"


# ------------------------------------------------------------------------------------------------------------------- ingest
INGEST_GEO = MK.geometry(depth=5, d_int=(203, 72, 64, 65, 130), prefix=2, dist_head=True)


def _load(eng, w, route, names):
    from ssp2vit._lib import T_KINDS
    lib = eng.lib
    eng._bind_stream()
    if route == "host":
        for k, l in names:
            t = w[MK.key_of(k, l)].contiguous()
            eng._check(lib.ssp2_load_tensor(eng.h, T_KINDS.index(k), l, C.cast(t.data_ptr(), C.POINTER(C.c_float)), t.numel()))
        return
    dev = [w[MK.key_of(k, l)].to(DEV).contiguous() for k, l in names]
    if route == "dev":
        for (k, l), t in zip(names, dev):
            eng._check(lib.ssp2_load_tensor_dev(eng.h, T_KINDS.index(k), l, _p(t), t.numel()))
    else:
        m = len(names)
        assert m > 64, "two launches of the batched ingest"
        eng._check(lib.ssp2_load_tensors_dev(eng.h, m, (C.c_int * m)(*[T_KINDS.index(k) for k, _ in names]), (C.c_int * m)(*[l for _, l in names]),
                                             (C.c_void_p * m)(*[t.data_ptr() for t in dev]), (C.c_size_t * m)(*[t.numel() for t in dev])))
    torch.cuda.synchronize()                             # the sources stay alive until the stream has passed


def _check_images(eng, w, names, what):
    for k, l in names:
        src = w[MK.key_of(k, l)]
        shape = eng.peek_shape(k, l)
        assert shape == dict(MK.fresh_shape(k, src), ld8=0), (what, k, l, shape)
        _same(eng.peek_tensor(k, l), MK.expected_image(k, src, shape), f"{what}: {k} of block {l}")


@pytest.mark.parametrize("route", ["host", "dev", "batch"])
def test_ingest_every_route_bit_for_bit(route):
    """ssp2_load_tensor / _dev / ssp2_load_tensors_dev: matrices are torch's .to(bfloat16) in a zero [ceil256(rows), ceil64(cols)] image,
    biases its bf16 rounding kept as fp32, zero padded, vectors unchanged — on ties, their fp32 neighbours, the fp32 maximum, subnormals,
    zeros, infinities and NaNs.  Loaded twice: the second image shows no trace of the first."""
    names = MK.tensor_list(INGEST_GEO["depth"], True)
    wa, wb = MK.special_weights(INGEST_GEO, seed=1), MK.special_weights(INGEST_GEO, seed=2)
    eng = _engine(MK.random_weights(INGEST_GEO, seed=5))
    try:
        _load(eng, wa, route, names)
        _check_images(eng, wa, names, f"{route}, first load")
        _load(eng, wb, route, names)
        _check_images(eng, wb, names, f"{route}, second load")
    finally:
        eng.close()


def test_peek_tensor_checks_its_arguments_and_changes_nothing(op):
    from ssp2vit._lib import T_KINDS
    lib = op.lib
    buf = torch.full((256 * 64,), 7, dtype=torch.int16)
    K = T_KINDS.index

    def peek(kind, layer, image, nbytes):
        return lib.ssp2_peek_tensor(op.h, kind, layer, image, C.c_void_p(buf.data_ptr()), nbytes)
    fc1 = 256 * 64 * 2
    for what, rc, args in [("kind -1", EINVAL, (-1, 0, 1, fc1)), ("kind past the last", EINVAL, (len(T_KINDS), 0, 1, fc1)), ("layer", EINVAL, (K("fc1_w"), 2, 1, fc1)),
                           ("layer < 0", EINVAL, (K("fc1_w"), -1, 1, fc1)), ("image", EINVAL, (K("fc1_w"), 0, 4, fc1)), ("bytes", EINVAL, (K("fc1_w"), 0, 1, fc1 - 2)),
                           ("shape bytes", EINVAL, (K("fc1_w"), 0, 0, 16)), ("no distillation token", EINVAL, (K("dist"), 0, 1, 256)),
                           ("e4m3 of a bias", EINVAL, (K("fc1_b"), 0, 2, 1024)), ("scale of a vector", EINVAL, (K("ln1_g"), 0, 3, 256)),
                           ("e4m3 on a bf16 engine", ESTATE, (K("fc1_w"), 0, 2, 256 * 128)), ("scale on a bf16 engine", ESTATE, (K("fc2_w"), 1, 3, 1024))]:
        assert peek(*args) == rc, what
    assert lib.ssp2_peek_tensor(op.h, K("fc1_w"), 0, 1, None, fc1) == EINVAL
    assert bool((buf == 7).all())
    before = op.peek_tensor("fc1_w", 0)
    assert peek(K("fc1_w"), 0, 1, fc1) == 0 and not bool((buf == 7).all())
    _same(op.peek_tensor("fc1_w", 0), before, "a second look")
    assert op.peek_shape("fc1_w", 0) == dict(rows=203, cols=64, rows_pad=256, ld=64, ld8=0)
    assert op.peek_shape("fc2_w", 1) == dict(rows=64, cols=72, rows_pad=256, ld=128, ld8=0)
    assert op.peek_shape("pos", 0) == dict(rows=5 * 64, cols=1, rows_pad=5 * 64, ld=1, ld8=0)


# --------------------------------------------------------------------------------------------------------------- compaction
GEO = MK.geometry()
FFN_KINDS = ("fc1_w", "fc1_b", "fc2_w", "fc2_b")


@pytest.fixture(scope="module")
def coded():
    return MK.coded_ffn(GEO, MK.random_weights(GEO, seed=3))


def _sliced(w, layer, keep):
    k = torch.as_tensor(list(keep), dtype=torch.long)
    w = dict(w)
    w[f"fc1_w.{layer}"], w[f"fc1_b.{layer}"], w[f"fc2_w.{layer}"] = w[f"fc1_w.{layer}"][k], w[f"fc1_b.{layer}"][k], w[f"fc2_w.{layer}"][:, k]
    return w


def _check_block(eng, w, layer, keep, fc1_rows_pad, what):
    """Block `layer` of `eng` holds the host-sliced images of `w` (None: the whole block), pads included, and says so in its shapes."""
    di = w[f"fc1_w.{layer}"].shape[0]
    keep = list(range(di)) if keep is None else list(keep)
    want = MK.pruned_images(w, layer, keep, fc1_rows_pad)
    assert eng.peek_shape("fc1_w", layer) == dict(rows=len(keep), cols=GEO["dim"], rows_pad=fc1_rows_pad, ld=64, ld8=0), what
    assert eng.peek_shape("fc2_w", layer) == dict(rows=GEO["dim"], cols=len(keep), rows_pad=256, ld=MK.ceil_to(len(keep), 64), ld8=0), what
    for k in FFN_KINDS:
        _same(eng.peek_tensor(k, layer), want[k], f"{what}: {k} of block {layer}")


def _prune(eng, layer, keep):
    arr = (C.c_int32 * len(keep))(*keep)
    return eng.lib.ssp2_prune_ffn(eng.h, layer, arr, len(keep))


def _prune_into(twin, eng, layer, keep):
    twin._bind_stream()
    arr = (C.c_int32 * len(keep))(*keep)
    return eng.lib.ssp2_prune_ffn_into(twin.h, eng.h, layer, arr, len(keep))


@pytest.mark.parametrize("which", ["all", "one", "64", "65", "ends on the last"])
def test_prune_in_place_gathers_rows_bias_and_columns(coded, which):
    keep = MK.keep_lists(203, seed=0)[which]
    eng = _engine(coded)
    try:
        _check_block(eng, coded, 0, None, 256, "before")
        assert _prune(eng, 0, keep) == 0
        assert eng.lib.ssp2_d_int(eng.h, 0) == len(keep)
        _check_block(eng, coded, 0, keep, 256, f"in place, keep {which}")
        _check_block(eng, coded, 1, None, 256, "the other block")
    finally:
        eng.close()


@pytest.mark.parametrize("which", ["all", "one", "64", "65", "ends on the last"])
def test_prune_into_a_twin_gathers_rows_bias_and_columns(coded, which):
    keep = MK.keep_lists(203, seed=0)[which]
    eng = _engine(coded)
    twin = eng.pruned_twin([len(keep), 72], max_images=4)
    try:
        assert _prune_into(twin, eng, 0, keep) == 0
        _check_block(twin, coded, 0, keep, MK.ceil_to(len(keep), 256), f"twin, keep {which}")
        _check_block(twin, coded, 1, None, 256, "the twin's other block (cloned)")
        _check_block(eng, coded, 0, None, 256, "the source")
    finally:
        twin.close(); eng.close()


def test_second_prune_of_a_pruned_block_counts_from_the_current_width(coded):
    first = MK.keep_lists(203, seed=0)["65"]
    second = [0, 3, 4, 31, 32, 63, 64]
    eng = _engine(coded)
    try:
        assert _prune(eng, 0, first) == 0 and _prune(eng, 0, second) == 0
        _check_block(eng, _sliced(coded, 0, first), 0, second, 256, "second prune")
        assert _prune(eng, 0, [0, 7]) == EINVAL, "7 is outside the current width"
        _check_block(eng, _sliced(coded, 0, first), 0, second, 256, "after the refused third")
    finally:
        eng.close()


def test_narrow_block_pruned_before_the_wide_one(coded):
    """The scratch of the in-place gather is allocated at the first call, for the widest block."""
    narrow, wide = list(range(1, 72, 2)), [j for j in range(203) if j % 50]
    eng = _engine(coded)
    try:
        assert _prune(eng, 1, narrow) == 0 and _prune(eng, 0, wide) == 0
        _check_block(eng, coded, 1, narrow, 256, "narrow block first")
        _check_block(eng, coded, 0, wide, 256, "wide block second")
    finally:
        eng.close()


def test_a_twin_filled_twice_keeps_no_remnant_and_a_pinned_list_may_be_rewritten_at_once(coded):
    a, b = MK.keep_lists(203, seed=0)["65"], MK.keep_lists(203, seed=7)["65"]
    assert a != b
    eng = _engine(coded)
    twin = eng.pruned_twin([65, 72], max_images=4)
    try:
        assert _prune_into(twin, eng, 0, a) == 0 and _prune_into(twin, eng, 0, b) == 0
        _check_block(twin, coded, 0, b, 256, "second fill of the twin")
        # stage_keep's contract: the list is copied before the call returns.  Work queued in front keeps the stream busy meanwhile.
        pin = torch.tensor(a, dtype=torch.int32).pin_memory()
        busy = torch.randn(2048, 2048, device=DEV)
        twin._bind_stream()
        for _ in range(8):
            busy = busy @ busy * 1e-3
        assert eng.lib.ssp2_prune_ffn_into(twin.h, eng.h, 0, C.cast(pin.data_ptr(), C.POINTER(C.c_int32)), 65) == 0
        pin.zero_()
        _check_block(twin, coded, 0, a, 256, "pinned list rewritten right after the call (twin)")
        pin.copy_(torch.tensor(b, dtype=torch.int32))
        eng._bind_stream()
        for _ in range(8):
            busy = busy @ busy * 1e-3
        assert eng.lib.ssp2_prune_ffn(eng.h, 0, C.cast(pin.data_ptr(), C.POINTER(C.c_int32)), 65) == 0
        pin.zero_()
        _check_block(eng, coded, 0, b, 256, "pinned list rewritten right after the call (in place)")
    finally:
        twin.close(); eng.close()


def test_refused_keep_lists_leave_the_images_alone(coded):
    eng = _engine(coded)
    twin = eng.pruned_twin([65, 72], max_images=4)
    good = MK.keep_lists(203, seed=0)["65"]
    try:
        assert _prune_into(twin, eng, 0, good) == 0
        for what, keep in [("not ascending", [5, 4] + good[2:]), ("repeated", [good[0]] + good[:-1]), ("out of range", good[:-1] + [203]), ("negative", [-1] + good[1:]),
                           ("n_keep is not the twin's width", good[:64])]:
            assert _prune_into(twin, eng, 0, keep) == EINVAL, what
        for what, keep in [("not ascending", [9, 3]), ("out of range", [0, 203]), ("negative", [-1, 2]), ("empty", []), ("too many", list(range(203)) + [203])]:
            assert _prune(eng, 0, keep) == EINVAL, what
        _check_block(twin, coded, 0, good, 256, "the twin after the refusals")
        _check_block(eng, coded, 0, None, 256, "the source after the refusals")
        assert eng.lib.ssp2_d_int(eng.h, 0) == 203
    finally:
        twin.close(); eng.close()


# -------------------------------------------------------------------------------------------------------------------- clone
def test_clone_copies_every_kind_of_every_layer():
    geo = MK.geometry(prefix=2, dist_head=True)
    w = MK.special_weights(geo, seed=4)
    names = MK.tensor_list(geo["depth"], True)
    eng = _engine(w)
    twin = eng.pruned_twin([203, 40], max_images=4)          # ssp2_clone_weights; block 1 differs in width
    try:
        _check_images(eng, w, names, "the source")
        for k, l in names:
            if l == 1 and k in ("fc1_w", "fc1_b", "fc2_w"):
                assert twin.peek_shape(k, l) != eng.peek_shape(k, l)
                continue
            assert twin.peek_shape(k, l) == eng.peek_shape(k, l), (k, l)
            _same(twin.peek_tensor(k, l), eng.peek_tensor(k, l), f"clone: {k} of block {l}")
    finally:
        twin.close(); eng.close()


# ---------------------------------------------------------------------------------------------------------- fp8 after a prune
GEO8 = MK.geometry(dim=128)
N8 = 58                                                      # 58 images x 5 tokens = 290 rows: a launch of at least 256


def _fp8_engine(w, n=64):
    e = _engine(w, n, precision="fp8")
    e.set_option("big_tile_min_rows", 256)
    return e


def _logits(eng, px):
    n = px.shape[0]
    x = eng.embed(px)
    eng.layers(x, n)
    return eng.head(x, n, want_logits=True)[0].cpu()


def test_fp8_images_after_a_prune_are_the_quantiser_on_the_compacted_matrices(op):
    """ld8 = ceil128(n_keep) shrinks in block 0 (203 -> 100: 256 -> 128) and stays in block 1 (72 -> 40: 128).  The e4m3 images and the
    scales equal ssp2_quantise_rows_e4m3 (tested against float64 on its own) of the host-compacted bf16 matrices over the whole
    [rows_pad, ld8]; then the pruned engine computes what a fresh fp8 engine built from the host-sliced weights computes, bit for bit."""
    w = MK.random_weights(GEO8, seed=11)
    keeps = {0: sorted(torch.randperm(203, generator=torch.Generator().manual_seed(1))[:100].tolist()),
             1: sorted(torch.randperm(72, generator=torch.Generator().manual_seed(2))[:40].tolist())}
    px = torch.randn(N8, 3, 28, 28, generator=torch.Generator().manual_seed(3)).to(DEV)
    eng = _fp8_engine(w)
    try:
        assert eng.peek_shape("fc2_w", 0)["ld8"] == 256 and eng.peek_shape("fc2_w", 1)["ld8"] == 128 and eng.peek_shape("fc1_w", 0)["ld8"] == 128
        ws = w
        for l, keep in keeps.items():
            eng.prune_ffn(l, keep)
            ws = _sliced(ws, l, keep)
        for l, keep in keeps.items():
            for kind, m in (("fc1_w", ws[f"fc1_w.{l}"]), ("fc2_w", ws[f"fc2_w.{l}"])):
                sh = eng.peek_shape(kind, l)
                assert sh["ld8"] == MK.ceil_to(m.shape[1], 128) and sh["rows"] == m.shape[0] and sh["cols"] == m.shape[1], (kind, l, sh)
                w8, sc = op.quantise_e4m3(m.to(torch.bfloat16), rows_pad=sh["rows_pad"], ld8=sh["ld8"])
                got8, gots = eng.peek_tensor(kind, l, "e4m3"), eng.peek_tensor(kind, l, "scale")
                _same(got8, w8.cpu(), f"e4m3 image of {kind}, block {l}")
                _same(gots, sc.cpu(), f"scales of {kind}, block {l}")
                assert not bool(got8[m.shape[0]:].any()) and not bool(got8[:, m.shape[1]:].any()) and bool((gots[m.shape[0]:] == 1).all())
                assert bool(got8[:m.shape[0], :m.shape[1]].any())
        got = _logits(eng, px)
        fresh = _fp8_engine(ws)
        try:
            want = _logits(fresh, px)
        finally:
            fresh.close()
        assert bool(want.isfinite().all()) and float(want.abs().max()) > 0
        _same(got, want, "logits of the pruned fp8 engine against a fresh one from the sliced weights")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------- fp8 calibration
N_CAL, G_CAL = 21, 7                                         # 3 slabs of 128 rows, 35 live each: M = 291


def _calibrate(eng, px, group, headroom=4.0):
    """begin, ssp2_embed + ssp2_layers in the layout `group`, end — the C entries, as a caller of the library's would."""
    n = px.shape[0]
    eng._bind_stream()
    eng._check(eng.lib.ssp2_fp8_calibrate_begin(eng.h))
    try:
        x = eng.embed(px, group=group)
        assert x.shape[0] == MK.layout(n, eng.tokens, group)[0] >= 256, "a launch on the e4m3 path"
        eng.layers(x, n, score_group=group)
    finally:
        eng._check(eng.lib.ssp2_fp8_calibrate_end(eng.h, headroom))
    return [float(eng.lib.ssp2_fp8_attn_scale(eng.h, l)) for l in range(eng.depth)]


def _cal_images():
    px = torch.randn(N_CAL, 3, 28, 28, generator=torch.Generator().manual_seed(21))
    many = px[torch.arange(N8) % N_CAL]                      # the same images, as many as a contiguous launch of >= 256 rows takes
    return px.to(DEV), many.to(DEV)


def test_fp8_calibration_counts_top_codes_of_the_images_only():
    """Two fc1 biases of block 1 at 600: every image row puts two bytes on the e4m3 top code, and so would the slab layout's pad rows
    (fc1 of the LayerNorm of a zero row).  Exactly 2 x images x tokens, in either layout."""
    w = MK.random_weights(GEO8, seed=12)
    b1 = w["fc1_b.1"].clone(); b1[5] = 600.0; b1[60] = 600.0
    w["fc1_b.1"] = b1
    px, many = _cal_images()
    eng = _fp8_engine(w)
    try:
        assert eng.rows(N_CAL, G_CAL) == 291 and eng.tokens == 5
        _calibrate(eng, px, G_CAL)
        slab = eng.fp8_fc2_top_codes()
        _calibrate(eng, many, 0)
        flat = eng.fp8_fc2_top_codes()
        print(f"\n[fp8 calibration] top codes: slab layout {slab} (images: {2 * N_CAL * 5}, all rows: {2 * 291}), contiguous {flat} ({2 * N8 * 5})")
        assert slab == 2 * N_CAL * 5
        assert flat == 2 * N8 * 5
    finally:
        eng.close()


def test_fp8_calibration_scale_ignores_stale_pad_rows():
    """A contiguous forward with every block's V bias at 100 leaves |o| ~ 100 in rows 35 .. 127 and 163 .. 255 of the attention output,
    which the slab layout never writes again.  The scales of a slab calibration must be those of the same images calibrated on a fresh
    engine in the contiguous layout."""
    from ssp2vit._lib import T_KINDS
    w = MK.random_weights(GEO8, seed=13)
    hot = dict(w)
    for l in range(GEO8["depth"]):
        b = w[f"qkv_b.{l}"].clone(); b[2 * 128:] = 100.0
        hot[f"qkv_b.{l}"] = b
    px, many = _cal_images()
    ref = _fp8_engine(w)
    try:
        want = _calibrate(ref, many, 0)
    finally:
        ref.close()
    eng = _fp8_engine(hot)
    try:
        x = eng.embed(many)
        eng.layers(x, N8)
        torch.cuda.synchronize()
        for l in range(GEO8["depth"]):
            t = w[f"qkv_b.{l}"].contiguous()
            eng._check(eng.lib.ssp2_load_tensor(eng.h, T_KINDS.index("qkv_b"), l, C.cast(t.data_ptr(), C.POINTER(C.c_float)), t.numel()))
        eng._check(eng.lib.ssp2_set_precision(eng.h, 1))
        got = _calibrate(eng, px, G_CAL)
        print(f"\n[fp8 calibration] scales: slab layout after a hot forward {got}, contiguous on a fresh engine {want}")
        assert all(0 < s < 16 * 1024 for s in want)
        assert got == want
    finally:
        eng.close()
