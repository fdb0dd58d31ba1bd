"""The restatements of tests/misc_kernel_cases.py, proved without a GPU: against float64 and torch CPU, on the very inputs
tests/test_misc_kernels_gpu.py hands to the kernels.  Every exact comparison is also shown to NOTICE the defect it is there for: a
wrong segment, a keep list shifted by one neuron, truncation instead of round-to-nearest-even, a pad that is not zero, another
association of the group sum."""
import numpy as np
import pytest
import torch

import misc_kernel_cases as MK

U = MK.U


# ------------------------------------------------------------------------------------------------------------------ row layout
@pytest.mark.parametrize("tokens,n,group,ld", MK.FUSED_CASES)
def test_layout_is_the_librarys_row_count_and_slabs_are_tile_aligned(tokens, n, group, ld):
    from ssp2vit.engine import ssp2_rows
    rows, first = MK.layout(n, tokens, group)
    assert rows == ssp2_rows(n, tokens, group)
    own = MK.row_owner(n, tokens, group)
    assert int((own >= 0).sum()) == n * tokens and [int(np.argmax(own == s)) for s in range(n)] == first
    if 0 < group < n:
        assert all(first[s] % 128 == 0 for s in range(0, n, group)), "every slab starts on a tile"
        if (group * tokens) % 128:
            assert int((own[:first[group]] < 0).sum()) == first[group] - group * tokens > 0, "pad rows between the slabs"
    assert MK.slab_tiles(n, tokens, group) * 128 >= rows


def test_fused_cases_cover_what_they_are_for():
    per = {c: MK.sample_entries(c[1], c[0], c[2]) for c in MK.FUSED_CASES}
    assert all(e == [(s, 0)] for s, e in enumerate(per[(128, 5, 0, 64)])), "128 tokens: one tile per image, segment 1 never used"
    assert {len(e) for e in per[(577, 3, 0, 64)]} == {5, 6}
    assert {len(e) for e in per[(577, 5, 2, 64)]} <= {5, 6}
    for c, ents in per.items():
        if c[0] != 128 and c[2] != 1:                # (one image per slab: every image starts its own tile)
            assert {seg for e in ents for _, seg in e} == {0, 1}, c
    grp = MK.group_of(37, 18)
    assert grp >= 16 and grp % 16 and 37 % grp == 1, "a 16-wide step, its tail and a one-image group"
    assert max(MK.slab_tiles(n, t, g) * 2 * ld * 4 for t, n, g, ld in MK.FUSED_CASES) < 100 * 1024


# ----------------------------------------------------------------------------------------------------------- fused score finish
@pytest.mark.parametrize("tokens,n,group,ld", MK.FUSED_CASES)
def test_finish_of_the_slab_is_the_per_sample_column_norm(tokens, n, group, ld):
    """The restatement is right: a slab built in float64 from activations laid out per ssp2_rows, finished, gives the direct norms."""
    g = torch.Generator().manual_seed(tokens + n)
    act = torch.randn(n, tokens, 8, generator=g, dtype=torch.float64) * torch.tensor([1e-3, 1, 1, 30, 1, 1, 1e3, 1], dtype=torch.float64)
    slab = MK.slab_from_activations(act, group)
    assert slab.shape[0] == MK.slab_tiles(n, tokens, group)
    out, norms = MK.finish_fused_f64(slab, n, tokens, group, 0)
    direct = (act ** 2).sum(1).sqrt()
    torch.testing.assert_close(norms, direct, rtol=1e-13, atol=0)
    grp = MK.group_of(n, group)
    want = torch.stack([direct[k * grp:(k + 1) * grp].sum(0) for k in range(-(-n // grp))])
    torch.testing.assert_close(out, want, rtol=1e-13, atol=0)
    # every live entry of the slab is read exactly once, by the image it belongs to
    seen = torch.zeros(slab.shape[:2])
    for ent in MK.sample_entries(n, tokens, group):
        for t, seg in ent:
            seen[t, seg] += 1
    assert bool(((seen == 1) == (slab.abs().sum(-1) > 0)).all()) and int(seen.max()) == 1


@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("i", range(len(MK.FUSED_CASES)))
def test_exact_slabs_are_exact_and_a_wrong_segment_shows(i, chain):
    tokens, n, group, ld = MK.FUSED_CASES[i]
    slab = MK.exact_slab(n, tokens, group, ld, seed=i)
    assert slab.unique().numel() == slab.numel() and float(slab.min()) == 1.0
    assert float(slab.max()) * MK.tiles_per_sample(n, tokens, group) < 2 ** 24, "every per-image sum is an exact fp32 integer"
    out, norms = MK.finish_fused(slab, n, tokens, group, chain)
    out64, norms64 = MK.finish_fused_f64(slab, n, tokens, group, chain)
    want_norm = norms64.float() if not chain else norms64.float()
    assert torch.equal(norms, want_norm), "norm = float32(sqrt(float64(exact sum))), then the chain's rounding"
    # the group sum is fp32 in image order: within (group - 1) u of float64 (positive terms), and exactly the sequential fp32 sum
    torch.testing.assert_close(out.double(), out64, rtol=(MK.group_of(n, group) + 1) * U if not chain else 2.0 ** -8, atol=0)
    bad, bad_norms = MK.finish_fused(slab, n, tokens, group, chain, wrong_segment=True)
    assert bool((bad_norms != norms).any(1).all()), "one wrong segment moves every image's norms"
    assert bool((bad != out).any(1).all()), "... and every group's sums"


@pytest.mark.parametrize("i", range(len(MK.FUSED_CASES)))
def test_realistic_slabs_the_fp32_statement_stays_inside_the_bounds_the_gpu_is_held_to(i):
    """rtol = (tiles per image + group + 2) u on the fp32 chain: a sequential fp32 sum of positive terms is within (count - 1) u of the
    exact one, the root halves the relative error of its operand and adds one rounding.  On the bf16 chain the fp32 statement is within
    1 bf16 ulp of the float64 one, element by element, on these inputs."""
    tokens, n, group, ld = MK.FUSED_CASES[i]
    slab = MK.realistic_slab(n, tokens, group, ld, seed=100 + i)
    assert float(slab.min()) > 0 and float(slab.max() / slab.min()) > 1e5
    rtol = (MK.tiles_per_sample(n, tokens, group) + MK.group_of(n, group) + 2) * U
    out, norms = MK.finish_fused(slab, n, tokens, group, 0)
    out64, norms64 = MK.finish_fused_f64(slab, n, tokens, group, 0)
    assert float(((out.double() - out64).abs() / out64).max()) <= rtol and float(((norms.double() - norms64).abs() / norms64).max()) <= rtol
    out, norms = MK.finish_fused(slab, n, tokens, group, 1)
    out64, norms64 = MK.finish_fused_f64(slab, n, tokens, group, 1)
    assert int(MK.bf16_ulps_apart(norms, norms64).max()) <= 1 and int(MK.bf16_ulps_apart(out, out64).max()) <= 1
    print(f"\n[fused finish {MK.FUSED_CASES[i]}] bf16 chain: {int((MK.bf16_ulps_apart(out, out64) > 0).sum())} of {out.numel()} sums and "
          f"{int((MK.bf16_ulps_apart(norms, norms64) > 0).sum())} of {norms.numel()} norms one ulp from float64")


# ----------------------------------------------------------------------------------------------------------- stand-alone route
def test_act_l2_cases_cover_what_they_are_for():
    toks = {c[0] for c in MK.ACT_L2_CASES}
    assert {1, 2, 7, 50, 129, 197, 257, 577} <= toks
    assert {c[2] for c in MK.ACT_L2_CASES if c[1] == 70} == {1, 3, 29, 33, 64, 0}
    assert {(c[3], c[4]) for c in MK.ACT_L2_CASES} == {(64, 64), (64, 200), (64, 512), (200, 200), (200, 512)}
    assert all(c[4] % 8 == 0 and c[4] >= c[3] for c in MK.ACT_L2_CASES)


@pytest.mark.parametrize("i", range(len(MK.ACT_L2_CASES)))
def test_act_l2_statement_against_float64_and_its_association_matters(i):
    tokens, n, group, d, ld = MK.ACT_L2_CASES[i]
    act = MK.act_l2_input(tokens, n, ld, seed=i)
    assert torch.equal(act.to(torch.bfloat16).float(), act) and float(act.abs().max()) <= 8 and bool((act[:, :, d:] != 0).any() or ld == d)
    want64 = MK.act_l2_f64(act, group)
    out = MK.act_l2_statement(act, group, 0)
    err = ((out.double() - want64).abs() / want64.clamp_min(1e-300))
    assert float(err.max()) <= (MK.group_of(n, group) + 4) * U
    out1 = MK.act_l2_statement(act, group, 1)
    assert torch.equal(out1.to(torch.bfloat16).float(), out1)
    if MK.group_of(n, group) >= 29:
        # the lanes' order is part of the statement: the plain image-order sum gives other bits somewhere
        nrm = MK.sqrt_f32((act.double() ** 2).sum(1).float())
        grp = MK.group_of(n, group)
        seq = torch.zeros(ld)
        for s in range(min(n, grp)):
            seq = seq + nrm[s]
        assert bool((seq != out[0]).any())


# ------------------------------------------------------------------------------------------------------------------- ingest
def test_rne_bits_is_torchs_bf16_cast_and_truncation_shows():
    vals = torch.cat([MK.special_values((4096,), seed=s) for s in range(4)] + [torch.randn(4096)])
    u = MK.f32_bits(vals)
    for b in MK.SPECIAL_BITS:
        assert (u == b).any(), hex(int(b))
    want = MK.bf16_bits(vals.to(torch.bfloat16))
    got = MK.rne_bits(u)
    nan = np.isnan(vals.numpy())
    assert nan.sum() >= 5 and ((got[nan] & 0x7fff) > 0x7f80).all() and ((want[nan] & 0x7fff) > 0x7f80).all()
    assert (got[~nan] == want[~nan]).all()
    # what the values are there for
    f = lambda bits: int(MK.rne_bits(np.array([bits], dtype=np.uint32))[0])
    assert f(0x3f808000) == 0x3f80 and f(0x3f818000) == 0x3f82 and f(0x3f807fff) == 0x3f80 and f(0x3f808001) == 0x3f81
    assert f(0x7f7fffff) == 0x7f80 and f(0xff7fffff) == 0xff80 and f(0x00000001) == 0 and f(0x80000001) == 0x8000 and f(0x00008000) == 0
    assert f(0x00018000) == 0x0002
    trunc = MK.rne_bits(u, truncate=True)
    assert (trunc[~nan] != want[~nan]).sum() > 1000, "truncation instead of round-to-nearest-even is noticed"
    img = MK.matrix_image(vals[:60].reshape(6, 10), 256, 64)
    assert not bool(MK.differs(img, img.clone()).any())
    t_img = torch.from_numpy(trunc[:60].view(np.int16).copy()).view(torch.bfloat16).reshape(6, 10)
    assert bool(MK.differs(img[:6, :10], t_img).any())
    assert int(MK.differs(MK.matrix_image(vals[:60].reshape(6, 10), 256, 64, zero_pad=False), img).sum()) == 1, "a pad that is not zero is noticed"


def test_differs_compares_nan_as_nan_and_everything_else_by_bits():
    a = torch.tensor([0.0, -0.0, MK.NAN, 1.0, float("inf")])
    b = torch.tensor([-0.0, -0.0, MK.NAN, 1.0, float("-inf")])
    b.view(torch.int32)[2] = 0x7f800001            # another NaN payload
    assert MK.differs(a, b).tolist() == [True, False, False, False, True]
    assert MK.differs(a.to(torch.bfloat16), b.to(torch.bfloat16)).tolist() == [True, False, False, False, True]


@pytest.mark.parametrize("dist", [False, True])
def test_special_weights_reach_every_kind_and_every_matrix_edge(dist):
    geo = MK.geometry(depth=5, d_int=(203, 72, 64, 65, 130), prefix=2 if dist else 1, dist_head=dist)
    names = MK.tensor_list(geo["depth"], dist)
    assert len(names) > 64 and len(set(names)) == len(names)
    kinds = [k for k, _ in names[:64]]
    assert any(a in MK.MATRIX_KINDS and b not in MK.MATRIX_KINDS and c in MK.MATRIX_KINDS for a, b, c in zip(kinds, kinds[1:], kinds[2:]))
    w = MK.special_weights(geo, seed=1)
    assert set(MK.key_of(k, l) for k, l in names) == set(MK.tensor_shapes(geo))
    assert w["patch_w"][0].numel() == 588 and 588 % 8 and 203 % 8, "an 8-column chunk straddles the matrix's edge"
    w2 = MK.special_weights(geo, seed=2)
    for k, l in names:
        key = MK.key_of(k, l)
        assert bool(MK.differs(w[key], w2[key]).any()), key
        sh = MK.fresh_shape(k, w[key])
        img = MK.expected_image(k, w[key], sh)
        if k in MK.MATRIX_KINDS:
            assert img.shape == (sh["rows_pad"], sh["ld"]) and not bool(img[sh["rows"]:].float().abs().nan_to_num(1).any())
            got = MK.rne_bits(MK.f32_bits(w[key].reshape(sh["rows"], -1)))
            ref = MK.bf16_bits(img[:sh["rows"], :sh["cols"]])
            nan = np.isnan(w[key].reshape(sh["rows"], -1).numpy())
            assert (got[~nan] == ref[~nan]).all()


# --------------------------------------------------------------------------------------------------------------- compaction
def test_coded_ffn_describes_itself_and_a_shifted_keep_list_shows():
    geo = MK.geometry()
    w = MK.coded_ffn(geo, MK.random_weights(geo, seed=3))
    for l, di in enumerate(geo["d_int"]):
        for key in (f"fc1_w.{l}", f"fc2_w.{l}", f"fc1_b.{l}", f"fc2_b.{l}"):
            t = w[key]
            assert torch.equal(t.to(torch.bfloat16).float(), t) and bool(t.isfinite().all()) and t.unique().numel() == t.numel() and float(t.min()) > 0
        lists = MK.keep_lists(di, seed=l) if di > 65 else {"some": list(range(3, di, 2))}
        for name, keep in lists.items():
            assert keep == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < di
            good = MK.pruned_images(w, l, keep, MK.ceil_to(di, 256))
            assert good["fc2_w"].shape == (256, MK.ceil_to(len(keep), 64)) and good["fc1_w"].shape == (MK.ceil_to(di, 256), 64)
            assert int((good["fc1_w"] != 0).sum()) == len(keep) * 64 and int((good["fc2_w"] != 0).sum()) == len(keep) * 64
            if len(keep) < di:
                bad = MK.pruned_images(w, l, keep, MK.ceil_to(di, 256), shift=1)
                for k in ("fc1_w", "fc1_b", "fc2_w"):
                    assert bool(MK.differs(good[k], bad[k]).any()), (name, k)
    kl = MK.keep_lists(203, seed=0)
    assert [len(kl[k]) for k in ("all", "one", "64", "65")] == [203, 1, 64, 65] and kl["ends on the last"][-1] == 202


# ----------------------------------------------------------------------------------------------------- the two additive entries
def test_new_entries_check_their_arguments_before_the_device():
    """No GPU here: every refusal below is decided on the host (the pointers are dummies)."""
    import ctypes as C
    from ssp2vit import _lib
    lib = _lib.load()
    P = C.c_void_p(4096)

    def fin(slab=P, n=3, tokens=197, group=0, ld=64, chain=0, norms=P, out=P, stride=64):
        return lib.ssp2_score_finish(None, slab, n, tokens, group, ld, chain, norms, out, stride)
    for what, kw in [("tokens < 128", dict(tokens=127)), ("ld < 1", dict(ld=0)), ("out_stride < ld", dict(stride=63)), ("null slab", dict(slab=None)),
                     ("null norms", dict(norms=None)), ("null out", dict(out=None)), ("n", dict(n=0)), ("group", dict(group=-2)), ("chain", dict(chain=3))]:
        assert fin(**kw) == -1, what
        assert lib.ssp2_last_error()
    assert lib.ssp2_act_l2_accum(None, P, 0, 4, 7, 64, 64, 0, 2, P, P, 63) == -1 and b"out_stride" in lib.ssp2_last_error()
    assert lib.ssp2_peek_tensor(None, 0, 0, 1, P, 16) == -1
