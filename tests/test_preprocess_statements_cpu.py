"""Proves tests/preprocess_cases.py on the CPU: the integer restatement of Pillow's 8-bit bicubic resampler equals arrays recorded from
Pillow itself byte for byte (tests/golden/preprocess_pil_axes.npz: every axis pair once per pass, four whole two-pass cases; and the three
cases of preprocess_pil.npz), equals live Pillow where Pillow is importable, and the cases the GPU module runs have the properties that
module relies on (which launch takes a second trip round the loop, where the 8-bit clip occurs, that the Normalize tables are monotone).
The golden tests never skip."""
import os

import numpy as np
import pytest
import torch

import preprocess_cases as PC
from conftest import GOLDEN


@pytest.fixture(scope="module")
def axes():
    return dict(np.load(os.path.join(GOLDEN, "preprocess_pil_axes.npz")))


def _diff(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} bytes differ, first at {np.argwhere(bad)[:4].tolist()}"


def test_golden_file_holds_every_listed_case_and_the_pillow_version(axes):
    assert str(axes["pillow_version"]).split(".")[0].isdigit()
    want = {"pillow_version"}
    for a, b in PC.AXIS_PAIRS:
        want |= {f"axis.{a}.{b}.{k}" for k in ("in", "h", "v")}
        assert axes[f"axis.{a}.{b}.in"].shape == (6, a, 3) and axes[f"axis.{a}.{b}.h"].shape == (6, b, 3) and axes[f"axis.{a}.{b}.v"].shape == (b, 6, 3)
    for h, w, s in PC.FULL_CASES:
        want |= {f"full.{h}.{w}.{s}.{k}" for k in ("in", "out")}
        assert axes[f"full.{h}.{w}.{s}.in"].shape == (3, h, w, 3) and axes[f"full.{h}.{w}.{s}.out"].shape == (3, s, s, 3)
    assert set(axes) == want
    assert os.path.getsize(os.path.join(GOLDEN, "preprocess_pil_axes.npz")) < 300 * 1024


@pytest.mark.parametrize("pair", PC.AXIS_PAIRS, ids=lambda p: f"{p[0]}->{p[1]}")
def test_one_pass_equals_pillow_on_every_axis_pair(axes, pair):
    a, b = pair
    strip = axes[f"axis.{a}.{b}.in"]
    assert strip[0:2].std() > 50 and set(np.unique(strip[2:4]).tolist()) <= {0, 255} and not strip[4].any() and (strip[5] == 255).all()
    got_h = PC.resample(strip, 1, b)
    _diff(got_h, axes[f"axis.{a}.{b}.h"], f"horizontal pass {a} -> {b}")
    _diff(PC.resample(np.ascontiguousarray(strip.transpose(1, 0, 2)), 0, b), axes[f"axis.{a}.{b}.v"], f"vertical pass {a} -> {b}")
    assert not got_h[4].any() and (got_h[5] == 255).all(), "constant lines stay constant: every row of coefficients sums to 2^22 closely enough"
    raw = PC.resample_raw(strip[:4], 1, b)
    lo, hi = int((raw < 0).sum()), int((raw > 255).sum())
    if pair in PC.AXIS_NO_CLIP:
        assert lo == 0 and hi == 0, "listed as a strip without clips"
    else:
        assert lo > 0 and hi > 0, f"{a} -> {b}: {lo} sums below 0 and {hi} above 255"


@pytest.mark.parametrize("case", PC.FULL_CASES, ids=lambda c: f"{c[0]}x{c[1]}->{c[2]}")
def test_two_passes_equal_pillow(axes, case):
    h, w, s = case
    imgs = axes[f"full.{h}.{w}.{s}.in"]
    _diff(PC.resize(imgs, s), axes[f"full.{h}.{w}.{s}.out"], f"{h}x{w} -> {s}")
    _diff(PC.resize(imgs[1], s), axes[f"full.{h}.{w}.{s}.out"][1], "a single [h, w, c] image")
    (l0, h0), (l1, h1) = PC.clip_counts(imgs[:2], s)
    if case in PC.FULL_NO_CLIP:
        assert l0 + h0 + l1 + h1 == 0
    else:
        assert l0 + l1 > 0 and h0 + h1 > 0


def test_statement_equals_the_fixture_of_the_parity_test():
    z = dict(np.load(os.path.join(GOLDEN, "preprocess_pil.npz")))
    for tag in ("cifar", "nonsquare", "down"):
        _diff(PC.resize(z[f"{tag}.in"], 224), z[f"{tag}.out"], tag)


def test_statement_equals_live_pillow():
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(5)
    geos = list(PC.LIVE_GEOMETRIES) + [tuple(int(v) for v in rng.integers(1, 65, size=3)) for _ in range(40)]
    for h, w, s in geos:
        img = PC.images(1, h, w, seed=h * 10007 + w * 101 + s)[0]
        want = np.asarray(Image.fromarray(img).resize((s, s), Image.BICUBIC))
        _diff(PC.resize(img, s), want, f"{h}x{w} -> {s}")


def test_live_pillow_on_a_very_tall_image_is_one_of_the_two_pass_orders():
    """height > 100 * width, shrinking: Pillow 12.2 resamples vertically first (an older one may not).  Either way it is the proven
    one-axis statement applied twice; which order is printed.  Every other geometry of this suite is outside that rule."""
    pytest.importorskip("PIL")
    import PIL
    from PIL import Image
    h, w, s = 1200, 8, 224
    assert PC.pillow_runs_vertical_first(h, w, s)
    assert not any(PC.pillow_runs_vertical_first(*g) for g in PC.LIVE_GEOMETRIES + PC.FULL_CASES)
    assert [k for k, (n, gh, gw, gs, _) in PC.GPU_CASES.items() if PC.pillow_runs_vertical_first(gh, gw, gs)] == ["grid-stride horizontal"]
    img = PC.images(1, h, w, seed=3)[0]
    live = np.asarray(Image.fromarray(img).resize((s, s), Image.BICUBIC))
    h_first, v_first = PC.resize(img, s), PC.resample(PC.resample(img, 0, s), 1, s)
    assert (h_first != v_first).any()
    order = "vertical first" if np.array_equal(live, v_first) else "horizontal first" if np.array_equal(live, h_first) else None
    print(f"\n[preprocess] Pillow {PIL.__version__} on {h}x{w} -> {s}: {order}")
    assert order is not None


def test_coefficient_tables():
    for a, b in PC.AXIS_PAIRS:
        bounds, kk, ksize = PC.coeffs(a, b)
        assert kk.shape == (b, ksize) and bounds.shape == (b, 2)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= a).all() and (bounds[:, 1] <= ksize).all()
        assert all(not kk[xx, bounds[xx, 1]:].any() for xx in range(b)), "zero past the window"
        assert int(np.abs(kk.sum(1) - (1 << 22)).max()) <= ksize, "a row sums to 2^22 up to one rounding per coefficient"
    assert PC.coeffs(1200, 224)[2] == 23 and PC.coeffs(1000, 32)[2] == 127 and PC.coeffs(32, 384)[2] == 5 and PC.coeffs(500, 384)[2] == 7
    for n in (96, 224):                                       # identity: one coefficient of exactly 2^22 on the pixel itself
        bounds, kk, _ = PC.coeffs(n, n)
        for xx in range(n):
            row = np.zeros(n, dtype=np.int64)
            row[bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = kk[xx, :bounds[xx, 1]]
            assert row[xx] == 1 << 22 and not np.delete(row, xx).any()
    b1, k1, _ = PC.coeffs(1, 32)
    assert (b1 == (0, 1)).all() and (k1[:, 0] == 1 << 22).all()
    b2, _, _ = PC.coeffs(2, 37)
    assert (b2[:, 0] == 0).all() and (b2[:, 1] == 2).all(), "both ends clamp on a two-pixel axis"


def test_resample_refuses_what_a_32_bit_accumulator_could_not_hold(monkeypatch):
    big = np.full((1, 4), 1 << 23, dtype=np.int64)
    monkeypatch.setattr(PC, "coeffs", lambda a, b: (np.array([[0, 4]], dtype=np.int64), big, 4))
    with pytest.raises(AssertionError):
        PC.resample_raw(np.full((2, 4), 255, dtype=np.uint8), 1, 1)


def test_gpu_cases_reach_what_they_are_for():
    trips = {}
    for name, (n, h, w, s, _) in PC.GPU_CASES.items():
        trips[name] = (PC.grid_trips(n * h * s * 3), PC.grid_trips(n * 3 * s * s))
    assert trips["grid-stride vertical"] == (1, 2) and trips["grid-stride horizontal"] == (2, 1)
    assert all(t == (1, 1) for k, t in trips.items() if k not in PC.LARGE_CASES)
    n, h, w, s, flipped = PC.GPU_CASES["grid-stride vertical"]
    assert PC.grid_trips((n - 1) * 3 * s * s) == 1 and flipped == (0, n - 1), "one image fewer stays in one trip"
    assert PC.GRID_LIMIT // (s * s) == 3 * (n - 1) + 2, "the second trip starts inside the last image's last channel"
    n, h, w, s, _ = PC.GPU_CASES["grid-stride horizontal"]
    assert PC.grid_trips((n - 1) * h * s * 3) == 1 and PC.coeffs(h, s)[2] == 23
    for name in PC.LARGE_CASES:
        imgs = PC.gpu_case(name)["images"]
        assert len({im.tobytes() for im in imgs}) == len(imgs), "distinct images"
    nf, hf, wf, sf = PC.FLIP_CASE
    assert len({hf, wf, sf}) == 3, "a flip indexed by the input's width or height instead of the output's lands elsewhere"
    u8 = PC.resize(PC.images(nf, hf, wf, seed=77), sf)
    assert all((u8[i] != u8[i, :, ::-1]).any() and (u8[i] != u8[i, ::-1]).any() for i in range(nf)), "no image is its own mirror"


@pytest.mark.parametrize("name", list(PC.GPU_CASES))
def test_gpu_case_references_clip_where_the_table_says(name):
    c = PC.gpu_case(name)
    counts = PC.clip_counts(c["images"], c["out"])
    passes = PC.CLIPPING_PASSES.get(name, (0, 1))
    for p in passes:
        assert counts[p][0] > 0 and counts[p][1] > 0, (name, p, counts)
    if not passes:
        assert counts == ((0, 0), (0, 0))
    if name in PC.IDENTITY_CASES:
        assert np.array_equal(c["u8"], c["images"])
    assert c["u8"].shape == (c["images"].shape[0], c["out"], c["out"], 3) and np.array_equal(c["u8"], PC.resize(c["images"], c["out"]))
    with pytest.raises(ValueError):
        c["u8"][0, 0, 0, 0] = 1                               # shared, so read-only


@pytest.mark.parametrize("stats", list(PC.STATS))
def test_normalize_table_is_finite_and_strictly_increasing(stats):
    mean, std = PC.STATS[stats]
    t = PC.normalize_table(mean, std)
    assert t.shape == (256, 3) and t.dtype == torch.float32 and bool(t.isfinite().all())
    assert bool((t[1:] > t[:-1]).all())
    m32, s32 = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    for v in (0, 1, 127, 128, 254, 255):
        for c in range(3):
            assert t[v, c].item() == ((torch.tensor(float(v), dtype=torch.float32) / 255 - m32[c]) / s32[c]).item()
    exact = (torch.arange(256, dtype=torch.float64)[:, None] / 255 - torch.tensor(mean, dtype=torch.float64)) / torch.tensor(std, dtype=torch.float64)
    assert float((t.double() - exact).abs().max()) <= 4 * 2.0 ** -24 * float(exact.abs().max().clamp_min(1.0)) / min(std), "three fp32 roundings"


def test_to_tensor_normalize_flips_the_resized_image_and_all_bytes_image_is_complete():
    img = PC.all_bytes_image()
    assert img.shape == (1, 16, 16, 3) and np.array_equal(PC.resize(img, 16), img)
    two = np.concatenate([img, img[:, ::-1].copy()])
    mean, std = PC.STATS["distinct"]
    plain = PC.to_tensor_normalize(two, mean, std)
    table = PC.normalize_table(mean, std)
    for c in range(3):
        assert torch.equal(plain[0, c], table[torch.as_tensor(img[0, :, :, c].astype(np.int64)), c])
    for flip in (np.array([0, 1], dtype=np.uint8), np.array([0, 255], dtype=np.uint8), np.array([False, True])):
        f = PC.to_tensor_normalize(two, mean, std, flip)
        assert torch.equal(f[0], plain[0]) and torch.equal(f[1], plain[1].flip(-1)) and not torch.equal(f[1], plain[1])
