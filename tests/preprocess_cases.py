"""TEST INFRASTRUCTURE — cases, images and the integer restatement of the device input pipeline (csrc/preproc.hip.h, pil_coeffs of
csrc/engine.hip, ssp2vit/preprocess.py).  Never imported by the product path.

Shared by tests/test_preprocess_statements_cpu.py (which proves the restatement on the CPU: byte for byte against arrays recorded from
Pillow itself, tests/golden/preprocess_pil_axes.npz and preprocess_pil.npz, and against live Pillow where it is importable) and
tests/test_preprocess_numerics_gpu.py (which holds the two kernels and the wrapper to it).

Resize.  Pillow's 8-bit `Image.resize(..., BICUBIC)` is two separable integer passes, the horizontal one first, with an 8-bit rounded and
clipped image between them.  Along one axis of `in` pixels resampled to `out`:
    scale = in / out, filterscale = max(scale, 1), support = 2 * filterscale, ksize = ceil(support) * 2 + 1
    center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) - xmin
    w[x] = bicubic((x + xmin - center + 0.5) * (1 / filterscale)), a = -0.5, x < xmax; the sum taken in index order; w[x] / sum
    k[x] = int(+-0.5 + w[x] * 2^22), the sign of the half that of w[x]  (C's conversion truncates, as Python's int does)
    pixel = clip((2^21 + sum_x byte[xmin + x] * k[x]) >> 22, 0, 255)  with an arithmetic shift (floor, as numpy's >> on int64)
Pillow multiplies by the reciprocal of filterscale, and so does `coeffs` (a division need not round alike on a down-scale).  Both Pillow
and the kernels accumulate in a 32-bit int: `resample` proves per call that no prefix of any sum can leave that range
(2^21 + 255 * sum |k| < 2^31 for every output position), so that int64 here and int there are the same integers.

ToTensor + Normalize.  `to_tensor_normalize` is torchvision's arithmetic in torch CPU fp32 ops: `.to(float32).div(255)`, then
`.sub(mean).div(std)` with mean and std float32 tensors made from the Python floats; a flip mirrors the RESIZED image.

Very tall images.  Pillow's Python `Image.resize` (12.2, which recorded the fixtures) runs the VERTICAL pass first when height > 100 * width and the height
shrinks; the two orders differ in the 8-bit image between them.  The device pipeline is horizontal-first at every geometry, as `resize`
is, so for such inputs it is not Pillow's result: `pillow_runs_vertical_first` names them, GpuPreprocessor refuses them, and the one
such geometry here (1200x8 -> 224, which is there for the size of its horizontal launch) is held to `resize`, not to Pillow.

Images (`images`): uniform random bytes with the lower half of the rows replaced by 0 / 255 noise — next to a 255 a bicubic up-scale
overshoots below 0 beside it and above 255 on it, so both clips occur; `clip_counts` counts them per pass.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

PRECISION_BITS = 22                                                   # Pillow: 32 - 8 - 2
GRID_LIMIT = 65536 * 256                                              # elements one trip of either kernel's grid covers

# ---------------------------------------------------------------------------------------------------------------- the case lists
# one axis, (in, out): recorded from Pillow on 6-line strips, once per pass
AXIS_PAIRS = [(32, 224), (32, 384), (32, 518), (96, 96), (224, 224), (256, 224), (300, 224), (375, 384), (500, 384), (1000, 32),
              (1200, 224), (64, 32), (1, 32), (2, 37), (3, 37), (7, 518)]
# strips in which no sum leaves [0, 255]: the identity's coefficient is exactly 2^22 on one byte, a one-pixel axis has one coefficient
# of 2^22, and 1000 -> 32 averages 125 bytes per output (the noise lines' means stay far inside the range).  The milder down-scales
# (1200 -> 224, 64 -> 32) do clip on the noise lines.
AXIS_NO_CLIP = {(96, 96), (224, 224), (1, 32), (1000, 32)}
# both passes, (h, w, out): recorded from Pillow on three whole images each
FULL_CASES = [(2, 3, 37), (1, 1, 32), (40, 48, 96), (64, 64, 32)]
FULL_NO_CLIP = {(1, 1, 32)}                                            # one pixel: every output is that pixel
# the geometries of the live cross-check (h, w, out), beside the seeded random ones
LIVE_GEOMETRIES = [(32, 32, 224), (32, 32, 384), (32, 32, 518), (500, 375, 384), (1000, 37, 32), (1, 1, 32), (2, 3, 37), (224, 224, 224),
                   (7, 300, 518), (96, 96, 96), (64, 64, 32), (40, 48, 224), (256, 300, 224), (300, 8, 224)]

# GPU cases: name -> (n, h, w, out, flip).  flip: None, or the images that are mirrored.
# The two large ones are the smallest that take a thread of one kernel round its loop a second time (`grid_trips`):
#   vertical pass    n * 3 * out^2 > 16 777 216:  38 * 3 * 384^2 = 16 809 984, 37 give 16 367 616; the horizontal pass has 1 400 832
#   horizontal pass  n * h * out * 3 > 16 777 216:  21 * 1200 * 224 * 3 = 16 934 400, 20 give 16 128 000; the vertical pass has 3 161 088
GPU_CASES: Dict[str, Tuple[int, int, int, int, Optional[Tuple[int, ...]]]] = {
    "grid-stride vertical": (38, 32, 32, 384, (0, 37)),
    "grid-stride horizontal": (21, 1200, 8, 224, None),
    "32x32->384": (2, 32, 32, 384, None),
    "32x32->518": (1, 32, 32, 518, None),
    "500x375->384": (1, 500, 375, 384, None),
    "224x224->224": (1, 224, 224, 224, None),
    "96x96->96": (2, 96, 96, 96, None),
    "64x64->32": (2, 64, 64, 32, None),
    "1000x37->32": (1, 1000, 37, 32, None),
    "7x300->518": (1, 7, 300, 518, None),
    "2x3->37": (2, 2, 3, 37, None),
    "1x1->32": (2, 1, 1, 32, None),
}
LARGE_CASES = ("grid-stride vertical", "grid-stride horizontal")
SIZE_CASES = tuple(k for k in GPU_CASES if k not in LARGE_CASES)
IDENTITY_CASES = ("224x224->224", "96x96->96")
# which passes of a GPU case clip both ways (0: horizontal, 1: vertical).  Not listed: both.  The identity passes copy and a one-pixel
# axis is constant; in 64x64->32 and 1000x37->32 the vertical pass averages the horizontal pass's already averaged bytes (64 -> 32 leaves
# a few above 255 and none below 0, 1000 -> 32 none at all), so only their horizontal passes (64 -> 32, 37 -> 32) clip both ways.
CLIPPING_PASSES = {"224x224->224": (), "96x96->96": (), "1x1->32": (), "64x64->32": (0,), "1000x37->32": (0,)}
# flip geometry: height, width and output size all differ, so a mirror indexed by the wrong one of them lands elsewhere.  (The bicubic
# filter is symmetric: mirroring the source and resizing gives the mirrored result, so WHICH image is mirrored cannot show in the values;
# that the mirror is taken at the output's width, per image, of the float result only, can.)
FLIP_CASE = (5, 24, 40, 56)                                            # n, h, w, out

# statistics sets (mean, std) of Normalize
STATS = {
    "half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "clip": ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
    "distinct": ((0.1, 0.45, 0.8), (0.2, 0.5, 1.25)),                 # no two channels alike: a swapped select cannot pass
}


# --------------------------------------------------------------------------------------------------------------- the statement
def bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def coeffs(in_size: int, out_size: int):
    """-> (bounds int64 [out, 2] = (xmin, count), kk int64 [out, ksize] zero past count, ksize)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    kk = np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        assert 0 < cnt <= ksize, (in_size, out_size, xx, cnt, ksize)
        w = [bicubic((x + xmin - center + 0.5) * inv) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, cnt)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk, ksize


def resample_raw(img_u8: np.ndarray, axis: int, out: int) -> np.ndarray:
    """(2^21 + sum byte * k) >> 22 along `axis`, int64, before the clip."""
    img_u8 = np.asarray(img_u8)
    assert img_u8.dtype == np.uint8
    a = np.moveaxis(img_u8, axis, 0)
    bounds, kk, _ = coeffs(a.shape[0], out)
    half = 1 << (PRECISION_BITS - 1)
    assert half + 255 * int(np.abs(kk).sum(axis=1).max()) < 2 ** 31, "a 32-bit accumulator could overflow on some image"
    res = np.empty((out,) + a.shape[1:], dtype=np.int64)
    for xx in range(out):
        x0, cnt = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = np.tensordot(kk[xx, :cnt], a[x0:x0 + cnt].astype(np.int64), axes=(0, 0)) + half
        assert int(np.abs(ss).max()) < 2 ** 31
        res[xx] = ss >> PRECISION_BITS
    return np.moveaxis(res, 0, axis)


def resample(img_u8: np.ndarray, axis: int, out: int) -> np.ndarray:
    """One pass of Pillow's 8-bit resampler along `axis` (any array of bytes)."""
    return np.ascontiguousarray(np.clip(resample_raw(img_u8, axis, out), 0, 255).astype(np.uint8))


def resize(img: np.ndarray, out: int) -> np.ndarray:
    """uint8 [n, h, w, c] (or [h, w, c]) -> [n, out, out, c]: the horizontal pass, then the vertical one on its 8-bit result."""
    img = np.asarray(img)
    return resample(resample(img, img.ndim - 2, out), img.ndim - 3, out)


def pillow_runs_vertical_first(h: int, w: int, out: int) -> bool:
    """The geometries at which Pillow 12's Image.resize swaps the passes (see the module docstring)."""
    return h > 100 * w and out < h


def clip_counts(img: np.ndarray, out: int):
    """((below 0, above 255) of the horizontal pass, the same of the vertical pass) for uint8 [n, h, w, c]"""
    r0 = resample_raw(img, img.ndim - 2, out)
    r1 = resample_raw(np.clip(r0, 0, 255).astype(np.uint8), img.ndim - 3, out)
    return tuple((int((r < 0).sum()), int((r > 255).sum())) for r in (r0, r1))


def to_tensor_normalize(u8_nhwc, mean: Sequence[float], std: Sequence[float], hflip=None) -> torch.Tensor:
    """uint8 [n, S, S', 3], already resized -> float32 [n, 3, S, S']: ToTensor, Normalize, images with a non-zero hflip mirrored."""
    t = torch.from_numpy(np.array(u8_nhwc)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor([float(v) for v in std], dtype=torch.float32).view(1, 3, 1, 1)
    t = t.sub(m).div(s)
    if hflip is not None:
        for i, f in enumerate(np.asarray(hflip).reshape(-1)):
            if f:
                t[i] = t[i].flip(-1)
    return t


def normalize_table(mean: Sequence[float], std: Sequence[float]) -> torch.Tensor:
    """float32 [256, 3]: every byte value through `to_tensor_normalize`, per channel."""
    u8 = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None, None], 3, axis=3)      # [1, 256, 1, 3]
    return to_tensor_normalize(u8, mean, std)[0, :, :, 0].t().contiguous()


# ---------------------------------------------------------------------------------------------------------------------- images
def images(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """n distinct uint8 [h, w, 3] images: uniform bytes in the upper rows, 0 / 255 noise in the rows from h // 2 on (h = 1: uniform)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    if h > 1:
        img[:, h // 2:] = rng.integers(0, 2, size=(n, h - h // 2, w, 3), dtype=np.uint8) * 255
    return img


def all_bytes_image() -> np.ndarray:
    """uint8 [1, 16, 16, 3]: every channel holds all 256 byte values, each in an order of its own."""
    v = np.arange(256, dtype=np.int64)
    img = np.stack([(v * m + o) % 256 for m, o in ((1, 0), (77, 85), (171, 170))], axis=-1).astype(np.uint8)       # odd multipliers: bijections
    assert all(len(set(img[:, c].tolist())) == 256 for c in range(3))
    return img.reshape(1, 16, 16, 3)


def grid_trips(total: int) -> int:
    """Trips round the grid-stride loop that the busiest thread of a launch over `total` elements makes."""
    return -(-total // GRID_LIMIT)


@functools.lru_cache(maxsize=None)
def gpu_case(name: str):
    """-> dict(images, out, flip uint8 [n] or None, tmp (the 8-bit image between the passes), u8 (`resize`)).  Computed once per
    process; the arrays are read-only."""
    n, h, w, out, flipped = GPU_CASES[name]
    img = images(n, h, w, seed=1000 + list(GPU_CASES).index(name))
    tmp = resample(img, 2, out)
    u8 = resample(tmp, 1, out)
    flip = None
    if flipped is not None:
        flip = np.zeros(n, dtype=np.uint8)
        flip[list(flipped)] = 1
    for a in (img, tmp, u8) + ((flip,) if flip is not None else ()):
        a.setflags(write=False)
    return dict(images=img, out=out, flip=flip, tmp=tmp, u8=u8)


def mismatches_by_image_and_channel(got: torch.Tensor, want: torch.Tensor) -> str:
    """For float32 [n, 3, H, W] compared as bits: '' when equal, else which (image, channel) planes differ and in how many elements."""
    bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    if not bool(bad.any()):
        return ""
    per = bad.flatten(2).sum(-1)
    where = [(int(i), int(c), int(per[i, c])) for i, c in per.nonzero().tolist()]
    first = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} of {bad.numel()} elements differ; (image, channel, count): {where[:12]}{' ...' if len(where) > 12 else ''}; first at {first}"
