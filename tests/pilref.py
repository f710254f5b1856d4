"""Pillow's 8-bit resize restated in numpy (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal pass, the byte
intermediate, the vertical pass, the passes it skips), the mask / fill composition of pbe_amd/csrc/exemplar.hip and the case lists of
tests/test_exemplar_cpu.py and tests/test_exemplar_gpu.py.  Not a conftest: plain functions only.

Everything here is written independently of pbe_amd/exemplar.py (python floats and loops, not numpy vectors) so that the comparison of the
two tables is a comparison of two derivations.  The arithmetic:

  in0, in1 are C floats (Pillow parses the box as four floats): scale = (double)(in1 - in0) / out, fs = max(scale, 1), support = S fs,
  ksize = ceil(support) 2 + 1; per output i: center = in0 + (i + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
  n = min((int)(center + support + 0.5), in_size) - xmin, w_x = f((x + xmin - center + 0.5) (1 / fs)), normalised by their sum in index order,
  k_x = (int)(+-0.5 + w_x 2^22); a pass gives clip((2^21 + sum_x byte_x k_x) >> 22, 0, 255) per byte, the shift arithmetic.
The horizontal pass runs first, over the rows the vertical pass reads, and its bytes are the vertical pass's input - except where
tall_first() holds (Image.resize's own rule for very tall pictures), where the vertical pass runs first over the full width.
"""
from __future__ import annotations

import math
import os

import numpy as np

PRECISION_BITS = 22
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "lanczos": 3.0}
FILTERS = ("bicubic", "bilinear", "lanczos")
HOLE = 128


def _bilinear(x: float) -> float:
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


KERNEL = {"bicubic": _bicubic, "bilinear": _bilinear, "lanczos": _lanczos}


def tables(in_size: int, in0, in1, out_size: int, filt: str):
    """(bounds int32 [out, 2] of (xmin, n), coeffs int32 [out, ksize] zero past n)."""
    f, in0, in1 = KERNEL[filt], np.float32(in0), np.float32(in1)
    scale = float(np.float32(in1 - in0)) / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, coeffs = np.zeros((out_size, 2), dtype=np.int32), np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / fs
    for i in range(out_size):
        center = float(in0) + (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, n)
        for x, v in enumerate(w):
            coeffs[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coeffs


def apply_pass(src: np.ndarray, bounds: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """One pass along axis 1 of src uint8 [rows, n_in, 3] -> uint8 [rows, out, 3]."""
    ksize = coeffs.shape[1]
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(ksize)[None], src.shape[1] - 1)        # taps past n carry coefficient 0
    acc = np.full((src.shape[0], bounds.shape[0], 3), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for k in range(ksize):
        acc += src[:, idx[:, k], :].astype(np.int64) * coeffs[None, :, k, None].astype(np.int64)
    assert np.abs(acc).max() < 2 ** 31, "a sum leaves int32: Pillow's accumulator would wrap"
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def compose(picture: np.ndarray, mask=None, fill=None) -> np.ndarray:
    """The picture the resampler reads: where the mask byte is < 128 the pixel is `fill` (three bytes)."""
    if mask is None:
        return picture
    out = picture.copy()
    out[mask < HOLE] = np.asarray(fill, dtype=np.uint8)
    return out


def needs(size_in, size_out, lo, hi) -> bool:
    """Pillow's need_horizontal / need_vertical: the pass is skipped when the sizes agree and the box spans the axis."""
    return size_out != size_in or float(np.float32(lo)) != 0.0 or float(np.float32(hi)) != size_out


def tall_first(Hs: int, Ws: int, oh: int) -> bool:
    return Hs > Ws * 100 and oh < Hs


def resize(picture: np.ndarray, out_hw, box=None, filt: str = "bicubic", mask=None, fill=None) -> np.ndarray:
    """Image.fromarray(picture).resize((ow, oh), filter, box=box) as uint8 [oh, ow, 3]."""
    src = compose(picture, mask, fill)
    Hs, Ws = src.shape[:2]
    oh, ow = int(out_hw[0]), int(out_hw[1])
    x0, y0, x1, y1 = (0, 0, Ws, Hs) if box is None else box
    need_h, need_v = needs(Ws, ow, x0, x1), needs(Hs, oh, y0, y1)
    bh, kh = tables(Ws, x0, x1, ow, filt)
    bv, kv = tables(Hs, y0, y1, oh, filt)
    first, last = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
    if tall_first(Hs, Ws, oh) and need_h:
        # Image.resize (its Python layer, as of Pillow 12.2) resizes a picture more than 100 times as tall as wide, when its height shrinks, in two
        # calls: the height over the full width, then the width - the one case in which the vertical pass runs first
        src = apply_pass(src.transpose(1, 0, 2), bv, kv).transpose(1, 0, 2)
        return np.ascontiguousarray(apply_pass(src, bh, kh))
    if need_h:
        bv = bv.copy()
        bv[:, 0] -= first
        src = apply_pass(src[first:last], bh, kh)
    if need_v:
        src = apply_pass(src.transpose(1, 0, 2), bv, kv).transpose(1, 0, 2)
    return np.ascontiguousarray(src)


def pillow(picture: np.ndarray, out_hw, box=None, filt: str = "bicubic") -> np.ndarray:
    from PIL import Image
    f = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "lanczos": Image.LANCZOS}[filt]
    return np.array(Image.fromarray(picture).resize((int(out_hw[1]), int(out_hw[0])), f, box=box), dtype=np.uint8)


def mask_box(mask: np.ndarray):
    """(ya, yb, xa, xb) inclusive of the bytes >= 128, or None."""
    ys, xs = np.nonzero(mask >= HOLE)
    return None if ys.size == 0 else (int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max()))


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "examples")
JPEGS = tuple(f"reference_example_{i}.jpg" for i in (1, 2, 3))
RANDOM_HW = ((7, 5), (37, 53), (224, 224), (300, 224), (225, 1000), (640, 481), (8, 1200))
SOURCES = JPEGS + tuple(f"random_{h}x{w}" for h, w in RANDOM_HW)
OUTPUTS = ((224, 224), (17, 9))
_cache = {}


def random_picture(hw, seed: int) -> np.ndarray:
    """Smooth structure plus noise plus saturated patches: the bicubic and lanczos overshoot has something to clip."""
    rng = np.random.default_rng(seed)
    h, w = hw
    a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    a[: h // 3, : w // 2] = 255
    a[h // 2:, w // 3: w // 3 + max(w // 4, 1)] = 0
    return a


def source(name: str) -> np.ndarray:
    """uint8 [H, W, 3], read-only, computed once."""
    if name not in _cache:
        if name in JPEGS:
            from PIL import Image
            a = np.array(Image.open(os.path.join(GOLDEN, name)).convert("RGB"), dtype=np.uint8)
        else:
            h, w = (int(v) for v in name.split("_")[1].split("x"))
            a = random_picture((h, w), 1000 * h + w)
        a.setflags(write=False)
        _cache[name] = a
    return _cache[name]


def boxes(hw):
    """whole, integral with a margin, fractional, an interior integral box: (x0, y0, x1, y1)."""
    H, W = hw
    return (None, (1, 2, W - 1, H - 1), (0.25, 0.5, W - 0.75, H - 1.5), (W // 4, H // 4, W - W // 4, H - H // 3))


def cases(name: str):
    """(box, out_hw, filter) of every case of one source."""
    hw = source(name).shape[:2]
    return [(b, o, f) for b in boxes(hw) for o in OUTPUTS for f in FILTERS]


def random_mask(hw, seed: int) -> np.ndarray:
    """uint8 [H, W]: an ellipse of 255 with a rim of 128 and 127, noise below 128 outside."""
    h, w = hw
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    d = ((yy - 0.45 * h) / (0.3 * h + 1)) ** 2 + ((xx - 0.55 * w) / (0.35 * w + 1)) ** 2
    m = rng.integers(0, 128, size=(h, w), dtype=np.uint8)
    m[d < 1.2] = 127
    m[d < 1.0] = 128
    m[d < 0.8] = 255
    return m
