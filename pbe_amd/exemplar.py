"""The exemplar cut from a picture of any size on the device.

resample_tables   Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) in float64 on the host: the per-axis filter tables the
                  kernels of csrc/exemplar.hip apply in integers, so that ops.resample_u8 gives Image.resize's bytes.
plan_crop         an object's bounding box -> the integer crop box around it (padding, squaring, kept inside the picture).
exemplar_from_picture / exemplars_from_pictures
                  a uint8 picture on the device (+ a box or an object mask) -> the CLIP-normalised exemplar planes the model takes.

Only the tables are host arithmetic (a few hundred doubles, like the prologue's divisions); every pixel is touched by HIP kernels only."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Sequence, Tuple

import numpy as np

from .lib import PbeError

PRECISION_BITS = 22                     # Pillow's 32 - 8 - 2: coefficients carry 22 fractional bits
FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "lanczos": 3.0}
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _bilinear(x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic with a = -0.5, in Pillow's expression order (each operation rounded on its own, as un-fused C doubles are)."""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: np.ndarray) -> np.ndarray:
    """Truncated sinc, through libm's sin one value at a time: numpy's vector sin may round the last bit differently."""
    flat = [(_sinc(v) * _sinc(v / 3) if -3.0 <= v < 3.0 else 0.0) for v in x.ravel().tolist()]
    return np.array(flat, dtype=np.float64).reshape(x.shape)


_KERNEL = {"bicubic": _bicubic, "bilinear": _bilinear, "lanczos": _lanczos}


def resample_tables(in_size: int, in0, in1, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """One axis of Pillow's 8-bit resize: in_size samples, the box in0 .. in1 of them, out_size outputs ->
    (bounds int32 [out, 2] of (xmin, n), coeffs int32 [out, ksize], zero past n).

    in0, in1 are rounded to fp32 first and subtracted in fp32 (Pillow parses the box as C floats).  Then, in float64:
    scale = (in1 - in0) / out, fs = max(scale, 1), support = S fs (S = 2 bicubic, 1 bilinear, 3 lanczos), ksize = ceil(support) 2 + 1; per
    output i: center = in0 + (i + 0.5) scale, xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in_size) -
    xmin, weights f((x + xmin - center + 0.5) (1 / fs)) summed in index order and divided by the sum, each rounded to
    int(+-0.5 + w 2^22) with the sign of w (int() truncates)."""
    if filter not in _KERNEL:
        raise PbeError(f"resample_tables: filter must be one of {sorted(_KERNEL)}, got {filter!r}")
    in_size, out_size = int(in_size), int(out_size)
    a0, a1 = np.float32(in0), np.float32(in1)
    if in_size < 1 or out_size < 1 or not (0.0 <= float(a0) < float(a1) <= in_size):
        raise PbeError(f"resample_tables: box {in0!r} .. {in1!r} must be non-empty and inside 0 .. {in_size}, sizes >= 1 (out {out_size})")
    scale = float(np.float32(a1 - a0)) / out_size
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = float(a0) + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    n = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = np.where(live, _KERNEL[filter](((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                              # cumsum adds in index order (np.sum is pairwise); + 0.0 past n changes nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS)))
    coeffs = np.where(live, k, 0.0).astype(np.int32)
    return np.stack([xmin, n], 1).astype(np.int32), np.ascontiguousarray(coeffs)


def vertical_first(Hs: int, Ws: int, oh: int) -> bool:
    """Image.resize's rule (the Python layer of Pillow 12.2, Image.py; older releases lack it): a picture more than 100 times as tall as wide whose height shrinks is resized in two
    calls, the height over the full width first, then the width.  Everywhere else the horizontal pass runs first.  The byte intermediate
    makes the order visible in the result, so ops.resample_u8 follows it."""
    return int(Hs) > int(Ws) * 100 and int(oh) < int(Hs)


def identity_tables(size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The tables of a pass that copies: (i, 1) and the coefficient 1.0 = 2^22."""
    i = np.arange(int(size), dtype=np.int32)
    return np.stack([i, np.ones_like(i)], 1), np.full((int(size), 1), 1 << PRECISION_BITS, dtype=np.int32)


def validate_box(box, picture_hw: Sequence[int]) -> Tuple[float, float, float, float]:
    """Pillow's box (x0, y0, x1, y1), floats allowed, as its resize checks it: no negative offset, inside the picture, not empty.
    None is the whole picture.  Returned as the fp32 values Pillow works with."""
    Hs, Ws = int(picture_hw[0]), int(picture_hw[1])
    if box is None:
        return 0.0, 0.0, float(Ws), float(Hs)
    try:
        vals = tuple(float(np.float32(v)) for v in box)
    except (TypeError, ValueError) as e:
        raise PbeError(f"box: expected four numbers (x0, y0, x1, y1), got {box!r}") from e
    if len(vals) != 4 or not all(math.isfinite(v) for v in vals):
        raise PbeError(f"box: expected four finite numbers (x0, y0, x1, y1), got {box!r}")
    x0, y0, x1, y1 = vals
    if x0 < 0 or y0 < 0:
        raise PbeError(f"box {box!r}: the offset can't be negative")
    if x1 > Ws or y1 > Hs:
        raise PbeError(f"box {box!r} exceeds the {Hs} x {Ws} picture")
    if x1 - x0 <= 0 or y1 - y0 <= 0:
        raise PbeError(f"box {box!r} is empty")
    return vals


def plan_crop(box, picture_hw: Sequence[int], pad=0.0, square: bool = False) -> Tuple[int, int, int, int]:
    """An object's inclusive box (ya, yb, xa, xb) in an Hs x Ws picture -> the integer crop (x0, y0, x1, y1), exclusive ends (Pillow's).

    Integers throughout; `pad` enters as the nearest rational with a denominator up to 2^20 (0.1 is 1 / 10, not the double next to it, so
    that 0.1 of 10 pixels is 1 pixel and not 2).  Per axis, with b = the box's extent:
      1. grow:    p = ceil(pad b) pixels on each side (rounded up: the crop never holds less than the asked margin);
      2. square:  the shorter extent is grown to the longer, d = long - short more pixels, d // 2 before and d - d // 2 after (the odd
                  pixel goes to the far side: the centre moves by half a pixel at most), but never beyond the picture's extent on that
                  axis - in a picture narrower than the object is tall the crop is the full width and not square;
      3. fit:     an extent larger than the picture's is clipped to it; otherwise a crop that sticks out is SHIFTED inside, size kept.
    So the crop lies inside the picture, holds the grown box wherever the picture does, and is square whenever the picture's shorter
    edge allows."""
    Hs, Ws = int(picture_hw[0]), int(picture_hw[1])
    try:
        vals = tuple(box)
        ya, yb, xa, xb = (int(v) for v in vals)
        ok = len(vals) == 4 and all(int(v) == v for v in vals)
    except (TypeError, ValueError) as e:
        raise PbeError(f"plan_crop: expected four integers (ya, yb, xa, xb), got {box!r}") from e
    if not ok or not (0 <= ya <= yb < Hs and 0 <= xa <= xb < Ws):
        raise PbeError(f"plan_crop: box (ya, yb, xa, xb) = {box!r} is not inside the {Hs} x {Ws} picture")
    try:
        fr = Fraction(pad).limit_denominator(1 << 20)
    except (TypeError, ValueError, OverflowError) as e:
        raise PbeError(f"plan_crop: pad must be a finite number >= 0, got {pad!r}") from e
    if fr < 0:
        raise PbeError(f"plan_crop: pad must be a finite number >= 0, got {pad!r}")
    lo, hi = [ya, xa], [yb + 1, xb + 1]
    for a in (0, 1):
        p = math.ceil(fr * (hi[a] - lo[a]))
        lo[a], hi[a] = lo[a] - p, hi[a] + p
    if square:
        ext = [hi[0] - lo[0], hi[1] - lo[1]]
        s = 0 if ext[0] < ext[1] else 1                                  # the shorter axis
        d = min(ext[1 - s], (Hs, Ws)[s]) - ext[s]
        if d > 0:
            lo[s], hi[s] = lo[s] - d // 2, hi[s] + (d - d // 2)
    for a, size in ((0, Hs), (1, Ws)):
        if hi[a] - lo[a] >= size:
            lo[a], hi[a] = 0, size
        elif lo[a] < 0:
            lo[a], hi[a] = 0, hi[a] - lo[a]
        elif hi[a] > size:
            lo[a], hi[a] = lo[a] - (hi[a] - size), size
    return lo[1], lo[0], hi[1], hi[0]


def _fill3(fill):
    if fill is None:
        return None
    try:
        vals = tuple(int(v) for v in fill)
        ok = len(vals) == 3 and all(int(v) == v and 0 <= int(v) <= 255 for v in fill)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise PbeError(f"fill must be three bytes (R, G, B), got {fill!r}")
    return vals


def exemplar_from_picture(picture_u8, box=None, mask=None, pad=0.0, square: bool = False, fill=None, size: int = 224, filter: str = "bicubic"):
    """A uint8 [Hs, Ws, 3] picture on the device -> {'ref': fp32 [1, 3, size, size] CLIP-normalised, 'u8': uint8 [size, size, 3],
    'box': the (x0, y0, x1, y1) that was cut}, all by the kernels of csrc/exemplar.hip: the bytes Pillow's
    Image.resize((size, size), filter, box=box) gives, the planes ops.u8_to_planes gives of them.

    box   Pillow's (x0, y0, x1, y1).  Without pad / square it is taken as it is (floats allowed); with either it must be integral and
          goes through plan_crop as the object's box.  None with a mask: the mask's bounding box (ops.mask_box) through plan_crop.
          None without a mask: the whole picture - then 'ref' is load_triple's exemplar bit for bit.
    mask  uint8 [Hs, Ws] on the device, a byte >= 128 is the object.  It places the crop when no box is given, and with `fill`
          (three bytes) every pixel off the object reads as that colour: the background is blanked before the filter sees it."""
    from . import ops
    if getattr(picture_u8, "dim", lambda: 0)() != 3:
        raise PbeError("exemplar_from_picture: expected a uint8 [Hs, Ws, 3] picture on the GPU")
    hw = (int(picture_u8.shape[0]), int(picture_u8.shape[1]))
    fill = _fill3(fill)
    if fill is not None and mask is None:
        raise PbeError("exemplar_from_picture: fill needs a mask (it colours the pixels off the object)")
    if mask is not None and tuple(mask.shape) != hw:
        raise PbeError(f"exemplar_from_picture: the mask is {tuple(mask.shape)}, the picture {hw}")
    planned = bool(square) or pad != 0
    if box is None and mask is not None:
        obj = ops.mask_box(mask)
        if obj is None:
            raise PbeError("exemplar_from_picture: the mask has no object (no byte >= 128)")
        box = plan_crop(obj, hw, pad, square)
    elif box is not None and planned:
        x0, y0, x1, y1 = validate_box(box, hw)
        if any(int(v) != v for v in (x0, y0, x1, y1)):
            raise PbeError(f"exemplar_from_picture: pad / square plan an integer crop: the box {box!r} must be integral")
        box = plan_crop((int(y0), int(y1) - 1, int(x0), int(x1) - 1), hw, pad, square)
    elif box is None and planned:
        raise PbeError("exemplar_from_picture: pad / square need a box or a mask to grow")
    size = int(size)
    u8, planes = ops.resample_u8(picture_u8, (size, size), box=box, filter=filter, mask=mask if fill is not None else None, fill=fill,
                                 mean=CLIP_MEAN, std=CLIP_STD)
    cut = tuple(int(v) if float(v).is_integer() else v for v in validate_box(box, hw))       # as Pillow takes it: fp32 values, integers as ints
    return {"ref": planes[None], "u8": u8, "box": cut}


def exemplars_from_pictures(pictures, boxes=None, masks=None, **kw):
    """pictures[b][k]: the k-th exemplar picture of sample b (uint8 [Hs, Ws, 3] on the device, any sizes); boxes / masks: the same nesting
    or None -> {'ref': fp32 [B, K, 3, size, size], 'u8': uint8 [B, K, size, size, 3], 'boxes': [[box]]}.  kw: exemplar_from_picture's."""
    import torch
    if not pictures or any(len(row) != len(pictures[0]) or not row for row in pictures):
        raise PbeError("exemplars_from_pictures: expected B lists of the same K >= 1 pictures")
    for name, nest in (("boxes", boxes), ("masks", masks)):
        if nest is not None and (len(nest) != len(pictures) or any(len(r) != len(pictures[0]) for r in nest)):
            raise PbeError(f"exemplars_from_pictures: {name} must be nested like the pictures")
    out = [[exemplar_from_picture(p, box=None if boxes is None else boxes[b][k], mask=None if masks is None else masks[b][k], **kw)
            for k, p in enumerate(row)] for b, row in enumerate(pictures)]
    return {"ref": torch.stack([torch.cat([e["ref"] for e in row]) for row in out]), "u8": torch.stack([torch.stack([e["u8"] for e in row]) for row in out]),
            "boxes": [[e["box"] for e in row] for row in out]}
