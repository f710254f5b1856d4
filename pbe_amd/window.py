"""Window planning for inpainting a region of a picture of any size (pipeline.inpaint_window): which rectangle of the picture goes
through the model.  Host side, integers only - the pixels are handled by the kernels of csrc/window.hip (ops.window_image,
ops.window_mask, ops.feather_alpha, ops.paste_window).  For one window per hole (pipeline.inpaint_holes) the planner below turns the
component table of ops.component_boxes (csrc/holes.hip) into groups with disjoint blend zones and one window per group.  shape_mask
brings a mask into the shape the model wants before anything is planned from it (csrc/maskshape.hip)."""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Sequence, Tuple

import numpy as np

from .lib import PbeError

HOLE = 128          # a mask byte >= 128 is the hole: the byte form of the (1 - v / 255) < 0.5 threshold of preprocess.load_triple
Window = Tuple[int, int, int, int]


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


def _host_mask(mask_u8) -> np.ndarray:
    if hasattr(mask_u8, "detach"):                         # a torch tensor, on any device
        mask_u8 = mask_u8.detach().cpu().numpy()
    m = np.asarray(mask_u8)
    if m.ndim != 2 or m.dtype != np.uint8 or m.size == 0:
        raise PbeError(f"plan_window: the mask must be a non-empty uint8 [Hs, Ws] array, got {m.dtype} {m.shape}")
    return m


def hole_box(mask_u8) -> Tuple[int, int, int, int]:
    """(ya, yb, xa, xb), inclusive: the bounding box of the bytes >= 128.  An empty hole raises."""
    hole = _host_mask(mask_u8) >= HOLE
    rows, cols = np.flatnonzero(hole.any(1)), np.flatnonzero(hole.any(0))
    if rows.size == 0:
        raise PbeError("plan_window: the mask has no hole (no byte >= 128): nothing to inpaint")
    return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def validate_window(window, picture_hw: Sequence[int]) -> Window:
    """window as four Python ints (y0, x0, wh, ww), or PbeError if they are not integers or not inside the Hs x Ws picture."""
    Hs, Ws = int(picture_hw[0]), int(picture_hw[1])
    try:
        vals = tuple(window)
        y0, x0, wh, ww = (int(v) for v in vals)
        ok = len(vals) == 4 and all(int(v) == v for v in vals)
    except (TypeError, ValueError) as e:
        raise PbeError(f"window: expected four integers (y0, x0, wh, ww), got {window!r}") from e
    if not ok or y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > Hs or x0 + ww > Ws:
        raise PbeError(f"window (y0, x0, wh, ww) = {window!r} is not inside the {Hs} x {Ws} picture")
    return y0, x0, wh, ww


def plan_window(mask_u8, working: Sequence[int], context=0.5, feather: int = 8, window: Optional[Sequence[int]] = None) -> Window:
    """The window (y0, x0, wh, ww) of the picture to inpaint at the working size `working` = (H, W), from the hole's bounding box
    bh x bw (rows ya .. yb, columns xa .. xb), r = feather and m = 2r + 1:

      need_h = bh + 2 max(m, ceil(context bh)), need_w likewise: the box plus `context` of its size, and never less than the width m of
               the feather (ops.feather_alpha is positive up to 2r from the hole), on each side;
      the smallest window of aspect H : W that holds need_h x need_w: (need_h, ceil(need_h W / H)) if need_h W >= need_w H, else
               (ceil(need_w H / W), need_w);
      never smaller than (H, W): the crop is not magnified when the picture allows it;
      clamped per dimension to the picture (Hs, Ws).  A picture too small in one dimension therefore gives an ANISOTROPIC window: its
               aspect is no longer H : W and the two axes are resampled by different factors (the kernels take any pair of scales);
      centred on the box: y0 = floor((ya + yb + 1 - wh) / 2) shifted into [0, Hs - wh], x0 likewise.

    So the window lies in the picture, the box lies in the window with a margin >= m on every side that is not the picture's border
    (where alpha is therefore 0), and a picture of exactly the working size gives the whole picture.  Integer arithmetic throughout
    (context is taken as the exact rational value of the float).  An empty hole raises PbeError.  `window`: a caller's own window, only
    validated (four integers inside the picture) and returned."""
    m8 = _host_mask(mask_u8)
    Hs, Ws = m8.shape
    if window is not None:
        return validate_window(window, (Hs, Ws))
    H, W = int(working[0]), int(working[1])
    r = int(feather)
    if H < 1 or W < 1 or r != feather or r < 0 or not (context >= 0) or context == float("inf"):
        raise PbeError(f"plan_window: working size {tuple(working)!r} must be positive, feather {feather!r} an integer >= 0, context {context!r} finite and >= 0")
    return plan_window_box(hole_box(m8), (Hs, Ws), working, context, feather)


def plan_window_box(box: Sequence[int], picture_hw: Sequence[int], working: Sequence[int], context=0.5, feather: int = 8) -> Window:
    """plan_window's arithmetic from the hole's bounding box (ya, yb, xa, xb), inclusive, in a picture of picture_hw = (Hs, Ws): what
    plan_window returns for a mask with that box.  plan_holes calls it once per group of holes."""
    Hs, Ws = int(picture_hw[0]), int(picture_hw[1])
    H, W = int(working[0]), int(working[1])
    r = int(feather)
    if H < 1 or W < 1 or r != feather or r < 0 or not (context >= 0) or context == float("inf"):
        raise PbeError(f"plan_window: working size {tuple(working)!r} must be positive, feather {feather!r} an integer >= 0, context {context!r} finite and >= 0")
    ya, yb, xa, xb = (int(v) for v in box)
    if not (0 <= ya <= yb < Hs and 0 <= xa <= xb < Ws):
        raise PbeError(f"plan_window: box (ya, yb, xa, xb) = {tuple(box)!r} is not inside the {Hs} x {Ws} picture")
    bh, bw, m, ctx = yb - ya + 1, xb - xa + 1, 2 * r + 1, Fraction(context)
    need_h = bh + 2 * max(m, int(-((-ctx * bh) // 1)))
    need_w = bw + 2 * max(m, int(-((-ctx * bw) // 1)))
    if need_h * W >= need_w * H:
        wh, ww = need_h, _ceil_div(need_h * W, H)
    else:
        wh, ww = _ceil_div(need_w * H, W), need_w
    wh, ww = min(max(wh, H), Hs), min(max(ww, W), Ws)
    y0 = min(max((ya + yb + 1 - wh) // 2, 0), Hs - wh)
    x0 = min(max((xa + xb + 1 - ww) // 2, 0), Ws - ww)
    return y0, x0, wh, ww


# ---- the shape of the hole (csrc/maskshape.hip): what a mask goes through before anything is planned from it ----------------------------
SHAPE_KEYS = ("open", "close", "grow", "box", "connectivity")


def shape_args(shape) -> dict:
    """The keywords of shape_mask, checked and with the defaults filled in: `shape` is a dict of some of open (>= 0), close (>= 0), grow
    (negative shrinks; all three reals up to 2047), box (a bool) and connectivity (8 or 4).  Anything else raises PbeError."""
    import numbers
    try:
        kw = dict(shape)
    except (TypeError, ValueError) as e:
        raise PbeError(f"shape_mask: expected a dict of {SHAPE_KEYS}, got {shape!r}") from e
    unknown = sorted(str(k) for k in kw if k not in SHAPE_KEYS)
    if unknown:
        raise PbeError(f"shape_mask: unknown key(s) {unknown}: the keys are {SHAPE_KEYS}")
    out = {"open": kw.get("open", 0), "close": kw.get("close", 0), "grow": kw.get("grow", 0), "box": kw.get("box", False),
           "connectivity": kw.get("connectivity", 8)}
    for k in ("open", "close", "grow"):
        v = out[k]
        lo = -2047 if k == "grow" else 0
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not (lo <= v <= 2047):
            raise PbeError(f"shape_mask: {k} must be a real number in {lo} .. 2047, got {v!r}")
    if not isinstance(out["box"], (bool, np.bool_)):
        raise PbeError(f"shape_mask: box must be True or False, got {out['box']!r}")
    if out["connectivity"] not in (4, 8):
        raise PbeError(f"shape_mask: connectivity must be 8 or 4, got {out['connectivity']!r}")
    return out


def shape_mask(mask, *, open=0, close=0, grow=0, box=False, connectivity=8):                       # noqa: A002 (the morphological names)
    """The mask in the shape the model wants: uint8 [Hs, Ws] on the GPU (a byte >= 128 is the hole) -> a NEW uint8 [Hs, Ws] in {0, 255},
    after, in this order and each only when it is not at its default,
      open   ops.mask_open(., open):   specks and spurs narrower than the disc of that radius go
      close  ops.mask_close(., close): gaps and pits narrower than the disc are filled (two fragments of one object become one hole)
      grow   ops.mask_grow(., grow):   the hole grown by the disc of that radius, a negative one shrinks it
      box    every component (ops.mask_components at `connectivity`, ops.component_boxes) replaced by its bounding box
             (ops.fill_boxes); boxes that overlap simply unite, and whoever labels afterwards sees them as one hole.
    All of it is exact integer arithmetic in Euclidean distance; the outside of the picture is neither hole nor background, so a hole
    at the border is not eroded from there.  With every stage at its default the result is the mask binarised.  The input is never
    modified; a result without a hole is not an error here (the planners raise for it)."""
    from . import ops
    a = shape_args({"open": open, "close": close, "grow": grow, "box": box, "connectivity": connectivity})
    m, staged = mask, False
    for stage, fn in (("open", "mask_open"), ("close", "mask_close"), ("grow", "mask_grow")):
        if a[stage] != 0:
            m, staged = getattr(ops, fn)(m, a[stage]), True
    if a["box"]:
        labels = ops.mask_components(m, a["connectivity"])
        try:
            _, table = ops.component_boxes(labels, capacity=4096)                                # what ops.fill_boxes takes
        except PbeError as e:
            raise PbeError(f"shape_mask: the box stage found more than 4096 components, more boxes than ops.fill_boxes takes ({e}): "
                           "remove the specks first (open=...), or close the gaps (close=...)") from e
        return ops.fill_boxes(np.asarray(table, dtype=np.int64).reshape(-1, 6)[:, 1:5], tuple(m.shape), device=m.device)
    return m if staged else ops.mask_grow(m, 0)


# ---- one window per hole (pipeline.inpaint_holes): the component table of ops.component_boxes -> groups -> windows ----------------------
def _box_gap(a, b) -> int:
    """Chebyshev distance of two inclusive boxes (ya, yb, xa, xb): per axis the index gap where they do not overlap, the larger of the two."""
    return max(a[0] - b[1], b[0] - a[1], a[2] - b[3], b[2] - a[3], 0)


def group_components(table, feather: int = 8):
    """Components whose blend zones could touch, grouped.  table: rows (label, ya, yb, xa, xb, area) of ops.component_boxes, any order.
    With r = feather and m = 2r + 1: one group per component, then any two groups whose bounding boxes have Chebyshev distance <= 2m are
    merged (box = the union), to the fixed point.  Merging only ever grows boxes, so a pair that may merge stays mergeable and every order
    of merges ends in the same partition: the finest one whose boxes lie pairwise farther apart than 2m.
    Why 2m: ops.feather_alpha is positive only within Chebyshev distance 2r of its hole.  Pixels of two groups are at least as far apart
    as their boxes, > 4r + 2, so no pixel lies within 2r of both: the alpha supports are disjoint, pasting is independent of order and no
    pixel is blended twice.
    Returns a list of (labels, box, area): labels a sorted tuple, box (ya, yb, xa, xb), ordered by the smallest label (the raster order of
    each group's first pixel)."""
    r = int(feather)
    if r != feather or r < 0:
        raise PbeError(f"group_components: feather {feather!r} must be an integer >= 0")
    rows = np.asarray(table, dtype=np.int64).reshape(-1, 6)
    if len(set(rows[:, 0].tolist())) != rows.shape[0]:
        raise PbeError("group_components: the table names a label twice")
    limit = 2 * (2 * r + 1)
    groups = [([int(l)], (int(ya), int(yb), int(xa), int(xb)), int(a)) for l, ya, yb, xa, xb, a in sorted(rows.tolist())]
    merged = True
    while merged:
        merged = False
        for i in range(len(groups)):
            j = i + 1
            while j < len(groups):
                (la, ba, aa), (lb, bb, ab) = groups[i], groups[j]
                if _box_gap(ba, bb) <= limit:
                    groups[i] = (la + lb, (min(ba[0], bb[0]), max(ba[1], bb[1]), min(ba[2], bb[2]), max(ba[3], bb[3])), aa + ab)
                    del groups[j]
                    merged, j = True, i + 1                # the grown box may now reach groups it passed
                else:
                    j += 1
    out = [(tuple(sorted(ls)), box, area) for ls, box, area in groups]
    return sorted(out, key=lambda g: g[0][0])


def plan_holes(table, picture_hw: Sequence[int], working: Sequence[int], context=0.5, feather: int = 8, max_holes: int = 16):
    """One window per group of holes: [(labels, box, window)] in group_components' order, window = plan_window_box(box, ...).  No component
    is dropped: more than `max_holes` groups raise PbeError, and so does an empty table (the error of hole_box)."""
    rows = np.asarray(table, dtype=np.int64).reshape(-1, 6)
    if rows.shape[0] == 0:
        raise PbeError("plan_window: the mask has no hole (no byte >= 128): nothing to inpaint")
    groups = group_components(rows, feather)
    if len(groups) > int(max_holes):
        raise PbeError(f"plan_holes: the mask has {len(groups)} separate holes, more than max_holes = {int(max_holes)}: raise max_holes, or use "
                       "inpaint_window, which treats them as one hole")
    return [(labels, box, plan_window_box(box, picture_hw, working, context, feather)) for labels, box, _ in groups]


# ---- the tone of a pasted window (csrc/tone.hip): one affine map per window and channel, fitted on the known pixels ---------------------
TONE_MODES = ("mean", "affine", "field")


def _f32(v) -> float:
    return float(np.float32(v))


def _tone_table(stats):
    """stats as a nested list [B][3][6] of Python ints, or PbeError."""
    if hasattr(stats, "detach"):
        stats = stats.detach().cpu()
    if hasattr(stats, "tolist"):
        stats = stats.tolist()
    try:
        table = [[[v for v in row] for row in sample] for sample in stats]
    except TypeError as e:
        raise PbeError(f"fit_tone: stats must be a [B, 3, 6] table of integers, got {stats!r}") from e
    for sample in table:
        if len(sample) != 3 or any(len(row) != 6 for row in sample):
            raise PbeError("fit_tone: stats must be a [B, 3, 6] table (per sample and channel n, So, Sq, Soo, Sqq, Soq)")
        for row in sample:
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in row):
                raise PbeError(f"fit_tone: stats must hold integers, got {row!r}")
        if len({int(row[0]) for row in sample}) != 1:
            raise PbeError(f"fit_tone: the three rows of a sample count different numbers of pixels: {[int(row[0]) for row in sample]}")
    return [[[int(v) for v in row] for row in sample] for sample in table]


def fit_tone(stats, mode: str = "affine", gain_limit: float = 1.25, min_pixels: int = 64):
    """One affine map per window and channel that brings the result's known pixels back onto the original's, from the table of
    ops.tone_stats: stats [B, 3, 6] (a host tensor, an array or a nested list; taken as Python ints), row [b, c] = n, So, Sq, Soo, Sqq,
    Soq, the sums over the counted pixels of o (the original's byte), q (the result's byte), their squares and their product.  Returns a
    list, one dict per window: {"n", "gain": [3], "offset": [3], "clamped": [3], "rms_before": [3], "rms_after": [3], "identity"}.
    Per channel, on exact integers:
      mode "affine": g = (n Soq - So Sq) / (n Sqq - Sq^2), the least-squares slope of o on q (two integers, divided once), clamped to
                     [1 / gain_limit, gain_limit] - `clamped` says whether that happened; a zero denominator (a flat result) gives g = 1;
      mode "mean":   g = 1;
      gain   = g rounded to fp32: the reported value is the applied one (ops.paste_window(tone=(gain, offset)));
      offset = (So - gain Sq) / (255 n) rounded to fp32: the least-squares offset FOR THE GAIN APPLIED, in [0, 1] units;
      rms_before = sqrt(sum (o - q)^2 / n), rms_after = sqrt(sum (o - gain q - 255 offset)^2 / n): grey levels over the counted pixels,
                   both expanded from the six sums in exact rationals.
    n < min_pixels (and n = 0 always) gives gain 1, offset 0: too little evidence changes nothing.  "identity" is True where the map
    applied is the identity in all three channels.
    DECISIONS (none of them is a measurement):
      least squares on PAIRED pixels, not moment matching (gain = sd o / sd q): it minimises what the eye sees at the seam, and texture
          noise in the result, which inflates sd q, does not inflate the gain;
      gain_limit = 1.25 by default: an autoencoder's tone drift is a few per cent; a larger gain means that the known pixels were
          redrawn, and that is not tone;
      min_pixels = 64.
    An unknown mode, gain_limit < 1 (or not finite), a table of another shape or rows of one sample with different n raise PbeError."""
    import math
    if mode == "field":
        raise PbeError("fit_tone: mode 'field' is not a fit of one map per window: pbe_amd.window.tone_field makes the difference field from the pictures themselves")
    if mode not in TONE_MODES:
        raise PbeError(f"fit_tone: mode must be one of {TONE_MODES[:2]}, got {mode!r}")
    try:
        limit = float(gain_limit)
    except (TypeError, ValueError) as e:
        raise PbeError(f"fit_tone: gain_limit must be a finite number >= 1, got {gain_limit!r}") from e
    if not (limit >= 1.0) or limit == float("inf"):
        raise PbeError(f"fit_tone: gain_limit must be a finite number >= 1, got {gain_limit!r}")
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or min_pixels < 0:
        raise PbeError(f"fit_tone: min_pixels must be an integer >= 0, got {min_pixels!r}")
    out = []
    for sample in _tone_table(stats):
        n = sample[0][0]
        fit = {"n": n, "gain": [], "offset": [], "clamped": [], "rms_before": [], "rms_after": []}
        for _, So, Sq, Soo, Sqq, Soq in sample:
            g, clamped = 1.0, False
            if mode == "affine" and n > 0 and n >= min_pixels:
                num, den = n * Soq - So * Sq, n * Sqq - Sq * Sq
                if den != 0:
                    g = num / den
                    clamped = not (1.0 / limit <= g <= limit)
                    g = min(max(g, 1.0 / limit), limit)
            gain = _f32(g)
            offset = 0.0
            if n > 0 and n >= min_pixels:
                gn, gd = gain.as_integer_ratio()
                offset = _f32((So * gd - gn * Sq) / (255 * n * gd))
            G, Bq = Fraction(gain), 255 * Fraction(offset)
            before = Fraction(Soo - 2 * Soq + Sqq, max(n, 1))
            after = (Soo + G * G * Sqq + Bq * Bq * n - 2 * G * Soq - 2 * Bq * So + 2 * G * Bq * Sq) / max(n, 1)
            fit["gain"].append(gain); fit["offset"].append(offset); fit["clamped"].append(clamped)
            fit["rms_before"].append(math.sqrt(before)); fit["rms_after"].append(math.sqrt(after))
        fit["identity"] = all(g == 1.0 for g in fit["gain"]) and all(b == 0.0 for b in fit["offset"])
        out.append(fit)
    return out


def tone_selection(mask, window, size, margin: int = 8, out=None):
    """The pixels the tone is fitted on: fp32 [1, H, W] on the device, 1 on the known working pixels that lie farther from the hole than
    `margin` WORKING pixels, else 0.  mask: uint8 [Hs, Ws] on the GPU (a byte >= 128 is the hole), window (y0, x0, wh, ww), size (H, W).
    In picture pixels the margin is r = max(ceil(margin wh / H), ceil(margin ww / W)) (integers; r > 2047 raises PbeError), and
      sel = ops.window_mask(ops.mask_grow(mask, r), window, size, out)     (the mask itself at r = 0): existing kernels only.
    DECISION: the default margin is 8 working pixels, one latent cell: nearer to the hole the decoder mixes generated content into the
    known pixels, and that is not tone."""
    from . import ops
    H, W = int(size[0]), int(size[1])
    if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or margin < 0:
        raise PbeError(f"tone_selection: margin must be an integer >= 0, got {margin!r}")
    if H < 1 or W < 1:
        raise PbeError(f"tone_selection: working size {tuple(size)!r} must be positive")
    _, _, wh, ww = validate_window(window, mask.shape[:2])
    r = max(_ceil_div(int(margin) * wh, H), _ceil_div(int(margin) * ww, W))
    if r > 2047:
        raise PbeError(f"tone_selection: a margin of {margin} working pixels is {r} picture pixels in window {tuple(window)}, more than 2047")
    return ops.window_mask(ops.mask_grow(mask, r) if r > 0 else mask, window, size, out=out)


# ---- a tone that varies across the window (csrc/tone_field.hip): a low-frequency field of the difference, added by the paste -----------
def field_levels(grid: Sequence[int]) -> int:
    """The levels of the pull-push pyramid over a grid of (Hc, Wc) cells, the table included: 1 for a 1 x 1 grid."""
    h, w, n = int(grid[0]), int(grid[1]), 1
    while h > 1 or w > 1:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def tone_field(image, result, sel, cell: int = 8, limit: float = 0.125, min_pixels: int = 64):
    """A tone that varies across the window - a vignette, a gradient the decoder flattens - as a low-frequency difference field.
    image fp32 [B, 3, H, W] is what the model saw, result fp32 [B, 3, H, W] in [0, 1] what it returned, sel fp32 [B, 1, H, W] the pixels
    to trust (tone_selection), all on the GPU.  Returns (field, cells, summary):
      cells   int32 [B, 4, Hc, Wc] = ops.tone_cells: per cell of `cell` x `cell` working pixels n and the sums of o - q per channel;
      field   fp32 [B, 3, Hc, Wc] = ops.tone_field: the pull-push fill of the cell means, in [0, 1] units, the cell means clamped to +-limit;
              ops.paste_window(..., field=field[i], cell=cell) adds it, sampled bilinearly, to the pasted window;
      summary a list, one dict per window: {"mode": "field", "n", "cell", "grid": [Hc, Wc], "levels", "offset": [3] (the pyramid's top
              mean per channel: tone="mean"'s offset, clamped to +-limit, for comparison), "field_min": [3], "field_max": [3] (grey
              levels), "identity"} - from ONE small host read (the cell sums and the field's range are reduced on the device).
    n < min_pixels (and n = 0 always) gives a field of zeros: too little evidence changes nothing.
    DECISIONS (none of them is a measurement):
      pull-push, not a harmonic (Poisson) solve: a fixed operation count, any grid size, no convergence question;
      a level trusts its own mean fully at one full finest cell of evidence: the cap is cell^2 at every level;
      limit = 0.125 is 32 grey levels: a larger local difference means that the known pixels were redrawn, and that is not tone;
      the field is additive, with gain 1; a constant difference gives exactly tone="mean"'s offset in every element.
    cell outside (4, 8, 16, 32, 64), a limit that is not finite and > 0, min_pixels < 0 and tensors of other shapes raise PbeError."""
    import torch
    from . import ops
    if isinstance(cell, bool) or cell not in ops.TONE_CELLS:
        raise PbeError(f"tone_field: cell must be one of {ops.TONE_CELLS}, got {cell!r}")
    try:
        lim = float(limit)
    except (TypeError, ValueError) as e:
        raise PbeError(f"tone_field: limit must be a finite number > 0, got {limit!r}") from e
    if not (lim > 0.0) or lim == float("inf"):
        raise PbeError(f"tone_field: limit must be a finite number > 0, got {limit!r}")
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or min_pixels < 0:
        raise PbeError(f"tone_field: min_pixels must be an integer >= 0, got {min_pixels!r}")
    cells = ops.tone_cells(image, result, sel, cell)
    field = ops.tone_field(cells, cell, lim, int(min_pixels))
    B, _, Hc, Wc = (int(v) for v in cells.shape)
    # one host read: the four whole-window sums (exact in fp64: below 2^37) and the field's range per channel
    small = torch.cat([cells.sum(dim=(2, 3), dtype=torch.int64).double(), field.amin(dim=(2, 3)).double(), field.amax(dim=(2, 3)).double()], dim=1).cpu().tolist()
    lim32 = _f32(lim)
    summary = []
    for row in small:
        n = int(row[0])
        identity = n == 0 or n < min_pixels
        offset = [0.0 if n == 0 else min(max(_f32(int(S) / (255.0 * n)), -lim32), lim32) for S in row[1:4]]
        summary.append({"mode": "field", "n": n, "cell": int(cell), "grid": [Hc, Wc], "levels": field_levels((Hc, Wc)), "offset": offset,
                        "field_min": [255.0 * v for v in row[4:7]], "field_max": [255.0 * v for v in row[7:10]], "identity": identity})
    return field, cells, summary
