"""The shape of a mask in numpy: what pbe_amd/csrc/maskshape.hip (ops.mask_dist2, ops.mask_grow, ops.mask_close, ops.mask_open,
ops.fill_boxes) and pbe_amd.window.shape_mask must give, restated independently of both.  Everything is an integer: the tests compare
by equality.

  dist2_brute      the definition: the minimum over the list of set pixels
  dist2_ref        two column sweeps and a minimum over shifted rows (what the larger shapes use; test_maskshape_cpu.py proves the two equal)
  grow_ref ...     the operations built on it
Also the cases the GPU tests run (DIST2_CASES, GROW_CASES) and the wrong maps (DIST2_FAULTS, GROW_FAULTS) which test_maskshape_cpu.py
requires those cases to tell from the reference.  Not a test file and not a conftest: plain functions only."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import holesref as hr

HOLE = 128
BIG = 1 << 40


def the_set(mask, to_hole, hole=HOLE):
    """bool [Hs, Ws]: the pixels the distance is taken to - the hole pixels (to_hole) or the others.  Only pixels of the picture."""
    m = np.asarray(mask) >= hole
    return m if to_hole else ~m


# ---- the distance map ------------------------------------------------------------------------------------------------------------------
def dist2_brute_full(s):
    """int64 [Hs, Ws]: min over the set pixels (y', x') of (y - y')^2 + (x - x')^2, BIG for an empty set.  No saturation."""
    s = np.asarray(s, dtype=bool)
    Hs, Ws = s.shape
    ys, xs = np.nonzero(s)
    out = np.full((Hs, Ws), BIG, dtype=np.int64)
    yy, xx = np.mgrid[0:Hs, 0:Ws].astype(np.int64)
    step = max(1, (1 << 22) // (Hs * Ws))
    for a in range(0, ys.size, step):
        dy = yy[None] - ys[a:a + step, None, None]
        dx = xx[None] - xs[a:a + step, None, None]
        out = np.minimum(out, (dy * dy + dx * dx).min(0))
    return out


def dist2_brute(s, rmax):
    return np.minimum(dist2_brute_full(s), rmax * rmax + 1)


def column_counts(s, cap, sweeps=("down", "up")):
    """int64 [Hs, Ws]: rows to the nearest set pixel of the same column, in the directions of `sweeps`, saturated at cap."""
    s = np.asarray(s, dtype=bool)
    Hs, Ws = s.shape
    g = np.full((Hs, Ws), cap, dtype=np.int64)
    for sweep in sweeps:
        d = np.full(Ws, cap, dtype=np.int64)
        for y in (range(Hs) if sweep == "down" else range(Hs - 1, -1, -1)):
            d = np.where(s[y], 0, np.minimum(d + 1, cap))
            g[y] = np.minimum(g[y], d)
    return g


def dist2_ref(s, rmax, *, sweeps=("down", "up"), taps=None, sat=None, metric="euclid"):
    """int64 [Hs, Ws] = min(dist2_brute_full(s), rmax^2 + 1) by a column pass and a minimum over rows shifted by dx = -rmax .. rmax,
    columns from outside the picture holding rmax + 1.  The keywords exist for the faults below and are never given by the reference."""
    s = np.asarray(s, dtype=bool)
    Hs, Ws = s.shape
    cap = rmax + 1
    g = column_counts(s, cap, sweeps)
    sat = rmax * rmax + 1 if sat is None else sat
    best = np.full((Hs, Ws), sat, dtype=np.int64)
    reach = min(rmax if taps is None else taps, Ws - 1)
    for dx in range(-reach, reach + 1):
        sh = np.full((Hs, Ws), cap, dtype=np.int64)
        if dx >= 0:
            sh[:, dx:] = g[:, :Ws - dx]
        else:
            sh[:, :Ws + dx] = g[:, -dx:]
        if metric == "euclid":
            v = dx * dx + sh * sh
        elif metric == "chebyshev":
            v = np.maximum(abs(dx), sh) ** 2
        else:
            v = (abs(dx) + sh) ** 2
        v = np.where(sh >= cap, sat, v)                        # a saturated count says only "farther than rmax"
        best = np.minimum(best, v)
    return best


def mask_dist2_ref(mask, to_hole, rmax):
    return dist2_ref(the_set(mask, to_hole), rmax)


# ---- grow, close, open, boxes ----------------------------------------------------------------------------------------------------------
def radius(r):
    """(floor(r^2), ceil(|r|)) of the exact value of r."""
    f = Fraction(r)
    return int(f * f // 1), int(-((-abs(f)) // 1))


def grow_ref(mask, r, dist2=mask_dist2_ref):
    """uint8 {0, 255}: r >= 0 the pixels with dist2(to the hole) <= floor(r^2), r < 0 those with dist2(to the rest) > floor(r^2)."""
    t2, rmax = radius(r)
    if Fraction(r) >= 0:
        return np.where(dist2(mask, True, rmax) <= t2, 255, 0).astype(np.uint8)
    return np.where(dist2(mask, False, rmax) > t2, 255, 0).astype(np.uint8)


def close_ref(mask, r, grow=grow_ref):
    return grow(grow(mask, r), -Fraction(r))


def open_ref(mask, r, grow=grow_ref):
    return grow(grow(mask, -Fraction(r)), r)


def fill_boxes_ref(boxes, shape):
    out = np.zeros(shape, dtype=np.uint8)
    for ya, yb, xa, xb in np.asarray(boxes, dtype=np.int64).reshape(-1, 4).tolist():
        out[ya:yb + 1, xa:xb + 1] = 255
    return out


def shape_mask_ref(mask, open=0, close=0, grow=0, box=False, connectivity=8):                      # noqa: A002
    m = np.asarray(mask)
    if open != 0:
        m = open_ref(m, open)
    if close != 0:
        m = close_ref(m, close)
    if grow != 0:
        m = grow_ref(m, grow)
    if box:
        return fill_boxes_ref(hr.boxes_ref(hr.label_ref(m, connectivity))[:, 1:5], m.shape)
    return grow_ref(m, 0)


# ---- wrong maps the case lists must catch ----------------------------------------------------------------------------------------------
def _padded(mask, to_hole, rmax, value):
    """The map of the mask inside a frame of `value` bytes rmax + 1 wide, cut back to the picture: the outside takes part."""
    p = rmax + 1
    big = np.pad(np.asarray(mask), p, constant_values=value)
    return mask_dist2_ref(big, to_hole, rmax)[p:-p, p:-p]


DIST2_FAULTS = {
    "the square (Chebyshev) element": lambda m, t, r: dist2_ref(the_set(m, t), r, metric="chebyshev"),
    "city-block distance": lambda m, t, r: dist2_ref(the_set(m, t), r, metric="cityblock"),
    "the outside of the picture counted as hole": lambda m, t, r: _padded(m, t, r, 255),
    "the outside of the picture counted as background": lambda m, t, r: _padded(m, t, r, 0),
    "a cap of rmax^2": lambda m, t, r: np.minimum(dist2_ref(the_set(m, t), r), r * r),
    "a column pass swept down only": lambda m, t, r: dist2_ref(the_set(m, t), r, sweeps=("down",)),
    "a column pass swept up only": lambda m, t, r: dist2_ref(the_set(m, t), r, sweeps=("up",)),
    "a row pass that stops one tap early": lambda m, t, r: dist2_ref(the_set(m, t), r, taps=r - 1),
    "the threshold applied at 127": lambda m, t, r: dist2_ref(the_set(m, t, 127), r),
    "the threshold applied at 129": lambda m, t, r: dist2_ref(the_set(m, t, 129), r),
}


def _strict(mask, r):
    """`<` in place of `<=` (and `>=` in place of `>` when shrinking)."""
    t2, rmax = radius(r)
    if Fraction(r) >= 0:
        return np.where(mask_dist2_ref(mask, True, rmax) < t2, 255, 0).astype(np.uint8)
    return np.where(mask_dist2_ref(mask, False, rmax) >= t2, 255, 0).astype(np.uint8)


GROW_FAULTS = {"`<` in place of `<=`": _strict, **{k: functools.partial(grow_ref, dist2=f) for k, f in DIST2_FAULTS.items()}}


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------------
SHAPES = hr.SHAPES                                             # (1, 300), (300, 1), (90, 130), (129, 257), (67, 1031)
RMAX = (0, 1, 2, 7, 33)
BEYOND = [((90, 130), 300), ((1, 300), 300)]                   # the radius exceeds the picture: the staged apron falls off both ends
DIST2_CASES = [(p, s, r) for p in hr.PATTERNS for s in SHAPES for r in RMAX] + [(p, s, r) for p in hr.PATTERNS for s, r in BEYOND]

GROW_R = (0, 1, 1.5, 2, 3, 7, 16.5, -1, -2.5, -7)
GROW_PATTERNS = ("threshold4", "last_corner", "wide_u", "noise41", "noise59", "all_hole", "no_hole", "blobs")
GROW_SHAPES = [(1, 300), (300, 1), (90, 130), (129, 257)]
GROW_CASES = [(p, s, r) for p in GROW_PATTERNS for s in GROW_SHAPES for r in GROW_R]


@functools.lru_cache(maxsize=None)
def case_mask(pattern, shape):
    """holesref's masks, and two of this file's: `threshold4` (bytes 127, 128, 129 and 255 mixed) and `blobs` (discs, specks and
    hairline gaps: what close and open exist for)."""
    if pattern not in ("threshold4", "blobs"):
        return hr.case_mask(pattern, shape)
    Hs, Ws = shape
    rs = np.random.RandomState(Hs * 131 + Ws * 7 + len(pattern))
    if pattern == "threshold4":
        m = rs.choice(np.array([127, 128, 129, 255], dtype=np.uint8), size=shape, p=[0.55, 0.15, 0.15, 0.15])
    else:
        yy, xx = np.mgrid[0:Hs, 0:Ws]
        hole = np.zeros(shape, dtype=bool)
        for _ in range(6):
            cy, cx, rad = rs.randint(0, Hs), rs.randint(0, Ws), rs.randint(3, 14)
            hole |= (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
        hole[:, Ws // 3] = False                               # a hairline gap through whatever lies there
        hole[Hs // 2] = False
        hole |= rs.rand(Hs, Ws) < 0.004                        # specks
        m = np.where(hole, rs.randint(128, 256, size=shape), rs.randint(0, 128, size=shape)).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def case_dist2(pattern, shape, to_hole, rmax):
    """mask_dist2_ref of a case, computed once and shared (read-only)."""
    d = mask_dist2_ref(case_mask(pattern, shape), to_hole, rmax)
    d.setflags(write=False)
    return d
