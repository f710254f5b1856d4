"""The holes of a mask in numpy: what pbe_amd/csrc/holes.hip (ops.mask_components, ops.component_boxes, ops.select_components) and the
grouping of pbe_amd.window.group_components must give, restated independently of both - labelling by row runs and a union-find over
the runs (the kernels work per pixel in tiles), grouping by whole rounds of a neighbour graph (window.py merges pair by pair).
Everything is an integer: the tests compare by equality.

Also the masks the GPU tests run (CASES) and three wrong labellers (MUTANTS) which tests/test_holes_cpu.py requires those masks to catch.
Not a test file and not a conftest: plain functions only."""
from __future__ import annotations

import functools

import numpy as np

HOLE = 128


# ---- labelling --------------------------------------------------------------------------------------------------------------------------
def _runs(row):
    d = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
    return np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()


def label_ref(mask, connectivity=8):
    """labels int64 [Hs, Ws]: -1 where mask < 128, else the smallest linear index y * Ws + x of the pixel's connected component."""
    assert connectivity in (4, 8)
    hole = np.asarray(mask) >= HOLE
    Hs, Ws = hole.shape
    reach = 1 if connectivity == 8 else 0
    parent, runs = [], []                                    # runs: (y, xa, xb); ids in raster order of the first pixel, so min id = min index

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    prev = []
    for y in range(Hs):
        cur = []
        k = 0
        for a, b in zip(*_runs(hole[y])):
            i = len(parent)
            parent.append(i)
            runs.append((y, a, b))
            cur.append((a, b, i))
            while k < len(prev) and prev[k][1] < a - reach:  # runs of the row above that end before this one begins
                k += 1
            j = k
            while j < len(prev) and prev[j][0] <= b + reach:
                ra, rb = find(i), find(prev[j][2])
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
                j += 1
        prev = cur
    out = np.full((Hs, Ws), -1, dtype=np.int64)
    for i, (y, a, b) in enumerate(runs):
        ry, ra, _ = runs[find(i)]
        out[y, a:b + 1] = ry * Ws + ra
    return out


def boxes_ref(labels):
    """int64 [count, 6]: (label, ya, yb, xa, xb, area) per component, sorted by label."""
    ys, xs = np.nonzero(labels >= 0)
    u, inv = np.unique(labels[ys, xs], return_inverse=True)
    big = max(labels.shape) + 1
    ya, xa = np.full(u.size, big, dtype=np.int64), np.full(u.size, big, dtype=np.int64)
    yb, xb = np.full(u.size, -1, dtype=np.int64), np.full(u.size, -1, dtype=np.int64)
    np.minimum.at(ya, inv, ys); np.maximum.at(yb, inv, ys)
    np.minimum.at(xa, inv, xs); np.maximum.at(xb, inv, xs)
    return np.stack([u.astype(np.int64), ya, yb, xa, xb, np.bincount(inv, minlength=u.size).astype(np.int64)], 1).reshape(-1, 6)


def select_ref(labels, wanted):
    """uint8 [Hs, Ws]: 255 where the label is one of `wanted`."""
    return np.where(np.isin(labels, np.asarray(list(wanted), dtype=np.int64)) & (labels >= 0), 255, 0).astype(np.uint8)


# ---- grouping ---------------------------------------------------------------------------------------------------------------------------
def _gap(a, b):
    dy = max(b[0] - a[1], a[0] - b[1], 0)
    dx = max(b[2] - a[3], a[2] - b[3], 0)
    return max(dy, dx)


def groups_ref(table, feather):
    """[(labels (sorted tuple), box (ya, yb, xa, xb))] ordered by the smallest label: rounds of 'join every cluster of groups linked by a
    box distance <= 2 (2 feather + 1)' until a round joins nothing."""
    limit = 2 * (2 * int(feather) + 1)
    groups = [((int(r[0]),), tuple(int(v) for v in r[1:5])) for r in np.asarray(table, dtype=np.int64).reshape(-1, 6)]
    while True:
        n = len(groups)
        seen, clusters = [False] * n, []
        for s in range(n):
            if seen[s]:
                continue
            seen[s], stack, members = True, [s], []
            while stack:
                i = stack.pop()
                members.append(i)
                for j in range(n):
                    if not seen[j] and _gap(groups[i][1], groups[j][1]) <= limit:
                        seen[j] = True
                        stack.append(j)
            clusters.append(members)
        if len(clusters) == n:
            return sorted(((tuple(sorted(ls)), box) for ls, box in groups), key=lambda g: g[0][0])
        groups = [(sum((groups[i][0] for i in c), ()),
                   (min(groups[i][1][0] for i in c), max(groups[i][1][1] for i in c), min(groups[i][1][2] for i in c), max(groups[i][1][3] for i in c)))
                  for c in clusters]


def group_masks_ref(mask, feather, connectivity=8):
    """[(labels, box, uint8 mask of the group alone)] of a mask, in group order."""
    labels = label_ref(mask, connectivity)
    return [(ls, box, select_ref(labels, ls)) for ls, box in groups_ref(boxes_ref(labels), feather)]


# ---- wrong labellers the case list must catch ------------------------------------------------------------------------------------------
def no_diagonal(mask, connectivity=8):
    """4-connectivity whatever was asked."""
    return label_ref(mask, 4)


def tile_local(T):
    """Components are not merged across multiples of T: every T x T tile labelled alone."""
    def labeller(mask, connectivity=8):
        mask = np.asarray(mask)
        Hs, Ws = mask.shape
        out = np.full((Hs, Ws), -1, dtype=np.int64)
        for y0 in range(0, Hs, T):
            for x0 in range(0, Ws, T):
                sub = label_ref(mask[y0:y0 + T, x0:x0 + T], connectivity)
                w = sub.shape[1]
                out[y0:y0 + T, x0:x0 + T] = np.where(sub >= 0, (y0 + sub // w) * Ws + x0 + sub % w, -1)
        return out
    labeller.__name__ = f"tile_local({T})"
    return labeller


def first_seen(mask, connectivity=8):
    """A component's label is the index of its first pixel in COLUMN order (smallest x, then y), not its smallest index."""
    lab = label_ref(mask, connectivity)
    Hs, Ws = lab.shape
    ys, xs = np.nonzero(lab >= 0)
    if ys.size == 0:
        return lab
    u, inv = np.unique(lab[ys, xs], return_inverse=True)
    key = np.full(u.size, Hs * Ws, dtype=np.int64)
    np.minimum.at(key, inv, xs * Hs + ys)
    new = (key % Hs) * Ws + key // Hs
    out = lab.copy()
    out[ys, xs] = new[inv]
    return out


TILES = (8, 16, 32, 64, 128)
MUTANTS = [no_diagonal, first_seen] + [tile_local(T) for T in TILES]


# ---- the masks of the GPU tests --------------------------------------------------------------------------------------------------------
SHAPES = [(1, 300), (300, 1), (90, 130), (129, 257), (67, 1031)]       # odd, and across any tile size up to 128 in both directions


def _spiral(Hs, Ws):
    """A one-pixel-wide spiral from the first corner inwards, arms one pixel apart: one component, its path as long as half the picture."""
    m = np.zeros((Hs, Ws), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < Hs and 0 <= nx < Ws and not m[ny, nx] and not (0 <= ay < Hs and 0 <= ax < Ws and m[ay, ax])
        if free:
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def _pattern(name, shape):
    Hs, Ws = shape
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    rs = np.random.RandomState(Hs * 7919 + Ws * 31 + sum(name.encode()))
    if name == "all_hole":
        hole = np.ones(shape, dtype=bool)
    elif name == "no_hole":
        hole = np.zeros(shape, dtype=bool)
    elif name == "threshold":                                # bytes 127 next to bytes 128, nothing else
        return np.where(rs.rand(Hs, Ws) < 0.5, 127, 128).astype(np.uint8)
    elif name == "last_corner":
        hole = (yy == Hs - 1) & (xx == Ws - 1)
    elif name == "diagonal":                                 # one component at 8, single pixels at 4
        hole = (yy == xx) | (yy == xx - 70)
    elif name == "antidiagonal":
        hole = (yy + xx == max(Hs, Ws) - 1) | (yy + xx == 63)
    elif name == "checkerboard":
        hole = (yy + xx) % 2 == 0
    elif name == "spiral":
        hole = _spiral(Hs, Ws)
    elif name == "serpentine":                               # full even rows, joined at alternating ends
        hole = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == Ws - 1)) | ((yy % 4 == 3) & (xx == 0))
    elif name == "u_shapes":                                 # arms in columns 4k and 4k + 2 that meet only in the last row
        hole = ((xx % 4 == 0) | (xx % 4 == 2)) | ((yy == Hs - 1) & (xx % 4 != 3))
    elif name == "wide_u":                                   # the first and the last column, joined by the last row: the junction is tiles away
        hole = (xx == 0) | (xx == Ws - 1) | (yy == Hs - 1)
        hole |= (xx == Ws // 2) & (yy < Hs - 2)              # and a bar of its own between them
    elif name in ("noise41", "noise59"):                     # near the percolation thresholds (0.407 at 8, 0.593 at 4): large ragged components
        hole = rs.rand(Hs, Ws) < (0.41 if name == "noise41" else 0.59)
    else:
        raise KeyError(name)
    low, high = rs.randint(0, 128, size=shape), rs.randint(128, 256, size=shape)
    return np.where(hole, high, low).astype(np.uint8)


PATTERNS = ["all_hole", "no_hole", "threshold", "last_corner", "diagonal", "antidiagonal", "checkerboard", "spiral", "serpentine", "u_shapes", "wide_u",
            "noise41", "noise59"]
CASES = [(p, s) for p in PATTERNS for s in SHAPES]


@functools.lru_cache(maxsize=None)
def case_mask(pattern, shape):
    m = _pattern(pattern, shape)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def case_labels(pattern, shape, connectivity):
    """label_ref of a case, computed once and shared (read-only)."""
    lab = label_ref(case_mask(pattern, shape), connectivity)
    lab.setflags(write=False)
    return lab
