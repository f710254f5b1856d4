"""numpy restatements of the tone field (pbe_amd/csrc/tone_field.hip, pbe_paste_window_field_u8 of window.hip) and the gates the tests hold
them to.  Nothing here imports the library: tests/test_tone_field_cpu.py runs these on themselves, tests/test_tone_field_gpu.py runs
the kernels through them.

  cells_ref / cells_loop       the int32 [B, 4, Hc, Wc] table, vectorised and by a plain loop; CELL_FAULTS are wrong variants
  pull                         the pyramid of sums in Python ints (object arrays)
  field64 / field32            the push in fp64 (from the unrounded double means) and in the kernel's fp32 order; FIELD_FAULTS
  sample_field                 the bilinear sample of the paste, fp64 (exact scale) or the kernel's fp32 order
  paste_field64 / paste_field32, gate_paste_field      windowref's paste with res + f; PASTE_FAULTS

Two tolerances, both from operation counts, u = 2^-24 (the unit roundoff of fp32), L the field's bound (`limit`):

FIELD against fp64, field_tol(levels, L) = 10 levels L u.  The top is one rounding of a value of size <= L: L u.  One level down, u is
three mixes fmaf(0.25, b - a, a): b - a is rounded (|b - a| <= 2 L: 2 L u, weighted 0.25) and the fmaf once (L u), 1.5 L u per mix and
two mixes deep, 3 L u; the errors that come in with a and b pass through convex weights (0.75, 0.25) and are not amplified.  Then
v = fmaf(w, m - u, u): m - u rounded (2 L u), w rounded (relative u on a product <= 2 L: 2 L u), the fmaf (L u), and the incoming errors of
m (L u) and of u again under convex weights w and 1 - w.  In all at most 3 + 2 + 2 + 1 + 1 = 9 L u per level, granted as 10, so the error is
linear in the number of levels.  The clamp is monotone and adds nothing.

PASTE near-tie tolerance, in units of v: toneref's bound at G = 1, (nx + ny + 16) u, plus
  the field's error            field_tol(levels of the grid, L), L = max(limit, max |field|): zero when both sides are handed the same field,
                               granted always;
  the sample's roundings       two mixes deep as above with |b - a| <= 2 L and a fraction <= 1: 2 (2 L + L) u = 6 L u, and res + f: 2 u;
  the coordinate term          ty = fmaf(oy + 0.5, sy, -0.5): sy is one rounding of the exact ratio (relative u on a product <= Hc) and the
                               fmaf another (|ty| <= Hc), so |ty32 - ty| <= 2 Hc u; the fraction ty - floor(ty) is exact.  The sample moves
                               by at most that times the largest step between neighbouring cells along the axis (the surface is
                               continuous across a flip of floor): 2 u (Hc Sy + Wc Sx).
all multiplied by alpha <= 1.  A reference byte 255 v nearer to a half-way point than 255 times that may round either way and is skipped; at
most 1 % of the alpha > 0 bytes may be (windowref.PASTE_TIE_CAP, asserted on the reference alone), and test_tone_field_cpu.py checks that
the fp32 emulation alone passes the gate on every case."""
import numpy as np

import toneref as tr
import windowref as wr

F = np.float32
U = wr.U
CELLS = (4, 8, 16, 32, 64)


# ---- pbe_tone_cells_i32 ----------------------------------------------------------------------------------------------------------------
def grid_of(H, W, cell):
    return -(-H // cell), -(-W // cell)


def cells_ref(image, result, sel, cell=8, *, rounding=np.rint, strict=False, swap=False, drop_ragged_row=False):
    """int32 [B, 4, Hc, Wc]: plane 0 the pixels of the cell with sel >= 0.5 (a NaN compares false), planes 1 .. 3 the sums of o - q over
    them.  The keywords are the wrong variants of CELL_FAULTS."""
    image, result, sel = (np.asarray(a, dtype=F) for a in (image, result, sel))
    B, _, H, W = image.shape
    Hc, Wc = grid_of(H, W, cell)
    o, q = tr.quant_image(image, rounding), tr.quant_result(result, rounding)
    if swap:
        o, q = q, o
    with np.errstate(invalid="ignore"):
        m = (sel > F(0.5) if strict else sel >= F(0.5)).astype(np.int64)          # [B, 1, H, W]
    per = np.concatenate([m, (o - q) * m], axis=1)                                 # [B, 4, H, W]
    pad = np.zeros((B, 4, Hc * cell, Wc * cell), dtype=np.int64)
    pad[:, :, :H, :W] = per
    t = pad.reshape(B, 4, Hc, cell, Wc, cell).sum(axis=(3, 5))
    if drop_ragged_row and H % cell:
        t[:, :, -1, :] = 0
    return t.astype(np.int32)


def cells_loop(image, result, sel, cell=8):
    """The same table from a plain Python loop over the pixels (tiny inputs only)."""
    B, _, H, W = np.shape(image)
    Hc, Wc = grid_of(H, W, cell)
    t = np.zeros((B, 4, Hc, Wc), dtype=np.int32)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if not float(sel[b][0][y][x]) >= 0.5:
                    continue
                t[b, 0, y // cell, x // cell] += 1
                for c in range(3):
                    o = int(tr.quant_image(image[b][c][y][x]))
                    q = int(tr.quant_result(result[b][c][y][x]))
                    t[b, 1 + c, y // cell, x // cell] += o - q
    return t


CELL_FAULTS = {
    "sel > 0.5 in place of >=": dict(strict=True),
    "floor in place of rint": dict(rounding=np.floor),
    "o and q exchanged": dict(swap=True),
    "the ragged last cell row dropped": dict(drop_ragged_row=True),
}

# ((B, H, W), what sel holds, cell).  One pixel; an odd H W below one cell row with ragged edges both ways; odd planes, two samples; W a
# multiple of 4 (the 4-wide path, cells 4 / 8 / 16: 1, 2 and 4 lanes per cell and, at cell 16 with scalar loads below, 16); W = 18: a
# multiple of 2 only; H W a multiple of 4 with an odd W (scalar loads); more than one block of 256 vectors along a row (W = 1100); all
# and none selected.  tests/test_tone_field_gpu.py adds the (1, 64, 96) planes one float off alignment.
CELL_CASES = [((1, 1, 1), "mixed", 8), ((1, 9, 17), "mixed", 8), ((2, 33, 47), "mixed", 8), ((1, 64, 96), "mixed", 8), ((2, 7, 18), "mixed", 8),
              ((1, 4, 5), "mixed", 4), ((1, 64, 96), "mixed", 4), ((1, 64, 96), "mixed", 16), ((2, 33, 47), "mixed", 16), ((1, 70, 90), "mixed", 64),
              ((1, 40, 66), "mixed", 32), ((1, 5, 1100), "mixed", 4), ((2, 33, 47), "ones", 8), ((2, 33, 47), "zeros", 8), ((1, 64, 96), "ones", 8)]


def cell_case_id(case):
    (B, H, W), mode, cell = case
    return f"{B}x{H}x{W}_{mode}_c{cell}"


# ---- the pyramid -----------------------------------------------------------------------------------------------------------------------
def levels_of(grid):
    h, w, n = int(grid[0]), int(grid[1]), 1
    while h > 1 or w > 1:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def pull(table, drop_odd_col=False):
    """table int [4, Hc, Wc] -> the list of levels, each an object array [4, Hl, Wl] of Python ints; the last is 1 x 1."""
    t = np.asarray(table).astype(object)
    out = [t]
    while t.shape[1] > 1 or t.shape[2] > 1:
        H, W = t.shape[1:]
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        p = np.zeros((4, 2 * H2, 2 * W2), dtype=object)
        p[:, :H, :W] = t
        if drop_odd_col and W % 2:
            p[:, :, W - 1] = 0
        t = p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]
        out.append(t)
    return out


def _means(level, limit, dtype, clamp=True):
    """[3, H, W]: clamp(S / (255 n), +-limit) where n > 0, else 0.  fp32: one rounding of the exact double quotient, as the kernel."""
    n, S = level[0], level[1:4]
    lim = float(F(limit))
    m = np.zeros(S.shape, dtype=np.float64)
    for idx in np.ndindex(*S.shape):
        k = int(n[idx[1:]])
        if k > 0:
            v = int(S[idx]) / (255.0 * k)
            v = float(F(v)) if dtype is F else v
            m[idx] = min(max(v, -lim), lim) if clamp else v
    return m.astype(dtype)


def _push(levels, cell, limit, min_pixels, dtype, wrong_side=False, no_min=False, no_clamp=False):
    top_n = int(levels[-1][0, 0, 0])
    if top_n == 0 or top_n < min_pixels:
        return np.zeros((3,) + levels[0].shape[1:], dtype=dtype)
    fma = wr.fma32 if dtype is F else (lambda a, b, c: a * b + c)
    mix = lambda a, b: fma(dtype(0.25), b - a, a)          # noqa: E731
    cap = cell * cell
    v = None
    for level in reversed(levels):
        m = _means(level, limit, dtype, clamp=not no_clamp)
        if v is None:
            v = _means(level, limit, dtype)
            continue
        H, W = level.shape[1:]
        Hh, Wh = v.shape[1:]
        i, j = np.arange(H), np.arange(W)
        sgn = -1 if wrong_side else 1
        ia, ja = i >> 1, j >> 1
        ib = np.clip(ia + sgn * np.where(i & 1, 1, -1), 0, Hh - 1)
        jb = np.clip(ja + sgn * np.where(j & 1, 1, -1), 0, Wh - 1)
        r = mix(v[:, ia, :], v[:, ib, :])
        u = mix(r[:, :, ja], r[:, :, jb])
        n = level[0].astype(np.float64)
        w = ((n if no_min else np.minimum(n, cap)).astype(dtype) / dtype(cap)).astype(dtype)
        v = fma(w[None], m - u, u).astype(dtype)
    return v


def field64(table, cell=8, limit=0.125, min_pixels=64):
    """fp64 [3, Hc, Wc] from one sample's table [4, Hc, Wc]: exact sums, unrounded double means, the push in fp64."""
    return _push(pull(table), cell, limit, min_pixels, np.float64)


def field32(table, cell=8, limit=0.125, min_pixels=64, *, drop_odd_col=False, **fault):
    """The kernel's arithmetic in fp32, operation for operation.  The keywords are the wrong variants of FIELD_FAULTS."""
    return _push(pull(table, drop_odd_col), cell, limit, min_pixels, F, **fault)


FIELD_FAULTS = {
    "the neighbour chosen on the wrong side": dict(wrong_side=True),
    "w without the min": dict(no_min=True),
    "the pull dropping the odd last column": dict(drop_odd_col=True),
    "the blend applied without the clamp of m": dict(no_clamp=True),
}


def field_tol(levels, limit=0.125):
    return 10.0 * levels * float(limit) * U


FIELD_GRIDS = [(1, 1), (1, 5), (3, 2), (5, 7), (8, 8), (13, 16), (64, 64)]


def random_table(grid, cell=8, seed=0, empty=0.3, amp=40.0):
    """A consistent table int32 [4, Hc, Wc]: n in 0 .. cell^2 (a share `empty` of the cells, and one block of them, hold nothing), the
    sums n * (a smooth difference + noise) per channel, some of them past the clamp at limit 0.125 (32 grey levels)."""
    rs = np.random.RandomState(100 * grid[0] + grid[1] + seed)
    Hc, Wc = grid
    n = rs.randint(0, cell * cell + 1, size=grid)
    n[rs.rand(*grid) < empty] = 0
    n[Hc // 3:Hc // 3 + max(Hc // 4, 1), Wc // 3:Wc // 3 + max(Wc // 4, 1)] = 0
    n[0, 0] = cell * cell                                       # the 1 x 1 grid holds evidence
    yy, xx = np.mgrid[0:Hc, 0:Wc]
    t = np.zeros((4, Hc, Wc), dtype=np.int64)
    t[0] = n
    for c in range(3):
        d = amp * ((xx / max(Wc - 1, 1) - 0.5) * (c + 1) / 2 + (yy / max(Hc - 1, 1) - 0.5) * (2 - c) / 2) + rs.normal(0, 6.0, grid)
        t[1 + c] = np.clip(np.rint(n * d), -255 * n, 255 * n).astype(np.int64)
    return t.astype(np.int32)


def constant_table(grid, d, cell=8, seed=0):
    """A table whose every selected pixel differs by d grey levels, with a hole in the selection and ragged counts."""
    rs = np.random.RandomState(7 * grid[0] + grid[1] + seed)
    n = rs.randint(1, cell * cell + 1, size=grid)
    n[grid[0] // 2:, grid[1] // 2:] = 0
    n[0, 0] = cell * cell
    return np.stack([n, d * n, d * n, d * n]).astype(np.int32)


# ---- pbe_paste_window_field_u8 ---------------------------------------------------------------------------------------------------------
def _axis(n_out, n_work, cell, n_cells, dtype, corner=False):
    """(a, b, t): the two clamped cells and the fraction for every window pixel along one axis.  fp32: the kernel's operations with the
    scale rounded to fp32 on the host; fp64: the exact ratio."""
    o = np.arange(n_out)
    half = 0.0 if corner else 0.5
    if dtype is F:
        s = F(float(n_work) / (float(n_out) * cell))
        c = wr.fma32(o.astype(F) + F(half), s, F(-0.5))
    else:
        c = (o + half) * (float(n_work) / (float(n_out) * cell)) - 0.5
    f = np.floor(c)
    i = f.astype(np.int64)
    return np.clip(i, 0, n_cells - 1), np.clip(i + 1, 0, n_cells - 1), (c - f).astype(dtype)


def sample_field(field, window_hw, size, cell, dtype=np.float64, corner=False):
    """[3, wh, ww]: the bilinear sample of field [3, Hc, Wc] at the window pixels' centres, along y and then along x."""
    fld = np.asarray(field).astype(dtype)
    fma = wr.fma32 if dtype is F else (lambda a, b, c: a * b + c)
    ya, yb, ty = _axis(window_hw[0], size[0], cell, fld.shape[1], dtype, corner)
    xa, xb, tx = _axis(window_hw[1], size[1], cell, fld.shape[2], dtype, corner)
    col = fma(ty[None, :, None], fld[:, yb, :] - fld[:, ya, :], fld[:, ya, :])
    return fma(tx[None, None, :], col[:, :, xb] - col[:, :, xa], col[:, :, xa]).astype(dtype)


def paste_field64(picture, result, alpha, window, field, cell=8):
    """windowref.paste64 with res + f: (bytes int [wh, ww, 3], x = 255 v fp64, ny [wh], nx [ww])."""
    _, _, wh, ww = window
    res, ny, nx = wr.filter64(np.asarray(result, dtype=np.float64), (wh, ww))
    res = (res + sample_field(field, (wh, ww), np.shape(result)[1:], cell)).transpose(1, 2, 0)
    old = wr.crop(picture, window).astype(np.float64)
    a = np.asarray(alpha, dtype=np.float64)[:, :, None]
    x = 255.0 * np.clip(a * res + (1.0 - a) * (old / 255.0), 0.0, 1.0)
    return np.where(a > 0, np.rint(x), old).astype(np.int64), x, ny, nx


def paste_field32(picture, result, alpha, window, field, cell=8, fault=None):
    """The kernel's arithmetic.  fault = the wrong variants the gate must reject: "corner" (the field sampled at the pixel's corner),
    "after_blend" (the field added to the blended value), "writes_everywhere" (alpha raised to 0.25: a write where alpha is 0)."""
    y0, x0, wh, ww = window
    a = np.asarray(alpha, dtype=F)[:, :, None]
    if fault == "writes_everywhere":
        a = np.maximum(a, F(0.25))
    f = sample_field(field, (wh, ww), np.shape(result)[1:], cell, F, corner=fault == "corner").transpose(1, 2, 0)
    res = wr.resample32(result, (wh, ww)).transpose(1, 2, 0)
    if fault != "after_blend":
        res = (res + f).astype(F)
    old = wr.crop(picture, window)
    v = wr.fma32(a, res, (F(1) - a) * (old.astype(F) / F(255)))
    if fault == "after_blend":
        v = (v + f).astype(F)
    new = np.rint(F(255) * np.clip(v, F(0), F(1))).astype(np.uint8)
    out = picture.copy()
    out[y0:y0 + wh, x0:x0 + ww] = np.where(a > 0, new, old)
    return out


PASTE_FAULTS = ("corner", "after_blend", "writes_everywhere")


def paste_tol(field, nx, ny, limit=0.125):
    """The near-tie tolerance of the module docstring in units of v: [wh, ww] fp64."""
    fld = np.asarray(field, dtype=np.float64)
    _, Hc, Wc = fld.shape
    L = max(float(limit), float(np.abs(fld).max()))
    Sy = float(np.abs(np.diff(fld, axis=1)).max()) if Hc > 1 else 0.0
    Sx = float(np.abs(np.diff(fld, axis=2)).max()) if Wc > 1 else 0.0
    fixed = field_tol(levels_of((Hc, Wc)), L) + (6.0 * L + 2.0) * U + 2.0 * U * (Hc * Sy + Wc * Sx)
    return (nx[None, :] + ny[:, None] + 16.0) * U + fixed


def gate_paste_field(got, picture, result, alpha, window, field, cell=8, limit=0.125, what="paste_window field"):
    """windowref.gate_paste for the field entry: outside the window and where alpha == 0 `got` is `picture` byte for byte; where
    alpha > 0 it is paste_field64's byte, or one grey level off where the reference's 255 v lies within 255 paste_tol of a half-way
    point.  Returns (bytes that differ, bytes allowed to, bytes with alpha > 0)."""
    y0, x0, wh, ww = window
    ref, x, ny, nx = paste_field64(picture, result, alpha, window, field, cell)
    live = np.broadcast_to((np.asarray(alpha) > 0)[:, :, None], ref.shape)
    tol = 255.0 * paste_tol(field, nx, ny, limit)[:, :, None]
    near = live & (np.abs(x - (np.floor(x) + 0.5)) <= tol)
    n_live = int(live.sum())
    assert near.sum() <= wr.PASTE_TIE_CAP * max(n_live, 1), f"{what}: {int(near.sum())} of {n_live} reference values lie at a rounding tie: the test's inputs are unfit"
    got = np.asarray(got)
    assert got.shape == picture.shape and got.dtype == np.uint8
    outside = np.ones(picture.shape[:2], dtype=bool)
    outside[y0:y0 + wh, x0:x0 + ww] = np.asarray(alpha) <= 0
    assert np.array_equal(got[outside], picture[outside]), f"{what}: {int((got[outside] != picture[outside]).sum())} byte(s) outside {{alpha > 0}} were changed"
    diff = wr.crop(got, window).astype(np.int64) - ref
    bad = live & (diff != 0) & ~(near & (np.abs(diff) == 1))
    assert not bad.any(), (f"{what}: {int(bad.sum())} byte(s) differ from the fp64 reference away from a rounding tie, first at "
                           f"{np.argwhere(bad)[0].tolist()} (got {wr.crop(got, window)[tuple(np.argwhere(bad)[0])]}, reference {ref[tuple(np.argwhere(bad)[0])]})")
    return int((live & (diff != 0)).sum()), int(near.sum()), n_live


# (name, picture (Hs, Ws), window, working size, cell): scale 1 (ragged cells both ways), scale 1.25, an anisotropic window, and
# windowref's downscaling paste (a working size larger than the window)
PASTE_CASES = [("scale1", (97, 131), (30, 40, 36, 50), (36, 50), 8), ("scale1.25", (120, 170), (9, 11, 80, 100), (64, 80), 8),
               ("anisotropic", (120, 170), (10, 60, 100, 40), (32, 48), 4), ("downscaling", (120, 170), (50, 70, 20, 30), (32, 48), 16)]


def paste_field_inputs(case, seed=33):
    """(picture, result, alpha, field fp32 [3, Hc, Wc] within +-0.125 with steps between neighbouring cells)."""
    _, shape, win, size, cell = case
    pic, result, alpha = wr.paste_inputs(shape, win, size, seed)
    rs = np.random.RandomState(seed + 1)
    return pic, result, alpha, rs.uniform(-0.125, 0.125, (3,) + grid_of(size[0], size[1], cell)).astype(F)


# ---- the planted smooth tone -----------------------------------------------------------------------------------------------------------
RAMP_SHAPES = [(96, 128), (100, 77)]
RAMP_MARGIN, RAMP_FEATHER, RAMP_AMP, RAMP_NOISE = 8, 4, 12.0, 4.0


def ramp_case(shape, seed=11):
    """A window at the identity scale whose result is the original minus a planted tone: channel 0 a ramp of +-RAMP_AMP grey levels along
    x, channel 1 along y, channel 2 a constant 6, each plus noise of sd RAMP_NOISE.  Returns (picture uint8 [H, W, 3] with bytes in
    40 .. 215, mask uint8 with one hole, result fp32 [3, H, W], planted fp64 [3, H, W] - the noiseless difference o - q in grey levels)."""
    H, W = shape
    rs = np.random.RandomState(seed + H + W)
    pic = rs.randint(40, 216, size=(H, W, 3)).astype(np.uint8)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[H // 2 - H // 8:H // 2 + H // 8, W // 2 - W // 6:W // 2 + W // 6] = 255
    yy, xx = np.mgrid[0:H, 0:W]
    planted = np.stack([RAMP_AMP * (2.0 * xx / (W - 1) - 1.0), RAMP_AMP * (2.0 * yy / (H - 1) - 1.0), np.full(shape, 6.0)])
    d = np.rint(planted + rs.normal(0.0, RAMP_NOISE, planted.shape)).astype(np.int64)
    q = pic.transpose(2, 0, 1).astype(np.int64) - d
    assert q.min() >= 0 and q.max() <= 255
    return pic, mask, np.ascontiguousarray((q.astype(F) / F(255)).astype(F)), planted


def ramp_errors(field, offset, planted, zone, cell=8):
    """(rms error of the field, rms error of one offset per channel) against the planted tone over the pixels of `zone`, per channel, in
    grey levels.  field [3, Hc, Wc] and offset [3] are in [0, 1] units."""
    H, W = planted.shape[1:]
    f = 255.0 * sample_field(field, (H, W), (H, W), cell)
    off = 255.0 * np.asarray(offset, dtype=np.float64)[:, None, None]
    rms = lambda e: np.sqrt((e[:, zone] ** 2).mean(axis=1))        # noqa: E731
    return rms(f - planted), rms(off - planted)
