"""numpy restatements of the windowed pre/post-processing (pbe_amd/csrc/window.hip, include/pbe_hip.h), and the gates the tests hold
the kernels to.  Nothing here imports the library: the CPU tests run these on themselves, the GPU tests run the kernels through them.

  aa_matrix / filter64      the antialiased triangle filter (ATen upsample_bilinear2d_aa) in fp64, as two dense matrices
  resample32                the same filter in fp32, one correctly rounded operation (or fmaf) at a time in the kernel's order
  image64 / image32         pbe_window_image_u8_f32
  mask_ref                  pbe_window_mask_u8_f32 (integers)
  alpha_ref                 pbe_feather_alpha_f32 (integers, one fp32 division)
  paste64 / paste32         pbe_paste_window_u8
  gate_image, gate_paste    the per-element bounds of the issue; equality gates are plain array_equal

Error bound of the image kernel (gate_image).  u = 2^-24 is the unit roundoff of fp32.  The kernel forms its weights from integers
(window.hip), so a normalised weight is off by at most 3 u relative (two conversions, one division) and there is no coordinate
rounding.  A row sum sum_j v_j w_j over nx taps (v = byte / 255 rounded, in [0, 1]; weights summing to 1) then errs by at most
(4 + nx) u: the weights and v, and one rounding per fmaf of a partial sum <= 1; the column combination adds (ny + 4) u the same
way.  Against the fp64 value f that is |f32 - f| <= (nx + ny + 8) u to first order; the normalisation divides
it by std and adds 2 u |y| for its subtraction and division (the bound grants 4).  Hence |err| <= ((nx + ny + 8) / std_c + 4 |y|) u,
the bound the issue states; image32 - the kernel's arithmetic on the CPU - has to pass it before any device result is looked at
(tests/test_window_cpu.py).  An earlier form of the kernel took ATen's fp32 centre c = s (o + 0.5): its rounding, 2 u c, moves every
weight by up to 2 u c / sup, which grows with the coordinate and not with the tap count; that emulation missed this bound by 1.6 x on
the anisotropic case, and the kernel, not the bound, was changed."""
import numpy as np

U = 2.0 ** -24
F = np.float32


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
def _axis_int(n_in, n_out):
    """The filter in integers (the derivation stands in window.hip): lo [n_out], n [n_out] and wnum [n_out, max n] with
    weight_j = wnum_j / sum_j wnum_j; wnum = 0 past each pixel's own tap count."""
    o = np.arange(n_out, dtype=np.int64)
    cnum, den = (2 * o + 1) * n_in, 2 * max(n_in, n_out)
    lo = np.maximum((cnum - den + n_out) // (2 * n_out), 0)
    n = np.minimum((cnum + den + n_out) // (2 * n_out), n_in) - lo
    j = np.arange(int(n.max()), dtype=np.int64)[None, :]
    d = (2 * (j + lo[:, None]) + 1) * n_out - cnum[:, None]
    return lo, n, np.where(j < n[:, None], np.maximum(den - np.abs(d), 0), 0)


def aa_matrix(n_in, n_out):
    """(M fp64 [n_out, n_in], taps int [n_out]): out = M @ in along one axis; taps = the kernel's tap count (zero-weight ends included)."""
    lo, n, wnum = _axis_int(n_in, n_out)
    M = np.zeros((n_out, n_in))
    for o in range(n_out):
        M[o, lo[o]:lo[o] + n[o]] = wnum[o, :n[o]] / float(wnum[o].sum())
    return M, n


def aa_matrix_float(n_in, n_out):
    """The same matrix from ATen's own floating-point statement of the filter, in fp64: the check that the integer form is that filter."""
    M = np.zeros((n_out, n_in))
    scale = n_in / n_out
    sup = max(scale, 1.0)
    for o in range(n_out):
        c = scale * (o + 0.5)
        lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
        w = np.maximum(1.0 - np.abs((np.arange(lo, hi) - c + 0.5) / sup), 0.0)
        M[o, lo:hi] = w / w.sum()
    return M


def filter64(planes, size):
    """fp64 [C, h, w] -> ([C, H, W], ny [H], nx [W])."""
    My, ny = aa_matrix(planes.shape[1], size[0])
    Mx, nx = aa_matrix(planes.shape[2], size[1])
    return (My @ np.asarray(planes, dtype=np.float64)) @ Mx.T, ny, nx


def _axis32(n_in, n_out):
    """The kernel's aa_axis for every output index at once: (lo int [n_out], w fp32 [n_out, max n]) with w = (float)wnum / (float)sum
    and 0 past each pixel's own tap count (adding x * 0 = 0 leaves a sum's bits alone)."""
    lo, _, wnum = _axis_int(n_in, n_out)
    return lo, wnum.astype(F) / wnum.sum(1).astype(F)[:, None]


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in fp64, the sum is rounded there and once more to fp32 - one rounding too
    many only when the fp64 sum lands on an fp32 tie (about one case in 2^29)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def resample32(planes, size):
    """fp32 [C, h, w] -> fp32 [C, H, W]: aa_resample3 of window.hip, r = fmaf(v, wx, r) per tap, acc = fmaf(r, wy, acc) per row, in order."""
    planes = np.asarray(planes, dtype=F)
    Cc, h, w = planes.shape
    ly, wy = _axis32(h, size[0])
    lx, wx = _axis32(w, size[1])
    acc = np.zeros((Cc, size[0], size[1]), dtype=F)
    for k in range(wy.shape[1]):
        slab = planes[:, np.minimum(ly + k, h - 1), :]
        r = np.zeros_like(acc)
        for j in range(wx.shape[1]):
            r = fma32(slab[:, :, np.minimum(lx + j, w - 1)], wx[None, None, :, j], r)
        acc = fma32(r, wy[None, :, k, None], acc)
    return acc


# ---- pbe_window_image_u8_f32 -----------------------------------------------------------------------------------------------------------
def crop(a, window):
    y0, x0, wh, ww = window
    return a[y0:y0 + wh, x0:x0 + ww]


def image64(picture, window, size, mean=(0.5,) * 3, std=(0.5,) * 3):
    """([3, H, W] fp64, ny, nx); mean / std are taken at their fp32 values, as the kernel receives them."""
    f, ny, nx = filter64(crop(picture, window).transpose(2, 0, 1).astype(np.float64) / 255.0, size)
    m, s = np.asarray(mean, dtype=F).astype(np.float64), np.asarray(std, dtype=F).astype(np.float64)
    return (f - m[:, None, None]) / s[:, None, None], ny, nx


def image32(picture, window, size, mean=(0.5,) * 3, std=(0.5,) * 3):
    f = resample32(crop(picture, window).transpose(2, 0, 1).astype(F) / F(255), size)
    m, s = np.asarray(mean, dtype=F), np.asarray(std, dtype=F)
    return (f - m[:, None, None]) / s[:, None, None]


def image_bound(ref, ny, nx, std=(0.5,) * 3):
    s = np.asarray(std, dtype=F).astype(np.float64)
    return ((nx[None, None, :] + ny[None, :, None] + 8.0) / s[:, None, None] + 4.0 * np.abs(ref)) * U


def gate_image(got, picture, window, size, mean=(0.5,) * 3, std=(0.5,) * 3, what="window_image"):
    """got [3, H, W] against image64 under the bound of the module docstring; returns the worst |err| / bound."""
    ref, ny, nx = image64(picture, window, size, mean, std)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{what}: shape {got.shape} vs {ref.shape}, or a non-finite value"
    ratio = np.abs(got - ref) / image_bound(ref, ny, nx, std)
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |err| is {worst:.3g} x the bound at {np.unravel_index(ratio.argmax(), ratio.shape)} (window {window}, size {size})"
    return worst


# ---- integers: mask, dilate, box -------------------------------------------------------------------------------------------------------
def mask_ref(mask, window, size):
    """keep plane fp32 [1, H, W]: 0 iff a byte >= 128 lies in the working pixel's footprint of window rows / columns."""
    _, _, wh, ww = window
    H, W = size
    S = np.zeros((wh + 1, ww + 1), dtype=np.int64)
    S[1:, 1:] = (crop(mask, window) >= 128).cumsum(0).cumsum(1)
    Y, X = np.arange(H), np.arange(W)
    ya, yb = (Y * wh) // H, -((-(Y + 1) * wh) // H)
    xa, xb = (X * ww) // W, -((-(X + 1) * ww) // W)
    cnt = S[yb[:, None], xb[None, :]] - S[ya[:, None], xb[None, :]] - S[yb[:, None], xa[None, :]] + S[ya[:, None], xa[None, :]]
    return (cnt == 0).astype(F)[None]


def box_count(a, r, pad="edge"):
    """Integer count of a (0/1, whole picture) over the (2r+1)^2 square around every pixel; pad = 'edge' (replicate) or 'constant' (zeros)."""
    p = np.pad(a.astype(np.int64), r, mode=pad)
    S = np.zeros((p.shape[0] + 1, p.shape[1] + 1), dtype=np.int64)
    S[1:, 1:] = p.cumsum(0).cumsum(1)
    m, (h, w) = 2 * r + 1, a.shape
    return S[m:m + h, m:m + w] - S[:h, m:m + w] - S[m:m + h, :w] + S[:h, :w]


def alpha_ref(mask, window, r, pad="edge", dilate=True):
    """alpha fp32 [wh, ww] = box_r(dilate_r(hole)) / (2r+1)^2 on the whole picture, cropped to the window; pad / dilate = the wrong
    variants the gates must reject (zero padding, the undilated hole)."""
    hole = mask >= 128
    d = box_count(hole, r, pad) > 0 if dilate else hole
    return (crop(box_count(d, r, pad), window).astype(F) / F((2 * r + 1) ** 2)).astype(F)


def chebyshev_within(mask, d):
    """True where a hole pixel lies within Chebyshev distance d (in the picture)."""
    return box_count(mask >= 128, d, "constant") > 0


# ---- pbe_paste_window_u8 ---------------------------------------------------------------------------------------------------------------
def paste64(picture, result, alpha, window):
    """(bytes int [wh, ww, 3] of the window where alpha > 0 (elsewhere the old byte), x = 255 v fp64, ny [wh], nx [ww])."""
    _, _, wh, ww = window
    res, ny, nx = filter64(np.asarray(result, dtype=np.float64), (wh, ww))
    old = crop(picture, window).astype(np.float64)
    a = np.asarray(alpha, dtype=np.float64)[:, :, None]
    x = 255.0 * np.clip(a * res.transpose(1, 2, 0) + (1.0 - a) * (old / 255.0), 0.0, 1.0)
    return np.where(a > 0, np.rint(x), old).astype(np.int64), x, ny, nx


def paste32(picture, result, alpha, window, rounding=np.rint, written=None):
    """The kernel's arithmetic: a copy of the picture with the window pasted; v = fmaf(alpha, res, (1 - alpha) o) through fma32.
    rounding / written (a boolean [wh, ww] in place of alpha > 0) = the wrong variants the gate must reject."""
    y0, x0, wh, ww = window
    a = np.asarray(alpha, dtype=F)[:, :, None]
    res = resample32(result, (wh, ww)).transpose(1, 2, 0)
    old = crop(picture, window)
    t = (F(1) - a) * (old.astype(F) / F(255))
    v = fma32(a, res, t)
    new = rounding(F(255) * np.clip(v, F(0), F(1))).astype(np.uint8)
    out = picture.copy()
    wr = (a > 0) if written is None else np.asarray(written)[:, :, None]
    out[y0:y0 + wh, x0:x0 + ww] = np.where(wr, new, old)
    return out


PASTE_TIE_CAP = 0.01


def gate_paste(got, picture, result, alpha, window, what="paste_window"):
    """got = the picture after the paste (uint8 [Hs, Ws, 3]).  Outside the window and where alpha == 0 it must be `picture` byte for
    byte; where alpha > 0 it must be paste64's byte, except that it may be one grey level off where the reference's 255 v lies
    within 255 (nx + ny + 12) 2^-24 of a half-way point.  Those pixels may be at most 1 % of the alpha > 0 ones: asserted on the
    reference alone, before `got` is looked at.  Returns (bytes that differ, bytes allowed to, bytes with alpha > 0)."""
    y0, x0, wh, ww = window
    ref, x, ny, nx = paste64(picture, result, alpha, window)
    live = np.broadcast_to((np.asarray(alpha) > 0)[:, :, None], ref.shape)
    tol = 255.0 * (nx[None, :, None] + ny[:, None, None] + 12.0) * U
    near = live & (np.abs(x - (np.floor(x) + 0.5)) <= tol)
    n_live = int(live.sum())
    assert near.sum() <= PASTE_TIE_CAP * max(n_live, 1), f"{what}: {int(near.sum())} of {n_live} reference values lie at a rounding tie: the test's inputs are unfit"
    got = np.asarray(got)
    assert got.shape == picture.shape and got.dtype == np.uint8
    outside = np.ones(picture.shape[:2], dtype=bool)
    outside[y0:y0 + wh, x0:x0 + ww] = np.asarray(alpha) <= 0
    assert np.array_equal(got[outside], picture[outside]), f"{what}: {int((got[outside] != picture[outside]).sum())} byte(s) outside {{alpha > 0}} were changed"
    diff = crop(got, window).astype(np.int64) - ref
    bad = live & (diff != 0) & ~(near & (np.abs(diff) == 1))
    assert not bad.any(), (f"{what}: {int(bad.sum())} byte(s) differ from the fp64 reference away from a rounding tie, first at "
                           f"{np.argwhere(bad)[0].tolist()} (got {crop(got, window)[tuple(np.argwhere(bad)[0])]}, reference {ref[tuple(np.argwhere(bad)[0])]})")
    return int((live & (diff != 0)).sum()), int(near.sum()), n_live


# ---- the shapes both test files use ----------------------------------------------------------------------------------------------------
# (name, picture (Hs, Ws), window (y0, x0, wh, ww), working size)
IMAGE_CASES = [
    ("scale2", (97, 131), (5, 7, 64, 96), (32, 48)),
    ("non_dyadic", (120, 170), (7, 5, 106, 159), (32, 48)),
    ("magnifying", (120, 170), (50, 70, 20, 30), (32, 48)),
    ("anisotropic", (120, 170), (10, 60, 100, 40), (32, 48)),
    ("flush_top_left", (120, 170), (0, 0, 64, 96), (32, 48)),
    ("flush_bottom_right", (120, 170), (67, 93, 53, 77), (32, 48)),
    ("scale40", (1300, 1300), (10, 10, 1280, 1280), (32, 32)),
    ("identity", (97, 131), (30, 40, 32, 48), (32, 48)),
]


def random_picture(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(shape[0], shape[1], 3)).astype(np.uint8)


def random_mask(shape, seed, blobs=3):
    """uint8 [Hs, Ws]: a few rectangles of 255, a thin line and single pixels on a background of values < 128 (and some in 128 .. 254)."""
    rs = np.random.RandomState(seed)
    Hs, Ws = shape
    m = rs.randint(0, 128, size=shape).astype(np.uint8)
    for _ in range(blobs):
        y, x = rs.randint(0, Hs), rs.randint(0, Ws)
        m[y:y + rs.randint(1, max(Hs // 6, 2)), x:x + rs.randint(1, max(Ws // 6, 2))] = rs.choice([128, 200, 255])
    m[rs.randint(0, Hs), :] = np.where(rs.rand(Ws) < 0.5, 255, m[0])
    for _ in range(4):
        m[rs.randint(0, Hs), rs.randint(0, Ws)] = 128
    return m


def paste_inputs(shape, win, size, seed):
    """(picture, result fp32 [3, H, W] uniform in [0, 1), alpha fp32 [wh, ww] uniform with 30 % zeros and 20 % ones)."""
    rs = np.random.RandomState(seed)
    pic = random_picture(shape, seed)
    result = rs.rand(3, *size).astype(np.float32)
    alpha = rs.rand(win[2], win[3]).astype(np.float32)
    alpha[rs.rand(win[2], win[3]) < 0.3] = 0.0
    alpha[rs.rand(win[2], win[3]) < 0.2] = 1.0
    return pic, result, alpha


PASTE_CASES = [("upscaling", (120, 170), (9, 11, 100, 150), (32, 48)), ("downscaling", (120, 170), (50, 70, 20, 30), (32, 48)),
               ("anisotropic", (120, 170), (10, 60, 100, 40), (32, 48)), ("identity", (97, 131), (30, 40, 32, 48), (32, 48))]
