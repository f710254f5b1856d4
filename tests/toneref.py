"""numpy restatements of the tone matching (pbe_amd/csrc/tone.hip, pbe_paste_window_tone_u8 of window.hip, pbe_amd.window.fit_tone) and
the gates the tests hold them to.  Nothing here imports the library: tests/test_tone_cpu.py runs these on themselves,
tests/test_tone_gpu.py runs the kernels through them.

  quant_image / quant_result   the two quantisers of pbe_tone_stats_i64 in fp32, one correctly rounded operation at a time
  stats_ref                    the int64 [B, 3, 6] table; STATS_FAULTS are wrong variants the case list must tell from it
  fit_ref                      pbe_amd.window.fit_tone restated with fractions.Fraction
  paste_tone64 / paste_tone32  pbe_paste_window_tone_u8 in fp64 and in the kernel's fp32 order
  gate_paste_tone              windowref.gate_paste with res replaced by g res + b

Tie tolerance of gate_paste_tone.  u = 2^-24.  windowref derives |res32 - res64| <= (nx + ny + 8) u for the resampled result and grants
4 u more for the blend (its 12 = 8 + 4).  The tone step res' = fmaf(g, res, b) multiplies the first error by |g| and adds one rounding
of a value of size at most |g| + |b|; the blend is unchanged.  So |v32 - v64| <= (|g| (nx + ny + 8) + |g| + |b| + 4) u, and with
G = max(|g|, 1) that is at most (G (nx + ny) + 16) u as long as 9 G + |b| + 4 <= 16 - true for every map fit_tone can return at its
default limit (G <= 1.25, |b| <= 0.75), and asserted by the gate for the map it is given.  A reference value 255 v within
255 (G (nx + ny) + 16) u of a half-way point may round either way.  Such values may be at most 1 % of the alpha > 0 bytes (asserted on
the reference alone); on the four windowref.PASTE_CASES with (g, b) = (1.25, -0.1) and (0.8, 0.05) the share is at most 0.08 % (0.065 %
seen), with the per-channel variation of TONES 0.11 %."""
import math
from fractions import Fraction

import numpy as np

import windowref as wr

F = np.float32
U = wr.U


# ---- pbe_tone_stats_i64 ----------------------------------------------------------------------------------------------------------------
def _c01(v):
    """fminf(fmaxf(v, 0), 1): np.fmax / np.fmin return the other operand for a NaN, as fmaxf / fminf do."""
    return np.fmin(np.fmax(v, F(0)), F(1))


def quant_image(x, rounding=np.rint, clamp=_c01):
    """o = (int)rintf(255 c01(0.5 x + 0.5)) for model-normalised fp32 x: a separate multiply (exact) and add, then np.rint (half to even)."""
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        return rounding(F(255) * clamp(F(0.5) * x + F(0.5))).astype(np.int64)


def quant_result(r, rounding=np.rint, clamp=_c01):
    """q = (int)rintf(255 c01(r)) for fp32 r."""
    with np.errstate(invalid="ignore", over="ignore"):
        return rounding(F(255) * clamp(np.asarray(r, dtype=F))).astype(np.int64)


def _sums(o, q, m):
    """o, q int64 [B, 3, HW], m bool [B, HW] -> int64 [B, 3, 6]."""
    mm = m[:, None, :].astype(np.int64)
    n = np.broadcast_to(m.sum(1).astype(np.int64)[:, None], o.shape[:2])
    return np.stack([n, (o * mm).sum(2), (q * mm).sum(2), (o * o * mm).sum(2), (q * q * mm).sum(2), (o * q * mm).sum(2)], axis=2)


def stats_ref(image, result, sel, *, rounding=np.rint, clamp=_c01, strict=False, swap=False, drop_tail=False, wrap32=False):
    """int64 [B, 3, 6]: row [b, c] = n, So, Sq, Soo, Sqq, Soq over the pixels with sel >= 0.5 (a NaN compares false).  The keywords are
    the wrong variants of STATS_FAULTS."""
    image, result, sel = (np.asarray(a, dtype=F) for a in (image, result, sel))
    B, _, H, W = image.shape
    o = quant_image(image, rounding, clamp).reshape(B, 3, H * W)
    q = quant_result(result, rounding, clamp).reshape(B, 3, H * W)
    with np.errstate(invalid="ignore"):
        m = (sel > F(0.5) if strict else sel >= F(0.5)).reshape(B, H * W)
    if swap:
        o, q = q, o
    if drop_tail:
        m = m.copy()
        m[:, (H * W) // 256 * 256:] = False
    t = _sums(o, q, m)
    if wrap32:
        t[:, :, 3:] &= 0xFFFFFFFF
    return t


def stats_loop(image, result, sel):
    """The same table from a plain Python loop (tiny inputs only)."""
    B, _, H, W = np.shape(image)

    def byte(v):
        v = float(F(v))
        v = 0.0 if math.isnan(v) else min(max(v, 0.0), 1.0)
        return int(np.rint(F(255) * F(v)))
    t = [[[0] * 6 for _ in range(3)] for _ in range(B)]
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if not float(sel[b][0][y][x]) >= 0.5:
                    continue
                for c in range(3):
                    o, q = byte(F(0.5) * F(image[b][c][y][x]) + F(0.5)), byte(result[b][c][y][x])
                    for k, v in enumerate((1, o, q, o * o, q * q, o * q)):
                        t[b][c][k] += v
    return np.asarray(t, dtype=np.int64)


def _unclamped(v):
    return np.nan_to_num(v, nan=0.0, posinf=4.0, neginf=-4.0).astype(F)


STATS_FAULTS = {
    "floor in place of rint": dict(rounding=np.floor),
    "sel > 0.5 in place of >=": dict(strict=True),
    "no clamp": dict(clamp=_unclamped),
    "o and q exchanged": dict(swap=True),
    "the last partial block of 256 dropped": dict(drop_tail=True),
    "32-bit wrap of the sums of squares": dict(wrap32=True),
}

# (B, H, W), what sel holds.  The issue's shapes: one pixel; an odd H W below one vector; an odd H W (planes off 16-byte alignment) with a
# tail and two samples; H W a multiple of 4 in three samples; 88 block partials, more than one finalise wave of 64.  (2, 7, 18): H W = 126
# is a multiple of 2 only, the float2 path.  "ones" draws bright inputs so that the sums of squares of the 300 x 300 case pass 2^32.
STATS_CASES = [((1, 1, 1), "mixed"), ((1, 3, 5), "mixed"), ((2, 33, 47), "mixed"), ((3, 64, 96), "mixed"), ((1, 300, 300), "mixed"), ((2, 7, 18), "mixed"),
               ((2, 33, 47), "zeros"), ((3, 64, 96), "ones"), ((1, 300, 300), "ones")]
SEL_VALUES = np.array([0.0, 1.0, 0.5, np.nextafter(F(0.5), F(0)), -0.0, np.nan], dtype=F)


def stats_inputs(shape, sel_mode, seed=0):
    """(image fp32 [B, 3, H, W] reaching outside [-1, 1], result fp32 [B, 3, H, W] reaching outside [0, 1], sel fp32 [B, 1, H, W]) with NaN,
    +-inf and exact ties (k + 0.5) / 255 planted in both pictures."""
    B, H, W = shape
    rs = np.random.RandomState(1000 * B + 10 * H + W + seed)
    if sel_mode == "ones":
        image, result = rs.uniform(0.2, 1.6, (B, 3, H, W)).astype(F), rs.uniform(0.6, 1.3, (B, 3, H, W)).astype(F)
    else:
        image, result = rs.uniform(-1.5, 1.5, (B, 3, H, W)).astype(F), rs.uniform(-0.25, 1.25, (B, 3, H, W)).astype(F)
    n = image.size
    special = np.array([np.nan, np.inf, -np.inf], dtype=F)
    if n >= 64:
        for arr, to in ((image, lambda r: F(2) * r - F(1)), (result, lambda r: r)):
            flat = arr.reshape(-1)
            at = rs.choice(n, size=max(n // 16, 8), replace=False)
            k = rs.randint(0, 255, size=at.size)
            flat[at] = to(((k + 0.5) / 255.0).astype(F))
            at = rs.choice(n, size=max(n // 64, 3), replace=False)
            flat[at] = special[rs.randint(0, 3, size=at.size)]
    if sel_mode == "mixed":
        sel = SEL_VALUES[rs.randint(0, SEL_VALUES.size, size=(B, 1, H, W))]
        sel.reshape(-1)[0] = 1.0                     # the single pixel of (1, 1, 1) counts
    else:
        sel = np.full((B, 1, H, W), 1.0 if sel_mode == "ones" else 0.0, dtype=F)
    return image, result, sel


# ---- pbe_amd.window.fit_tone -----------------------------------------------------------------------------------------------------------
def fit_ref(stats, mode="affine", gain_limit=1.25, min_pixels=64):
    """fit_tone's list from exact rationals: the slope (n Soq - So Sq) / (n Sqq - Sq^2) clamped to [1 / gain_limit, gain_limit] (both bounds
    the doubles fit_tone compares with), rounded to double and to fp32; the offset (So - gain Sq) / (255 n) for that fp32 gain, rounded
    the same way; the two rms from the expanded sums."""
    out = []
    lo, hi = Fraction(1.0 / float(gain_limit)), Fraction(float(gain_limit))
    for sample in np.asarray(stats, dtype=object).tolist():
        n = int(sample[0][0])
        fitted = n > 0 and n >= min_pixels
        d = {"n": n, "gain": [], "offset": [], "clamped": [], "rms_before": [], "rms_after": []}
        for _, So, Sq, Soo, Sqq, Soq in ([int(v) for v in row] for row in sample):
            g, clamped = Fraction(1), False
            if mode == "affine" and fitted and n * Sqq - Sq * Sq != 0:
                g = Fraction(float(Fraction(n * Soq - So * Sq, n * Sqq - Sq * Sq)))          # rounded to double once, then compared
                clamped = g < lo or g > hi
                g = min(max(g, lo), hi)
            gain = Fraction(float(F(float(g))))
            offset = Fraction(float(F(float((So - gain * Sq) / (255 * n))))) if fitted else Fraction(0)
            m = max(n, 1)
            before = Fraction(Soo - 2 * Soq + Sqq, m)
            k = 255 * offset                           # sum (o - gain q - k)^2 expanded
            after = (Soo + gain * gain * Sqq + k * k * n - 2 * gain * Soq - 2 * k * So + 2 * gain * k * Sq) / m
            d["gain"].append(float(gain)); d["offset"].append(float(offset)); d["clamped"].append(clamped)
            d["rms_before"].append(math.sqrt(float(before))); d["rms_after"].append(math.sqrt(float(after)))
        d["identity"] = all(v == 1.0 for v in d["gain"]) and all(v == 0.0 for v in d["offset"])
        out.append(d)
    return out


def random_table(rs, B, n_pixels, g=1.0, b=0.0, noise=6.0, o_range=(0, 255)):
    """A consistent table: bytes o in o_range, q = clip(rint((o - 255 b) / g + noise)) per channel and sample, all pixels counted."""
    o = rs.randint(o_range[0], o_range[1] + 1, size=(B, 3, n_pixels)).astype(np.int64)
    q = np.clip(np.rint((o - 255.0 * b) / g + rs.normal(0.0, noise, o.shape)), 0, 255).astype(np.int64)
    return _sums(o, q, np.ones((B, n_pixels), dtype=bool))


# ---- pbe_paste_window_tone_u8 ----------------------------------------------------------------------------------------------------------
def _gb(gain, offset):
    """The fp32 values the kernel receives, in fp64."""
    return np.asarray(gain, dtype=F).astype(np.float64).reshape(3), np.asarray(offset, dtype=F).astype(np.float64).reshape(3)


def paste_tone64(picture, result, alpha, window, gain, offset):
    """windowref.paste64 with res replaced by g res + b: (bytes int [wh, ww, 3], x = 255 v fp64, ny [wh], nx [ww])."""
    _, _, wh, ww = window
    g, b = _gb(gain, offset)
    res, ny, nx = wr.filter64(np.asarray(result, dtype=np.float64), (wh, ww))
    res = g[None, None, :] * res.transpose(1, 2, 0) + b[None, None, :]
    old = wr.crop(picture, window).astype(np.float64)
    a = np.asarray(alpha, dtype=np.float64)[:, :, None]
    x = 255.0 * np.clip(a * res + (1.0 - a) * (old / 255.0), 0.0, 1.0)
    return np.where(a > 0, np.rint(x), old).astype(np.int64), x, ny, nx


def paste_tone32(picture, result, alpha, window, gain, offset, fault=None):
    """The kernel's arithmetic: res = fmaf(g, res, b), then windowref.paste32's blend.  fault = the wrong variants the gate must reject:
    "after_blend" (the map applied to the blended value), "no_offset", "writes_everywhere" (alpha raised to 0.25: a write where alpha is 0)."""
    y0, x0, wh, ww = window
    g, b = np.asarray(gain, dtype=F).reshape(3), np.asarray(offset, dtype=F).reshape(3)
    if fault == "no_offset":
        b = np.zeros(3, dtype=F)
    a = np.asarray(alpha, dtype=F)[:, :, None]
    if fault == "writes_everywhere":
        a = np.maximum(a, F(0.25))
    res = wr.resample32(result, (wh, ww)).transpose(1, 2, 0)
    if fault != "after_blend":
        res = wr.fma32(g[None, None, :], res, b[None, None, :])
    old = wr.crop(picture, window)
    v = wr.fma32(a, res, (F(1) - a) * (old.astype(F) / F(255)))
    if fault == "after_blend":
        v = wr.fma32(g[None, None, :], v, b[None, None, :])
    new = np.rint(F(255) * np.clip(v, F(0), F(1))).astype(np.uint8)
    out = picture.copy()
    wrote = a > 0
    out[y0:y0 + wh, x0:x0 + ww] = np.where(wrote, new, old)
    return out


def gate_paste_tone(got, picture, result, alpha, window, gain, offset, what="paste_window tone"):
    """windowref.gate_paste for the tone entry (module docstring): outside the window and where alpha == 0 `got` is `picture` byte for
    byte; where alpha > 0 it is paste_tone64's byte, or one grey level off where the reference's 255 v lies within
    255 (G (nx + ny) + 16) 2^-24 of a half-way point, G = max(|g|, 1) per channel.  Returns (bytes that differ, bytes allowed to, bytes
    with alpha > 0)."""
    y0, x0, wh, ww = window
    g, b = _gb(gain, offset)
    G = np.maximum(np.abs(g), 1.0)
    assert np.all(9.0 * G + np.abs(b) + 4.0 <= 16.0), f"{what}: the tolerance is derived for 9 max(|g|, 1) + |b| + 4 <= 16, not for gain {g}, offset {b}"
    ref, x, ny, nx = paste_tone64(picture, result, alpha, window, gain, offset)
    live = np.broadcast_to((np.asarray(alpha) > 0)[:, :, None], ref.shape)
    tol = 255.0 * (G[None, None, :] * (nx[None, :, None] + ny[:, None, None]) + 16.0) * U
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


# (gain [3], offset [3]) of the paste gates: the issue's (1.25, -0.1) with per-channel variations, and (0.8, 0.05)
TONES = [((1.25, 1.1, 0.93), (-0.1, 0.02, 0.07)), ((0.8, 0.8, 0.8), (0.05, 0.05, 0.05))]


# ---- the recovery case: a result that is the original with a tone of its own -----------------------------------------------------------
RECOVERY = [(0.9, 0.04), (1.1, -0.03), (1.0, 0.05)]           # (g0, b0): res = g0 o / 255 + b0
RECOVERY_SHAPE, RECOVERY_WINDOW, RECOVERY_MARGIN, RECOVERY_FEATHER = (120, 170), (20, 30, 64, 96), 8, 4


def recovery_case(g0, b0, seed=7):
    """(picture uint8 with bytes in 20 .. 235, mask uint8 with one hole inside the window, result fp32 [3, H, W] = g0 o / 255 + b0 over
    the whole window, hole included) at the identity scale: the working size is the window's."""
    rs = np.random.RandomState(seed)
    pic = rs.randint(20, 236, size=(*RECOVERY_SHAPE, 3)).astype(np.uint8)
    mask = np.zeros(RECOVERY_SHAPE, dtype=np.uint8)
    mask[45:56, 70:86] = 255
    o = wr.crop(pic, RECOVERY_WINDOW).transpose(2, 0, 1).astype(F)
    result = (F(g0) * (o / F(255)) + F(b0)).astype(F)
    return pic, mask, np.ascontiguousarray(result)
