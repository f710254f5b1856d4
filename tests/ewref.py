"""References, per-element bounds and CPU emulations of the element-wise kernels at both ends of the pipeline (pbe_amd/csrc/elementwise.hip):
the sampler step (pbe_plms_update, pbe_plms_pack_input), the VAE boundary (pbe_posterior_sample, pbe_scale_latent_f16, pbe_image_post_f32),
the layout conversions, the byte <-> plane kernels and pbe_resize_bilinear_f32.  Plain numpy functions, no product code, no conftest:
tests/test_ewgate_cpu.py runs the emulations through the gates (and shows every planted fault rejected), tests/test_ewgate_gpu.py runs
the kernels through them.

Everywhere u = 2^-24 (the unit roundoff of fp32), FLOOR = 1e-38 (the subnormal floor of the edge tests) and a reference is computed in
fp64 from the operands the kernel actually reads: fp16 / fp32 values, coefficients passed through fp32 as the launch passes them.  A
rounding errs by at most u times its result, every result is at most the sum of the magnitudes of the terms it was formed from, so an
output formed by R roundings errs by at most R u S to first order in u, S that magnitude sum.

pbe_plms_update (plms_reference / plms_gate / plms_emulated).  The kernel is plain C++ under -ffp-contract=fast: the compiler may fuse a
multiply into the add after it or not, so the roundings counted are those of the UNFUSED form (fusing only removes some):
    e   = e_u + cfg (e_c - e_u)                     S_e  = |e_u| + |cfg| (|e_c| + |e_u|)     R_e  = 3   (dup 1: e exact, S_e = |e|, R_e = 0)
    e'  = c0 e + c1 h1 + c2 h2 + c3 h3              S_ep = |c0| S_e + sum |c_i h_i|          R_ep = R_e + 1 + 2 n_hist
    x0  = (x - c4 e') c5                            S_0  = (|x| + |c4| S_ep) |c5|            R_0  = R_ep + 3
    x'  = c6 x0 + c7 e'                             S_p  = |c6| S_0 + |c7| S_ep              R_p  = R_0 + 3
(e: the difference, the product, the sum; e': one product for c0 e, a product and a sum per history term; x0: product, difference,
product; x': two products and a sum, and R_p >= R_ep + 2 covers the c7 e' branch).  Gates: |d e_t| <= R_e u S_e, |d pred_x0| <= R_0 u S_0,
|d x_prev| <= R_p u S_p, each + FLOOR.  The gate is relative to S, not to the result: where x = c4 e' cancels, pred_x0 is all rounding
error and S_0 says how large that may be.

pbe_posterior_sample (posterior_reference / gate / posterior_emulated).  z = scale (mean + exp(0.5 clamp(lv, -30, 20)) eps).
The clamp of an fp16 value and the halving are exact; the device expf errs by at most E ulp of its result, an ulp being at most 2 u times
it; then one rounding each for the product with eps, the sum with mean and the product with scale, all on
    S = |scale| (|mean| + ex |eps|),   ex = exp(0.5 clamp(lv))
so |d z| <= u (3 S + 2 E |scale| ex |eps|) + FLOOR.  E = EXPF_ULP = 2: the installed ROCm headers and documentation state no accuracy
for expf, so the gate stands at the 2 ulp the issue sets for that case; it is not fitted to the kernel's output.  The kernel as first
measured missed it (1.035 of the bound, 7.2 u, at logvar <= -30 with mean 0): under -ffp-contract=fast the inline expansion of expf is
itself contracted and loses up to |x| u (expf_lowered states both forms; the contracted one is the planted fault expf_contracted).
The kernel now takes exp in fp64 and rounds once; the gate did not move.

The exact kernels (image_post32, u8_to_planes32, canvas_bytes, rne16 / rne16_bits, widen16).  Their expected value is a bit pattern: the
kernel's arithmetic restated in IEEE fp32 numpy, one correctly rounded operation at a time; the CPU test pins each restatement to the
reference's own expression (torch's clamp((x + 1) / 2), ToTensor + Normalize, (255. * x).astype(np.uint8), Tensor.half()).
pbe_scale_latent_f16 alone keeps a bound (scale_latent_check): one fp32 product stored as fp16 in one rounding or two, so half an fp16
ulp plus the fp32 rounding, (2^-11 + 2^-23) |p| + 2^-25; a product that rounds past 65504 is inf.

pbe_resize_bilinear_f32 (resize_matrix / resize_reference / gate / resize_emulated).  The reference is the filter in fp64 from the
kernel's fp32 scale s = (float)n_in / (float)n_out taken as given (windowref.aa_matrix states the same triangle filter from the exact
rational scale; the CPU test shows the two agree wherever s is exact).  out = My v Mx^T.  Per axis, for an output index o with centre
c = s (o + 0.5), support sup = max(s, 1), n taps of raw weights w_j, T = sum w_j, W_j = w_j / T:
  - the fp32 centre carries u c, which moves every raw weight by at most u c / sup; the tap offset (j - c) + 0.5, the product with the
    rounded 1 / s and 1 - a add at most 9 u more (two roundings of a value <= sup + 1 divided by sup >= 1: 4 u, two relative roundings of
    a <= 2: 4 u, one of 1 - a: u):                                  |d w_j| <= delta = u (c / sup + 9)
  - T accumulates n roundings and n delta, 1 / T and w_j (1 / T) one rounding each:
                                                                   |d W_j| <= delta / T + W_j rho,   rho = (n + 1) u + n delta / T
  - a row sum takes a product and an addition per tap, (n_x + 1) u on its magnitude sum, the column combination (n_y + 1) u.
With |v| the magnitudes of the source, F the 0/1 footprint of the taps and S = |My| |v| |Mx|^T:
    |d out| <= u S (n_x + n_y + 2) + (rho_x + rho_y) S + (delta_x / T_x) (|My| |v| F_x^T) + (delta_y / T_y) (F_y |v| |Mx|^T) + FLOOR
The 2-tap filter (antialias 0) has T = 1 and no normalisation (rho = 0), delta = u (2 c + 1) (the centre, the subtraction of 0.5,
1 - l; l = f - floor(f) is exact) and 6 roundings for the two nested interpolations in place of the accumulation term.
This bound is NOT everywhere below the flat 2e-6 that tests/test_ops_gpu.py::test_resize_bilinear_against_torch holds on inputs in
[0, 1]: the centre term grows with the coordinate (c / sup = 64 at the far edge of 512 -> 64), and a far-edge pixel of a non-dyadic
scale is granted up to about 1e-5.  That is what the fp32 centre can cost on an adversarial plane, so the bound stays as derived and
the 2e-6 check stays where it is; both run.  Where the scale is a power of two the kernel is far inside either.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
FLOOR = 1e-38
EXPF_ULP = 2.0
F = np.float32
D = np.float64


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def f32(v):
    return float(F(v))


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in fp64 (one extra rounding only on an fp64 tie)."""
    return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


class Worst:
    """The worst |err| / bound of a gate and where it sits."""

    def __init__(self, what, err, bound):
        ratio = err / bound
        i = int(np.argmax(ratio))
        self.what, self.ratio, self.where, self.n = what, float(ratio.reshape(-1)[i]), tuple(int(k) for k in np.unravel_index(i, ratio.shape)), ratio.size

    def __str__(self):
        return f"{self.what}: worst |err| / bound = {self.ratio:.3f} at {self.where} of {self.n}"


def gate(got, want, bound, what):
    """Every element finite and within its bound; -> Worst (ratio in units of the bound).  bound already holds its floor."""
    got, want, bound = _np(got, D).reshape(np.shape(want)), np.asarray(want, D), np.asarray(bound, D)
    assert np.isfinite(got).all(), f"{what}: non-finite output at {tuple(np.argwhere(~np.isfinite(got))[0])}"
    w = Worst(what, np.abs(got - want), bound)
    assert w.ratio <= 1.0, str(w)
    return w


# ---- pbe_plms_update --------------------------------------------------------------------------------------------------------------------
PLMS_FAULTS = ("coef_fp16", "swap_h12", "swap_halves", "c4_prev", "drop_hist")
AB = {0: (1.0,), 1: (3 / 2, -1 / 2), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
# the six forms the samplers launch: (name, history tensors, weights, e_t asked for, pred_x0 asked for)
PLMS_FORMS = (("probe", 0, AB[0], True, False), ("step0-second-half", 1, (0.5, 0.5), False, True), ("adams-bashforth-1", 1, AB[1], True, True),
              ("adams-bashforth-2", 2, AB[2], True, True), ("adams-bashforth-3", 3, AB[3], True, True), ("ddim", 0, (1.0,), False, True))
PLMS_ROWS = (49, 48, 47, 25, 1, 0)


def plms_operands(B, HW, dup, n_hist, seed):
    """(eps fp16 [dup*B, HW, 4], x fp32 [B, 4, HW], [history fp32 [B, 4, HW]] * n_hist): unit normal draws, x three times as wide."""
    r = np.random.RandomState(seed)
    eps = r.standard_normal((dup * B, HW, 4)).astype(np.float16)
    x = (3.0 * r.standard_normal((B, 4, HW))).astype(F)
    return eps, x, [r.standard_normal((B, 4, HW)).astype(F) for _ in range(n_hist)]


def _halves(eps, dup):
    """eps fp16 [dup*B, HW, >= 4] -> (e_u, e_c) fp16-valued arrays [B, 4, HW] (dup 1: (e, None))."""
    e = np.swapaxes(_np(eps)[..., :4], 1, 2)
    if dup == 1:
        return e, None
    B = e.shape[0] // 2
    return e[:B], e[B:]


def plms_reference(eps, dup, cfg, x, hist, coef8):
    """One pbe_plms_update call in fp64: eps fp16 [dup*B, HW, >= 4], x and every history tensor fp32 [B, 4, HW], coef8 as
    PLMSSampler._coef builds it.  -> dict of e, ep, x0, xp (values), Se, Sep, S0, Sp (magnitude sums), Re, R0, Rp (rounding counts)."""
    c = [f32(v) for v in coef8]
    cfg = f32(cfg)
    eu, ec = _halves(eps, dup)
    eu = eu.astype(D)
    if dup == 2:
        ec = ec.astype(D)
        e, se, re = eu + cfg * (ec - eu), np.abs(eu) + abs(cfg) * (np.abs(ec) + np.abs(eu)), 3
    else:
        e, se, re = eu, np.abs(eu), 0
    ep, sep = c[0] * e, abs(c[0]) * se
    for ci, h in zip(c[1:4], hist):
        h = _np(h, D)
        ep, sep = ep + ci * h, sep + np.abs(ci * h)
    xd = _np(x, D)
    x0, s0 = (xd - c[4] * ep) * c[5], (np.abs(xd) + abs(c[4]) * sep) * abs(c[5])
    xp, sp = c[6] * x0 + c[7] * ep, abs(c[6]) * s0 + abs(c[7]) * sep
    rep = re + 1 + 2 * len(hist)
    return dict(e=e, ep=ep, x0=x0, xp=xp, Se=se, Sep=sep, S0=s0, Sp=sp, Re=re, R0=rep + 3, Rp=rep + 6)


def plms_gate(got_e, got_x0, got_xp, ref, what=""):
    """got_* fp32 [B, 4, HW] or None (an output the launch did not ask for) -> the worst error of (e_t, pred_x0, x_prev) in units of
    u S; raises AssertionError past R_e / R_0 / R_p."""
    worst = []
    for name, got, want, s, r in (("e_t", got_e, ref["e"], ref["Se"], ref["Re"]), ("pred_x0", got_x0, ref["x0"], ref["S0"], ref["R0"]),
                                  ("x_prev", got_xp, ref["xp"], ref["Sp"], ref["Rp"])):
        if got is None:
            worst.append(0.0)
            continue
        got = _np(got, D).reshape(want.shape)
        assert np.isfinite(got).all(), f"{what}: non-finite {name}"
        err = np.abs(got - want)
        over = err > r * U * s + FLOOR
        worst.append(float((err / (U * s + FLOOR)).max()))
        assert not over.any(), (f"{what}: {name} misses {r} * 2^-24 * S at {int(over.sum())} of {over.size} elements, worst {worst[-1]:.1f} u S, "
                                f"first at {tuple(np.argwhere(over)[0])}")
    return tuple(worst)


def plms_emulated(eps, dup, cfg, x, hist, coef8, fused=False, fault=None):
    """The kernel's fp32 arithmetic on the CPU -> (e, pred_x0, x_prev) fp32 [B, 4, HW].  fused: every multiply followed by an add is one
    fmaf (what -ffp-contract=fast allows); otherwise each operation is rounded on its own.  fault: one of PLMS_FAULTS -
      coef_fp16    1 / sqrt(a_t) (c5) rounded to fp16 on its way to the kernel
      swap_h12     the two newest history tensors exchanged (needs 2 or more)
      swap_halves  the conditional half read where the unconditional belongs, and the other way round (dup 2)
      c4_prev      c4 taken as sqrt(1 - a_prev) (the value of c7) in place of sqrt(1 - a_t)
      drop_hist    the oldest history term left out (needs 1 or more)"""
    assert fault is None or fault in PLMS_FAULTS
    c = [F(v) for v in coef8]
    hist = [_np(h, F) for h in hist]
    if fault == "coef_fp16":
        c[5] = F(np.float16(c[5]))
    if fault == "c4_prev":
        c[4] = c[7]
    if fault == "swap_h12":
        hist[0], hist[1] = hist[1], hist[0]
    if fault == "drop_hist":
        hist = hist[:-1]
    cfg = F(cfg)
    eu, ec = _halves(eps, dup)
    eu = eu.astype(F)
    if dup == 2:
        ec = ec.astype(F)
        if fault == "swap_halves":
            eu, ec = ec, eu
        e = fma32(cfg, ec - eu, eu) if fused else eu + cfg * (ec - eu)
    else:
        e = eu
    ep = c[0] * e
    for ci, h in zip(c[1:4], hist):
        ep = fma32(ci, h, ep) if fused else ep + ci * h
    xs = _np(x, F)
    x0 = (fma32(-c[4], ep, xs) if fused else xs - c[4] * ep) * c[5]
    xp = fma32(c[6], x0, c[7] * ep) if fused else c[6] * x0 + c[7] * ep
    return e.astype(F), x0.astype(F), xp.astype(F)


def plms_cancelling_x(eps, dup, cfg, x, hist, coef8, every=4):
    """x with every `every`-th element replaced by fp32(c4 e') of the fp64 e': pred_x0 is all cancellation there."""
    ref = plms_reference(eps, dup, cfg, x, hist, coef8)
    out = _np(x, F).copy()
    flat, ep = out.reshape(-1), (f32(coef8[4]) * ref["ep"]).astype(F).reshape(-1)
    flat[::every] = ep[::every]
    return out


# ---- pbe_posterior_sample ---------------------------------------------------------------------------------------------------------------
POSTERIOR_FAULTS = ("no_clamp", "clamp20", "exp_lv", "expf_contracted")


def posterior_reference(mom, eps, scale):
    """mom fp16 [B, HW, >= 8] (mean in channels 0 .. 3, log-variance in 4 .. 7), eps fp32 [B, 4, HW] -> (z fp64 [B, 4, HW], bound)."""
    m = _np(mom)
    mean, lv = np.swapaxes(m[..., :4], 1, 2).astype(D), np.swapaxes(m[..., 4:8], 1, 2).astype(D)
    e, s = _np(eps, D), f32(scale)
    ex = np.exp(0.5 * np.clip(lv, -30.0, 20.0))
    z = s * (mean + ex * e)
    mag = abs(s) * (np.abs(mean) + ex * np.abs(e))
    return z, U * (3.0 * mag + 2.0 * EXPF_ULP * abs(s) * ex * np.abs(e)) + FLOOR


def expf_lowered(x, contracted):
    """expf as the compiler expands it inline for gfx950, in fp32 on the CPU: ph = x log2e (high word), pl = fma(x, log2e, -ph) +
    x log2e_lo its error and the low word, n = rint(ph), exp2((ph - n) + pl) * 2^n: 0.65 ulp here with an exact exp2, so within 2 ulp with
    the 1 ulp of the exp2 instruction.  contracted: the difference ph - n
    taken as fma(x, log2e, -n), what -ffp-contract=fast makes of it when the call carries the contract flag - that difference then
    holds the rounding error of ph already, pl adds it a second time, and the result is off by up to |x| u (7 ulp at x = -15)."""
    x = np.asarray(x, F)
    hi, lo = np.array([0x3FB8AA3B, 0x32A5705F], np.uint32).view(F)
    ph = x * hi
    pl = fma32(x, lo, fma32(x, hi, -ph))
    n = np.rint(ph)
    a = (fma32(x, hi, -n) if contracted else ph - n) + pl
    return np.ldexp(np.exp2(a.astype(D)).astype(F), n.astype(np.int64)).astype(F)


def posterior_emulated(mom, eps, scale, fault=None):
    """The kernel's fp32 chain on the CPU (numpy's fp32 exp for expf).  fault: no_clamp, clamp20 (the clamp at +-20), exp_lv (exp(lv)
    in place of exp(lv / 2)), expf_contracted (expf_lowered with the contracted difference: the kernel as it was built before
    posterior_kernel switched contraction off)."""
    assert fault is None or fault in POSTERIOR_FAULTS
    m = _np(mom)
    mean, lv = np.swapaxes(m[..., :4], 1, 2).astype(F), np.swapaxes(m[..., 4:8], 1, 2).astype(F)
    if fault != "no_clamp":
        lo = F(-20.0) if fault == "clamp20" else F(-30.0)
        lv = np.minimum(np.maximum(lv, lo), F(20.0))
    with np.errstate(over="ignore", invalid="ignore"):
        h = (F(1.0) if fault == "exp_lv" else F(0.5)) * lv
        ex = expf_lowered(h, True) if fault == "expf_contracted" else np.exp(h).astype(F)
        return F(scale) * (mean + ex * _np(eps, F))


def posterior_lanes(n):
    """n (mean, log-variance) fp16 pairs and n fp32 eps values: the log-variance cycles through the fp16 values around both clamp bounds
    (-65504, -inf, -31, the two fp16 neighbours of -30 on each side, -30, 0, 20 and its neighbours, 31, 65504, +inf; 17 values), the
    mean through 5 values up to +-65504 with 0 among them, eps through 7 with 0 and +-4: the periods are coprime, so every combination
    occurs within 595 lanes."""
    def near(v):
        b = int(np.array([v], np.float16).view(np.uint16)[0])
        return [np.array([b + d], np.uint16).view(np.float16)[0] for d in (-2, -1, 1, 2)]
    lv = np.array([-65504.0, -np.inf, -31.0, *near(-30.0), -30.0, 0.0, 20.0, *near(20.0), 31.0, 65504.0, np.inf], np.float16)
    mean = np.array([0.0, 1.5, -65504.0, 65504.0, -0.37], np.float16)
    eps = np.array([0.0, 4.0, -4.0, 1.0, -0.5, 2.25, -1.75], F)
    k = np.arange(n)
    return mean[k % 5], lv[k % 17], eps[k % 7]


# ---- the exact kernels ------------------------------------------------------------------------------------------------------------------
def all_f16_bits():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def widen16(bits):
    """fp16 bit patterns -> the fp32 values they widen to (exact; NaN stays NaN)."""
    return np.asarray(bits, np.uint16).view(np.float16).astype(F)


def image_post32(x16):
    """pbe_image_post_f32: clamp((fp32(x) + 1) * 0.5, 0, 1) in IEEE fp32 (x fp16 values, no NaN)."""
    with np.errstate(over="ignore"):
        return np.minimum(np.maximum((np.asarray(x16).astype(F) + F(1.0)) * F(0.5), F(0.0)), F(1.0))


def u8_to_planes32(v, mean=None, std=None, mode=0):
    """pbe_u8_to_planes_f32 on bytes v [..., C]: mode 0 (v / 255 - mean) / std as three separately rounded fp32 operations (ToTensor, then
    Normalize's sub and div), mode 1 (1 - v / 255) < 0.5 ? 0 : 1, mode 2 1 - v / 255."""
    t = np.asarray(v).astype(F) / F(255.0)
    if mode == 1:
        return np.where(F(1.0) - t < F(0.5), F(0.0), F(1.0)).astype(F)
    if mode == 2:
        return F(1.0) - t
    c = t.shape[-1]
    return ((t - np.asarray(mean, F)[:c]) / np.asarray(std, F)[:c]).astype(F)


def canvas_bytes(x, a, b):
    """pbe_planes_to_u8_canvas on fp32 values: trunc(255 * clamp(fp32(x * a) + b, 0, 1)), multiply then add (two roundings)."""
    with np.errstate(over="ignore"):
        y = (np.asarray(x, F) * F(a)).astype(F) + F(b)
    return (F(255.0) * np.minimum(np.maximum(y, F(0.0)), F(1.0))).astype(np.uint8)


def canvas_sources(a, b):
    """Source values for pbe_planes_to_u8_canvas under (a, b): (k / 255 - b) / a for k = 0 .. 255 rounded to fp32 with both fp32
    neighbours of each (the truncation's edges), values that land below 0 and above 1, and exactly 0 and 1."""
    k = np.arange(256, dtype=D)
    v = ((k / 255.0 - f32(b)) / f32(a)).astype(F)
    out = [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf)),
           ((np.array([-0.5, -1e-3, 1.0 + 1e-3, 1.5, -40.0, 40.0]) - f32(b)) / f32(a)).astype(F), np.array([-1e30, 1e30, 0.0, 1.0, -0.0], F)]
    return np.concatenate(out).astype(F)


def rne16(x32):
    """fp32 -> fp16 bit patterns, round to nearest even (numpy's conversion; rne16_bits states it in integers)."""
    with np.errstate(over="ignore"):
        return np.asarray(x32, F).astype(np.float16).view(np.uint16)


def rne16_bits(x32):
    """fp32 -> fp16 bit patterns by integer arithmetic on the fp32 bits: round to nearest, ties to even; overflow from 65520 on is inf,
    2^-25 ties to zero, fp32 subnormals give a signed zero.  NaN is not handled (no test feeds one)."""
    b = np.asarray(x32, F).view(np.uint32).astype(np.int64)
    sign, mag = (b >> 16) & 0x8000, b & 0x7FFFFFFF
    e = (mag >> 23) - 112                                       # the fp16 exponent field of a normal result
    m = np.where(mag >> 23 > 0, (mag & 0x7FFFFF) | 0x800000, 0)
    shift = np.clip(np.where(e >= 1, 13, 14 - e), 13, 26)       # bits dropped: 13 for a normal result, more for a subnormal one
    val = np.where(e >= 1, ((e - 1) << 10) + (m >> 13), m >> shift)
    rem, half = m & ((1 << shift) - 1), 1 << (shift - 1)
    val = val + ((rem > half) | ((rem == half) & (val & 1 == 1)))
    val = np.where((mag >> 23 >= 255) | (val >= 0x7C00), 0x7C00, val)
    return (sign | val).astype(np.uint16)


def rne_inputs():
    """fp32 values that decide a float -> half conversion: for every non-negative finite fp16 pattern p the value itself, the fp32 midpoint
    of p and its successor (65520 after 65504) and both fp32 neighbours of that midpoint, all with both signs; then 65504, the largest
    fp32 below 65520, 65520, 1e30, +-inf, 2^-25 and its upper neighbour, and an fp32 subnormal."""
    p = np.arange(0x7C00, dtype=np.uint16)
    lo = p.view(np.float16).astype(D)
    hi = np.append(lo[1:], 65536.0)
    mid = ((lo + hi) / 2).astype(F)
    assert np.array_equal(mid.astype(D), (lo + hi) / 2)
    pos = np.concatenate([lo.astype(F), mid, np.nextafter(mid, F(0.0)), np.nextafter(mid, F(np.inf))])
    special = np.array([65504.0, np.nextafter(F(65520.0), F(0.0)), 65520.0, 1e30, np.inf, -np.inf, 2.0 ** -25, np.nextafter(F(2.0 ** -25), F(1.0)), 1e-40, -1e-40], F)
    return np.concatenate([pos, -pos, special]).astype(F)


def scale_latent_check(got_bits, x32, inv_scale, what=""):
    """pbe_scale_latent_f16's stated bound: within (2^-11 + 2^-23) |p| + 2^-25 of the exact product p = x * fp32(inv_scale); p rounding
    past 65504 (|p| >= 65520 in either rounding order, up to the fp32 rounding) must be inf of p's sign, below it finite.
    -> the worst |err| / bound over the finite range."""
    got = np.asarray(got_bits, np.uint16).view(np.float16).astype(D)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(x32, F).astype(D) * f32(inv_scale)
    big, small = np.abs(p) >= 65520.0 * (1 + 2.0 ** -23), np.abs(p) <= 65520.0 * (1 - 2.0 ** -23)
    assert np.array_equal(got[big], np.sign(p[big]) * np.inf), f"{what}: a product past 65520 did not become inf"
    assert np.isfinite(got[small]).all(), f"{what}: a product below 65520 became non-finite"
    edge = ~big & ~small
    assert (np.isinf(got[edge]) | (np.abs(got[edge]) == 65504.0)).all(), f"{what}: a product at 65520 is neither 65504 nor inf"
    return Worst(what, np.abs(got[small] - p[small]), (2.0 ** -11 + 2.0 ** -23) * np.abs(p[small]) + 2.0 ** -25)


# ---- pbe_resize_bilinear_f32 ------------------------------------------------------------------------------------------------------------
RESIZE_FAULTS = ("unnormalised", "no_half", "support1")
RS_MAX_TAPS = 64


def resize_scale(n_in, n_out):
    return float(F(n_in) / F(n_out))


def resize_accepts(w_in, w_out):
    """The horizontal scale an antialiased call accepts: 2 max(s, 1) + 2 <= 64 taps, evaluated in fp32 as the entry point does."""
    s = F(w_in) / F(w_out)
    return bool(F(2.0) * max(s, F(1.0)) + F(2.0) <= F(RS_MAX_TAPS))


def resize_matrix(n_in, n_out, aa):
    """One axis of the filter in fp64 from the fp32 scale -> (M [n_out, n_in], taps [n_out], T [n_out] the raw weight sum,
    delta [n_out] the raw-weight error in units of u)."""
    s = resize_scale(n_in, n_out)
    M, taps, T, delta = np.zeros((n_out, n_in)), np.zeros(n_out, int), np.ones(n_out), np.zeros(n_out)
    for o in range(n_out):
        c = s * (o + 0.5)
        if aa:
            sup = max(s, 1.0)
            lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
            w = np.maximum(1.0 - np.abs((np.arange(lo, hi) - c + 0.5) / sup), 0.0)
            M[o, lo:hi], taps[o], T[o], delta[o] = w / w.sum(), hi - lo, w.sum(), c / sup + 9.0
        else:
            f = max(c - 0.5, 0.0)
            i0 = int(f)
            i1 = i0 + (1 if i0 < n_in - 1 else 0)
            M[o, i0] += 1.0 - (f - i0)
            M[o, i1] += f - i0
            taps[o], delta[o] = 2, 2.0 * c + 1.0
    return M, taps, T, delta


def resize_reference(src, size, aa):
    """src fp32 [P, Hin, Win] -> (out fp64 [P, Hout, Wout], bound) (module docstring)."""
    v = _np(src, D)
    My, ny, Ty, dy = resize_matrix(v.shape[1], size[0], aa)
    Mx, nx, Tx, dx = resize_matrix(v.shape[2], size[1], aa)
    out = My @ v @ Mx.T
    av = np.abs(v)
    S = My @ av @ Mx.T
    Fy, Fx = (My > 0).astype(D), (Mx > 0).astype(D)
    for Fm, M in ((Fy, My), (Fx, Mx)):                           # zero-weight end taps belong to the footprint: widen it by one each way
        Fm[:, 1:] = np.maximum(Fm[:, 1:], (M[:, :-1] > 0))
        Fm[:, :-1] = np.maximum(Fm[:, :-1], (M[:, 1:] > 0))
    if aa:
        rho_y, rho_x = (ny + 1 + ny * dy / Ty) * U, (nx + 1 + nx * dx / Tx) * U
        acc = (nx[None, None, :] + ny[None, :, None] + 2.0) * U
    else:
        rho_y, rho_x, acc = np.zeros(size[0]), np.zeros(size[1]), 6.0 * U
    bound = (acc + rho_x[None, None, :] + rho_y[None, :, None]) * S
    bound = bound + (My @ av @ Fx.T) * (dx * U / Tx)[None, None, :] + (Fy @ av @ Mx.T) * (dy * U / Ty)[None, :, None]
    return out, bound + FLOOR


def _axis32(n_in, n_out, fault):
    """The kernel's antialias tap range and normalised fp32 weights for every output index: (lo int [n_out], W fp32 [n_out, taps]), zero
    past each index's own tap count."""
    s = F(n_in) / F(n_out)
    sup = s if s >= 1 else F(1.0)
    inv = F(1.0) / s if s >= 1 else F(1.0)
    if fault == "support1":
        sup, inv = F(1.0), F(1.0)
    o = np.arange(n_out).astype(F)
    c = s * (o + (F(0.0) if fault == "no_half" else F(0.5)))
    lo = np.maximum((c - sup + F(0.5)).astype(np.int64), 0)
    n = np.minimum((c + sup + F(0.5)).astype(np.int64), n_in) - lo
    j = np.arange(int(n.max()))[None, :]
    a = np.abs((((j + lo[:, None]).astype(F) - c[:, None]) + F(0.5)) * inv)
    w = np.where((a < 1) & (j < n[:, None]), F(1.0) - a, F(0.0)).astype(F)
    tw = np.zeros(n_out, F)
    for t in range(w.shape[1]):
        tw = tw + w[:, t]
    norm = np.where(tw != 0, F(1.0) / np.where(tw != 0, tw, F(1.0)), F(0.0)).astype(F)
    if fault == "unnormalised":
        norm = np.ones(n_out, F)
    return lo, (w * norm[:, None]).astype(F)


def resize_emulated(src, size, aa, fault=None):
    """The kernel's fp32 arithmetic on the CPU, unfused (each product and sum rounded; fusing only removes roundings).  fault (antialias
    only): unnormalised (weights not divided by their sum), no_half (the + 0.5 of the centre left out), support1 (support 1 when
    down-scaling)."""
    assert fault is None or (fault in RESIZE_FAULTS and aa)
    v = _np(src, F)
    P, h, w = v.shape
    H, W = size
    if not aa:
        sh, sw = F(h) / F(H), F(w) / F(W)
        fy = np.maximum(sh * (np.arange(H).astype(F) + F(0.5)) - F(0.5), F(0.0))
        fx = np.maximum(sw * (np.arange(W).astype(F) + F(0.5)) - F(0.5), F(0.0))
        y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
        y1, x1 = y0 + (y0 < h - 1), x0 + (x0 < w - 1)
        ly, lx = (fy - y0.astype(F))[None, :, None], (fx - x0.astype(F))[None, None, :]
        g = lambda yy, xx: v[:, yy][:, :, xx]                    # noqa: E731
        top = (F(1.0) - lx) * g(y0, x0) + lx * g(y0, x1)
        bot = (F(1.0) - lx) * g(y1, x0) + lx * g(y1, x1)
        return ((F(1.0) - ly) * top + ly * bot).astype(F)
    ly, wy = _axis32(h, H, fault)
    lx, wx = _axis32(w, W, fault)
    acc = np.zeros((P, H, W), F)
    for k in range(wy.shape[1]):
        slab = v[:, np.minimum(ly + k, h - 1), :]
        r = np.zeros((P, H, W), F)
        for j in range(wx.shape[1]):
            r = r + slab[:, :, np.minimum(lx + j, w - 1)] * wx[None, None, :, j]
        acc = acc + r * wy[None, :, k, None]
    return acc
