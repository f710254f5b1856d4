"""Code-by-code gate of the two e4m3 quantisers of the fp8 path: pbe_layernorm_f8 (layernorm_f8_kernel<1..4>, pbe_amd/csrc/norm.hip) and
ops.pack_linear_f8.  Helpers imported by test_f8gate_cpu.py and test_f8gate_gpu.py.  Not a conftest: plain functions only.

An e4m3 code is a decision, not a value with an error bar: the kernel's fp32 LayerNorm differs from fp64 by a few 2^-24, so an element
that close to a rounding boundary may take either neighbouring code, and every other element may take exactly one.  Hence two tiers:

random tier (ln8_gate), for the scale S the kernel reported:
    t  = y64 / S                      dt = dy / S + 3 2^-24 |t|
    gate 1   q_e4m3(t - dt) <= decode(code) <= q_e4m3(t + dt)   for every element (quantisation is monotone: this is the whole admissible
             set); a NaN code fails outright, and so does an element with |t| - dt > 448: the clamp of q_e4m3 is admissible only
             within dt, because a scale that covers its row leaves nothing to saturate (S >= amax (1 - 2 2^-24) / 448)
    gate 2   |S - max_c|y64| / 448| <= max_c(dy) / 448 + 2 2^-24 S, and every S finite, normal, positive
    gate 3   every row holds a code of magnitude 448
    cap      the share of elements with q_e4m3(t - dt) != q_e4m3(t + dt) is at most CAP = 2 %: a condition on the case, never raised
y64 and dy are accgate.ln_terms' (the fp64 LayerNorm and the error of the kernel's fp32 value before any store).  3 2^-24 |t|: the
rounding of 1 / S and of the product y * inv, half an ulp each, and one unit of margin.  2 2^-24 S: the rounding of fl32(1 / 448) and of
the product amax * fl32(1 / 448).

exact tier (exact_rows): gamma = 0, so (x - mean) * rstd * 0 + b is b whatever x holds and whether or not the compiler contracts the
expression to an fma (the product is +-0 and finite); beta holds V 2^k and +-448 2^k, so amax * fl32(1 / 448) is exactly 2^k (k = -3, 0,
5), 1 / 2^k and y * 2^-k are exact, and the kernel converts exactly V.  V: the 127 non-negative e4m3 magnitudes, the 126 midpoints
between neighbours and the fp32 neighbour on either side of each midpoint, in both signs: 1010 values, each with one right byte.

ln8_emulate restates the kernel in plain fp32 (never a kernel's own output) and carries the mutations the gate must reject.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import accgate as ag

U32 = ag.U32
E4M3_MAX = 448.0
CAP = 0.02
SCALE_FLOOR = 2.0 ** -100            # the kernel's and pack_linear_f8's floor of a non-zero row's scale: 1 / scale stays finite
F32_MIN_NORMAL = 2.0 ** -126
EXACT_K = (-3, 0, 5)
EXACT_C = (512, 1024, 1536, 2048)
MUTATIONS = {                         # name -> ln8_emulate keywords
    "truncation": dict(rounding="trunc"),
    "round-half-away": dict(rounding="away"),
    "FNUZ encoding": dict(fnuz=True),
    "scale before beta": dict(scale_before_beta=True),
    "amax over the first 512 columns": dict(amax_cols=512),
    "reported scale off by 2^-9": dict(report_factor=1.0 + 2.0 ** -9),
    "no saturation": dict(saturate=False),
    "variance / (C - 1)": dict(var_divisor_off=1),
}


# ---- the format -------------------------------------------------------------------------------------------------------------------------
def q_e4m3(t, rounding="rne", saturate=True, emin=-6, vmax=E4M3_MAX):
    """OCP e4m3 round-to-nearest-even of an fp64 tensor, in fp64 throughout: |t| clamped to 448, step 2^(max(floor(log2|t|), -6) - 3),
    torch.round (half to even), the sign kept; the decoded value.  rounding 'trunc' / 'away', saturate=False (a magnitude above the
    maximum becomes NaN) and another (emin, vmax) are the mutations."""
    assert t.dtype == torch.float64
    a = t.abs()
    over = a > vmax
    a = a.clamp(max=vmax)
    e = torch.frexp(a)[1].double() - 1.0                       # floor(log2 a), exact; frexp(0) has exponent 0
    step = torch.exp2(torch.clamp(e, min=float(emin)) - 3.0)
    r = a / step                                                # exact: a power-of-two division
    r = torch.round(r) if rounding == "rne" else torch.floor(r) if rounding == "trunc" else torch.floor(r + 0.5)
    q = torch.copysign(torch.clamp(r * step, max=vmax), t)
    q = torch.where(torch.isnan(t), t, q)
    return q if saturate else torch.where(over, torch.full_like(q, math.nan), q)


def _table(bias):
    b = torch.arange(128)
    e, m = (b >> 3).double(), (b & 7).double()
    return torch.where(e == 0, m * 2.0 ** (-2 - bias), (1 + m / 8) * torch.exp2(e - bias))


_OCP = _table(7)                      # magnitudes of codes 0x00 .. 0x7F; 0x7F (480 by the formula) is the NaN code
_FNUZ = _table(8)                     # bias 8, maximum 240 at 0x7F, NaN at 0x80


def decode(codes):
    """uint8 -> fp64 value of an OCP e4m3 code; 0x7F and 0xFF are NaN."""
    c = codes.to(torch.int64)
    mag = _OCP.clone()
    mag[127] = math.nan
    v = mag[c & 127]
    return torch.where((c & 128) != 0, -v, v)


def encode(q, fnuz=False):
    """fp64 values on the e4m3 grid -> uint8 codes (NaN -> 0x7F; a negative zero keeps its sign bit in OCP)."""
    tab = _FNUZ if fnuz else _OCP[:127]
    a = q.abs()
    nan = torch.isnan(q)
    i = torch.searchsorted(tab, torch.where(nan, torch.zeros_like(a), a).contiguous())
    assert bool((tab[i.clamp(max=len(tab) - 1)] == a)[~nan].all()), "encode: a value off the grid"
    neg = torch.signbit(q) & ~nan
    if fnuz:
        neg = neg & (i != 0)                                    # FNUZ has no negative zero: 0x80 is its NaN
        c = torch.where(nan, torch.full_like(i, 128), i + 128 * neg)
    else:
        c = torch.where(nan, torch.full_like(i, 127), i + 128 * neg)
    return c.to(torch.uint8)


# ---- pbe_layernorm_f8 -------------------------------------------------------------------------------------------------------------------
def ln8_reference(x, gamma, beta, eps, S):
    """(t, dt) fp64 for the scale S the kernel reported: t = y64 / S, dt = dy / S + 3 2^-24 |t|."""
    y, dy = ag.ln_terms(x, gamma, beta, eps)
    s = S.double().view(-1, 1)
    t = y / s
    return t, dy / s + 3 * U32 * t.abs()


class Gate:
    """Outcome of one gate: failed = {name: message}; the figures of the report."""

    def __init__(self, what):
        self.what, self.failed = what, {}
        self.scale_ratio = self.ambiguous = self.off_nearest = self.worst = 0.0
        self.where, self.n = "-", 0

    def line(self):
        return (f"f8gate {self.what:44s} ambiguous={100 * self.ambiguous:.3f}% off-nearest={100 * self.off_nearest:.3f}% "
                f"scale err/bound={self.scale_ratio:.3f} worst |got - t| / (step / 2 + dt)={self.worst:.3f} at {self.where} ({self.n} elements)")

    def check(self):
        assert not self.failed, f"{self.what}: " + "; ".join(f"{k}: {v}" for k, v in self.failed.items())
        return self


def _intervals(g, got, t, dt, cap):
    """gate 1 and the cap on decoded codes got against t +- dt; fills the report figures."""
    lo, hi = q_e4m3(t - dt), q_e4m3(t + dt)
    nan = torch.isnan(got)
    bad = nan | (got < lo) | (got > hi) | (t.abs() - dt > E4M3_MAX)
    g.n = t.numel()
    g.ambiguous = (lo != hi).double().mean().item()
    g.off_nearest = (nan | (got != q_e4m3(t))).double().mean().item()
    a = t.abs().clamp(max=E4M3_MAX)
    step = torch.exp2(torch.clamp(torch.frexp(a)[1].double() - 1.0, min=-6.0) - 3.0)
    r = torch.where(nan, torch.full_like(t, math.inf), (got - t.clamp(-E4M3_MAX, E4M3_MAX)).abs() / (step / 2 + dt))
    i = int(torch.argmax(r).item())
    row, col = divmod(i, t.shape[1])
    g.worst, g.where = float(r.reshape(-1)[i]), f"row {row}, column {col}"
    if bool(nan.any()):
        g.failed["gate 1 (NaN code)"] = f"{int(nan.sum())} NaN codes, first at {divmod(int(torch.nonzero(nan.reshape(-1))[0]), t.shape[1])}"
    if bool(bad.any()):
        j = int(torch.nonzero(bad.reshape(-1))[0])
        g.failed["gate 1 (admissible interval)"] = (
            f"{int(bad.sum())} of {t.numel()} codes outside [q(t - dt), q(t + dt)], first at {divmod(j, t.shape[1])}: got {got.reshape(-1)[j].item():.6g}, "
            f"t {t.reshape(-1)[j].item():.9g}, dt {dt.reshape(-1)[j].item():.3g}, admissible [{lo.reshape(-1)[j].item():.6g}, {hi.reshape(-1)[j].item():.6g}]")
    if g.ambiguous > cap:
        g.failed["cap"] = f"ambiguous share {100 * g.ambiguous:.3f} % exceeds the cap of {100 * cap:g} %: the case is too soft to gate, choose another"


def ln8_gate(codes, S, x, gamma, beta, eps, what="layernorm_f8", check=True, cap=CAP):
    """The three gates and the cap on what one launch returned (codes uint8 [rows, C], S fp32 [rows]) for the operands that were sent.
    -> Gate; check=True asserts that nothing failed, naming every part that did."""
    codes, S = codes.cpu(), S.cpu()
    x, gamma, beta = x.cpu(), gamma.cpu(), beta.cpu()
    g = Gate(what)
    s = S.double()
    ok_s = torch.isfinite(s) & (s >= F32_MIN_NORMAL)
    if not bool(ok_s.all()):
        g.failed["gate 2 (scale not finite, normal and positive)"] = f"rows {torch.nonzero(~ok_s).view(-1).tolist()[:8]}: {S[~ok_s].tolist()[:8]}"
        S = torch.where(ok_s, S, torch.ones_like(S))
        s = S.double()
    y, dy = ag.ln_terms(x, gamma, beta, eps)
    t, dt = ln8_reference(x, gamma, beta, eps, S)
    _intervals(g, decode(codes), t, dt, cap)
    s_ref = y.abs().amax(1) / E4M3_MAX
    lim = dy.amax(1) / E4M3_MAX + 2 * U32 * s
    ratio = (s - s_ref).abs() / lim
    r = int(torch.argmax(ratio).item())
    g.scale_ratio = float(ratio[r])
    if g.scale_ratio > 1.0:
        g.failed["gate 2 (scale)"] = f"|S - max|y| / 448| = {g.scale_ratio:.3g} of its bound in row {r}: S {float(s[r]):.9g}, want {float(s_ref[r]):.9g}"
    top = ((codes & 0x7F) == 0x7E).any(1)
    if not bool(top.all()):
        g.failed["gate 3 (row maximum)"] = f"no code of magnitude 448 in rows {torch.nonzero(~top).view(-1).tolist()[:8]}"
    return g.check() if check else g


def ln8_emulate(x, gamma, beta, eps, *, rounding="rne", fnuz=False, scale_before_beta=False, amax_cols=None, report_factor=None,
                saturate=True, var_divisor_off=0, floor=SCALE_FLOOR):
    """layernorm_f8_kernel in plain fp32 -> (codes uint8 [rows, C], S fp32 [rows]): mean from a row sum, centred variance, rsqrt,
    (x - mean) rstd g + b, amax, scale = max(amax fl32(1 / 448), 2^-100) (1 when amax == 0), inv = 1 / scale, codes from q_e4m3 of the
    fp32 product.  The keywords are the mutations (MUTATIONS); floor=None is the kernel before the floor."""
    C = x.shape[-1]
    xf = x.float()
    mean = xf.sum(-1, keepdim=True) / C
    d = xf - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / float(C - var_divisor_off) + eps)
    pre = d * rstd * gamma.float()
    y = pre + beta.float()
    amax = (pre if scale_before_beta else y)[:, :amax_cols].abs().amax(1, keepdim=True)
    scale = amax * torch.tensor(1.0, dtype=torch.float32).div(448.0)
    if floor is not None:
        scale = scale.clamp(min=floor)
    scale = torch.where(amax > 0, scale, torch.ones_like(scale))
    inv = 1.0 / scale
    v = (y * inv).double()
    if fnuz:
        codes = encode(q_e4m3(v, rounding, saturate, emin=-7, vmax=240.0), fnuz=True)
    else:
        codes = encode(q_e4m3(v, rounding, saturate))
    S = scale.view(-1)
    if report_factor is not None:
        S = S * torch.tensor(report_factor, dtype=torch.float32)
    return codes, S


def random_case(rows, C, seed, offset=0.3, spread=1.5):
    """(x fp16 [rows, C], gamma, beta fp32 [C]) of the random tier: x = randn spread + offset; gamma = 1 + 0.1 randn with a few entries 0
    and a few negative; beta = 0.1 randn with a few entries exactly 0."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * spread + offset).half()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    p = torch.randperm(C, generator=g)
    gamma[p[:3]] = 0.0
    gamma[p[3:6]] = -gamma[p[3:6]].abs() - 0.5
    beta[p[2:5]] = 0.0                                           # one of them where gamma is 0 too: y = 0 exactly
    beta[p[8:10]] = 0.0
    return x, gamma, beta


RANDOM_CASES = ((5, 16), (7, 64), (33, 320), (9, 512), (9, 528), (17, 640), (6, 1024), (6, 1040), (33, 1280), (5, 1536), (5, 1552), (5, 2048))
FAR_MEAN_CASE = (100, 320, 6.0)      # x = randn 1.5 + 6: the mean far above the standard deviation
STRIDED_CASE = (5, 1040)             # ldx = C + 8, ldy = C + 16


def random_tier():
    """(name, x, gamma, beta) of every random-tier launch of test_f8gate_gpu.py; test_f8gate_cpu.py asserts the cap for each."""
    for i, (rows, C) in enumerate(RANDOM_CASES):
        yield (f"random {rows}x{C}",) + random_case(rows, C, 100 + i)
    rows, C, off = FAR_MEAN_CASE
    yield (f"far mean {rows}x{C}",) + random_case(rows, C, 200, offset=off)
    rows, C = STRIDED_CASE
    yield (f"strided {rows}x{C}",) + random_case(rows, C, 300)


def tiny_case(C=32, rows=3):
    """gamma = 0, beta = +-1e-39 (fp32 subnormals, alternating signs): max|y| / 448 is below 448 2^-128."""
    x = (torch.randn(rows, C, generator=torch.Generator().manual_seed(1)) * 1.5).half()
    beta = torch.full((C,), 1e-39) * (1 - 2 * (torch.arange(C) % 2))
    assert bool((beta != 0).all()) and bool((beta.abs() < F32_MIN_NORMAL).all())
    return x, torch.zeros(C), beta


def tiny_check(codes, S, beta):
    """What a row below the floor must come out as: no NaN code, S finite, normal and positive, |y8 S - y| <= S 2^-10 + dy."""
    codes, s = codes.cpu(), S.cpu().double().view(-1, 1)
    assert bool(((codes & 0x7F) != 0x7F).all()), f"NaN codes: {codes[0].tolist()}"
    assert bool((torch.isfinite(s) & (s >= F32_MIN_NORMAL)).all()), f"scale not finite, normal and positive: {S.tolist()}"
    y = beta.double().view(1, -1)
    err = (decode(codes) * s - y).abs()
    assert bool((err <= s * 2.0 ** -10 + 4 * U32 * y.abs()).all()), f"|y8 S - y| up to {err.max().item():.3g} with S {S.tolist()}"


# ---- exact tier -------------------------------------------------------------------------------------------------------------------------
def decision_values():
    """V fp32 [1010] and the byte each must become: the 127 magnitudes, the 126 midpoints and the fp32 neighbour on either side of each
    midpoint, both signs.  The expectation is q_e4m3 of the value in fp64 (a midpoint goes to the even code; 2^-10 goes to zero)."""
    mag = _OCP[:127].numpy()
    mid = (mag[:-1] + mag[1:]) / 2
    mid32 = mid.astype(np.float32)
    assert (mid32.astype(np.float64) == mid).all()
    pos = np.concatenate([mag.astype(np.float32), mid32, np.nextafter(mid32, np.float32(-np.inf)), np.nextafter(mid32, np.float32(np.inf))])
    v = np.concatenate([pos, -pos]).astype(np.float32)
    return v, encode(q_e4m3(torch.from_numpy(v.astype(np.float64)))).numpy()


def exact_rows(C, k, rows=5, seed=0):
    """The launches of the exact tier at width C and scale 2^k: a list of dicts with x fp16 [rows, C] (random; the last row constant:
    variance 0, rstd = eps^-1/2), gamma = 0, beta fp32 [C] = decision values 2^k, and want uint8 [C], the byte of every column (the
    same in every row).  beta is shared by the rows of a launch, so V (1010 values) is laid over ceil(1010 / (C - 2)) launches, repeated
    cyclically until the row is full (every 512-column chunk of a VPL > 1 row converts decision points); the last two columns hold
    +448 2^k and -448 2^k, so every launch has the scale 2^k exactly.  zero[c] marks the columns whose value is zero or rounds to it."""
    v, want = decision_values()
    slots = C - 2
    n = -(-len(v) // slots)
    g = torch.Generator().manual_seed(seed + C + 7 * (k + 3))
    out = []
    for j in range(n):
        idx = (np.arange(slots) + j * slots) % len(v)
        b = np.concatenate([v[idx], np.float32([448.0, -448.0])])
        w = np.concatenate([want[idx], np.uint8([0x7E, 0xFE])])
        beta = (b * np.float32(2.0 ** k)).astype(np.float32)
        assert (beta.astype(np.float64) == b.astype(np.float64) * 2.0 ** k).all()
        x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).half()
        x[rows - 1] = 0.75
        out.append(dict(x=x, gamma=torch.zeros(C), beta=torch.from_numpy(beta), want=torch.from_numpy(w), k=k,
                        zero=torch.from_numpy((w & 0x7F) == 0), negative=torch.from_numpy(np.signbit(b))))
    return out


def exact_mismatch(codes, case):
    """Columns of codes [rows, C] whose byte is not the expected one.  A negative value that is zero or rounds to it may come out as 0x80
    or 0x00 (the report says which); everything else is compared as bytes.
    -> (bad mask [rows, C], bytes seen for negative non-zero values that round to zero, bytes seen for -0 itself: there the sign of
    y = (x - mean) * rstd * 0 + (-0) is the sign of x - mean, so both bytes are expected)."""
    codes = codes.cpu()
    want = case["want"].view(1, -1).expand_as(codes)
    negz = (case["zero"] & case["negative"]).view(1, -1).expand_as(codes)
    tiny = negz & (case["beta"] != 0).view(1, -1)
    bad = torch.where(negz, (codes & 0x7F) != 0, codes != want)
    return bad, set(codes[tiny].tolist()), set(codes[negz & ~tiny].tolist())


# ---- ops.pack_linear_f8 -----------------------------------------------------------------------------------------------------------------
def pack_gate(w, w8, scale, what="pack_linear_f8", check=True):
    """ops.pack_linear_f8 (host code; torch converts) on w fp32 [N, K]: codes within the admissible interval of w64 / scale with only the
    division's 2^-24 |t| as dt, scale within 2^-24 relative of max(amax / 448, 2^-100) (1 for an all-zero row), no NaN code, +-448 in
    every row whose amax / 448 is at or above the floor."""
    g = Gate(what)
    w64, s = w.double(), scale.double()
    amax = w64.abs().amax(1)
    s_ref = torch.where(amax > 0, (amax / E4M3_MAX).clamp(min=SCALE_FLOOR), torch.ones_like(amax))
    t = w64 / s.view(-1, 1)
    _intervals(g, decode(w8), t, U32 * t.abs(), 1.0)
    ratio = (s - s_ref).abs() / (U32 * s_ref)
    g.scale_ratio = float(ratio.max())
    if not bool((torch.isfinite(s) & (s >= F32_MIN_NORMAL)).all()):
        g.failed["scale not finite, normal and positive"] = str(scale.tolist()[:8])
    elif g.scale_ratio > 1.0:
        g.failed["scale"] = f"|scale - amax / 448| = {g.scale_ratio:.3g} of 2^-24 relative in row {int(torch.argmax(ratio))}"
    need = amax / E4M3_MAX >= SCALE_FLOOR
    top = ((w8 & 0x7F) == 0x7E).any(1)
    if not bool(top[need].all()):
        g.failed["row maximum"] = f"no +-448 in rows {torch.nonzero(need & ~top).view(-1).tolist()[:8]}"
    if tuple(w8.shape) != tuple(w.shape) or w8.dtype != torch.uint8 or not w8.is_contiguous():
        g.failed["codes layout"] = f"{tuple(w8.shape)} {w8.dtype} contiguous={w8.is_contiguous()}"
    if tuple(scale.shape) != (w.shape[0],) or scale.dtype != torch.float32 or not scale.is_contiguous():
        g.failed["scale layout"] = f"{tuple(scale.shape)} {scale.dtype} contiguous={scale.is_contiguous()}"
    return g.check() if check else g
