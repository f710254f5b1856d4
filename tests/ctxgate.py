"""Per-element accuracy gate for the multi-token cross-attention kernel, ctx_attn_kernel<RW, AM> (pbe_amd/csrc/ctx_attention.hip), reached
through pbe_ctx_attention_f16 / _w_f16 / _rw_f16 / _map_f16.  Helpers imported by test_ctxgate_cpu.py, test_ctxgate_gpu.py and the
_gate functions of the four older ctx test files.  Not a conftest: plain functions only, on the CPU.

One `table` [B, N, Nk] (log2 domain, -inf = absent; fp32 values, as sent) stands for the three launch forms, as in mapref: None is the
plain launch, log2 w[b, j] on every row the weighted one, a regional table the row-weight one.  The fp64 reference is ctxref.reference /
regionref.reference: written from LayerNorm(x) itself.  Every constant is tilecheck's / accgate's (U16 = 2^-11, U32 = 2^-24, ACC_C, LN2,
REL_L2_FACTOR); none is fitted to a run.

The bound, term by term from the kernel text
--------------------------------------------
Statistics (`tid < CTX_TM` branch).  a = sum_z stats[z, m, 0], q = sum_z stats[z, m, 1] in fp32, in order: parts - 1 roundings each,
    d_a = (parts - 1) U32 sum_z |a_z|,  d_q = (parts - 1) U32 sum_z q_z.
mean = a / C and var = q / C - mean^2 are formed in fp64 (no rounding counted), var is rounded to fp32, max(var, 0) + eps is an fp32 add,
v_rsq_f32 is good to 1 ulp = 2 U32, and nmr = -(float)mean * rstd rounds the mean and the product.  With mean_s, var_s, v_s = max(var_s, 0)
+ eps, rstd_s = v_s^-1/2 the fp64 values of the partials AS SENT:
    d_mean = d_a / C,  d_var = d_q / C + 2 |mean_s| d_mean + d_mean^2 + U32 |var_s|,  d_v = d_var + U32 eps + U32 v_s,
    rho    = d_v / (2 (v_s - d_v)) + 2 U32                                      relative error of rstd
    d_mf   = d_mean + U32 |mean_s|                                                error of (float)mean
Scores (log2 domain).  s = fmaf(rstd, acc, fmaf(nmr, colsum, kb)), kb = kbias [+ log2w | + log2rw] (one fp32 add, U32 |kb|); nmr carries
rstd's error, so rstd's relative error multiplies the CANCELLED quantity core = rstd_s (D - mean_s colsum), D = x . kq exact:
    d_acc = ACC_C U32 sqrt(C) sum_c |x_c kq_c|                                   the fp32 MFMA sum over C
    d_s   = rho |core| + rstd_s (1 + rho) (d_acc + d_mf |colsum|)
          + U32 (1 + rho) |nmr colsum|                                            the product -(float)mean * rstd, rounded
          + U32 (|nmr colsum| + |kb|) + U32 (|rstd_s D| + |nmr colsum| + |kb|)    the two fmaf: they carry |nmr colsum| and |rstd acc|, not |s|
          + U32 |kb|                                                              kbias + log2w / log2rw
          + |s_s - s_ref|                                                         s_s = core + kb: the statistics as sent against those of x,
                                                                                  and colsum as sent against sum_c kq; evaluated in fp64
An absent token (kb = -inf) has s = -inf and weight 0 exactly in kernel and reference: d_s = 0 there.
Weights.  The group maximum is the kernel's own, and any common shift cancels in the normalisation; v - mx is one fp32 subtraction
(U32 |s - smax| in the exponent), v_exp_f32 is good to 1 ulp (2 U32), the sum over Nk is Nk - 1 fp32 adds of positive terms, 1.0f / sum
is taken at 1 ulp and e * inv rounds once more: kappa = (Nk + 2) U32.  With G_j = expm1(ln 2 (d_s + U32 |s_j - smax|)) + 2 U32:
    cw_j = w_j ((1 + G_j) / (1 - sum_i w_i G_i) (1 + kappa) - 1)                  the fp32 weight
    c_j  = cw_j (1 + U16) + U16 w_j + 2^-25                                       rounded to fp16 ONCE, after normalising; nothing renormalises,
                                                                                  so sum_j w16_j != 1 by up to Nk 2^-11 and c carries it
Output.  o = sum_(h,j) w16 vo in the fp32 MFMA, then (o + bias) + x in fp32, then the fp16 store:
    d_o   = c @ |vo| + ACC_C U32 sqrt(HJ) ((w + c) @ |vo|)
    d_y   = d_o (1 + 2 U32) + U32 (|term| + |y|)
    bound = d_y (1 + U16) + U16 |y| + 2^-25
The worst case assumes every rounding aligns, so the two whole-tensor terms of ctxref.verdict stay beside it, unchanged: rel-L2 <=
REL_L2_FACTOR x the emulation's, and the _close limit CLOSE["attention"].  The emitted row statistics keep the limits of
test_kernel_against_fp64_reference.
Map.  The head-mean map keeps mapref.verdict, unchanged.  Beside it every map element is held to the weights' own bound, with the fp16
rounding at its exact size - half an ulp of the binade the weight lies in, hulp(v) = max(2^(floor(log2 v) - 11), 2^-25), not U16 v:
    m_bound = mean_h (cw + hulp(w + cw)) (1 + (H + 1) U32) + (H + 1) U32 m      H - 1 fp32 adds, the rounded 1 / H, the product
At H = 1 the map IS the fp16 weight, so this is the one place where a second rounding of the weights shows (fault w16_first).

Recipes (operands(shape, recipe)): unit - ctxref.random_operands; quiet - its x times 2^-4 (LayerNorm removes the scale, so the term
stays and |X| << |term|: the fp16 store no longer hides the term); far - rows with mean 16 std; flat - rows of variance about eps = 1e-5
around a per-row offset, rows 0, 63, 64 (where present) and N - 1 of every sample exactly constant (rstd = eps^-1/2); outlier - one channel
per row 30 std from the rest; peaked - one token per (sample, head) ahead by 32 log2 units in kbias, the weighted form with tokens at
-inf (never a whole sample), the row-weight form with every third row keeping exactly one token.

Exact pins (pin_case): integer x, bias and vo.  plain: every kq row of a head equal (integers in {-1, 0, 1}: every partial sum of the
first MFMA is exact in any order) and kbias constant per head, so all Nk scores of a (row, head) are the same fp32 number, e = 1, sum =
Nk, and for Nk in {2, 4, 8, 16} every weight is exactly 1 / Nk.  weighted: per sample all tokens but j(b) at -inf, so the weights are
exactly one-hot whatever the scores.  row-weight: one token j(b, t) = (t + 3 b + t // 64) % Nk kept per row, changing from every row to
the next and across every tile seam; the map of that launch is exactly one-hot.  |y| < 128 with quantum 1 / 16: representable.
"""
from __future__ import annotations

import math

import torch

import ctxref as cr
import kbiasref as kr
import mapref as mr
import regionref as rr
from accgate import ACC_C, LN2, U16, U32, rel_l2

EPS = cr.EPS
INF = math.inf
TM = 64                                                             # CTX_TM: rows per workgroup

# (B, N, C, H, Nk, parts): the smallest shapes that reach each path ("per-element gate")
NEW_SHAPES = [
    (2, 130, 320, 8, 10, 1),      # NJ = 3; three row tiles per sample, the last with two rows
    (2, 65, 64, 8, 12, 1),        # NJ = 3 at HJ = 96; a second tile holding one row
    (3, 64, 128, 5, 13, 1),       # NJ = 3; HJ = 65: a Vo chunk that is all padding but one column; tokens exactly one tile
    (2, 72, 64, 1, 16, 2),        # H = 1: one softmax group per row
    (2, 40, 192, 16, 8, 1),       # H = 16: NJ = 4 with tokens < 64 and B > 1
]
VIEW_SHAPE = (2, 72, 64, 8, 4, 1)                                   # run as a view: ldx, ldy above C, ln_stats_ld above M
RECIPES = ("unit", "quiet", "far", "flat", "outlier", "peaked")
FORMS = ("plain", "weights", "regions")
ORDERS = ("forward", "reverse", "permuted")
GRIDS = {130: (10, 13), 65: (5, 13), 64: (4, 16), 72: (8, 9), 40: (5, 8)}       # N -> the non-square grid of the regional table
# exact pins: (B, N, C, H, Nk).  Every form has an NJ = 3 shape and one whose tokens are no multiple of 64.
PIN_SHAPES = {
    "plain": [(2, 130, 128, 5, 16), (2, 72, 64, 8, 4), (1, 64, 320, 16, 8), (2, 65, 64, 8, 2)],
    "weights": [(2, 130, 320, 8, 10), (3, 64, 128, 5, 13), (2, 72, 64, 8, 5)],
    "regions": [(2, 130, 320, 8, 10), (3, 64, 128, 5, 13), (2, 72, 64, 8, 5)],
}


def shape_id(s):
    return "B%d-N%d-C%d-H%d-K%d-p%d" % tuple(s[:6]) if len(s) >= 6 else "B%d-N%d-C%d-H%d-K%d" % tuple(s)


def nj_of(shape):
    return (shape[3] * shape[4] + 31) // 32


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _with_x(o, x, parts):
    return cr.Operands(x, o.kq, o.colsum, o.kbias, o.vo, o.bias, cr.row_partials(x, parts), o.B, o.N, o.C, o.H, o.Nk)


def operands(shape, recipe="unit", seed=0):
    """ctxref.Operands of a named recipe (module docstring) at shape (B, N, C, H, Nk, parts)."""
    B, N, C, H, Nk, parts = shape
    o = cr.random_operands(B, N, C, H, Nk, parts, seed=seed)
    if recipe == "unit":
        return o
    g = torch.Generator().manual_seed(77000 + 131 * seed + 7 * C + Nk + RECIPES.index(recipe))
    M = B * N
    if recipe == "quiet":
        return _with_x(o, (o.x.float() * 2.0 ** -4).half(), parts)
    if recipe == "far":
        sd = 0.5 + 0.5 * torch.rand(M, 1, generator=g)
        sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
        return _with_x(o, (torch.randn(M, C, generator=g) * sd + 16.0 * sd * sign).half(), parts)
    if recipe == "flat":
        off = (torch.rand(M, 1, generator=g) - 0.5) * 0.5
        sd = math.sqrt(EPS) * (0.5 + 1.5 * torch.rand(M, 1, generator=g))
        x = (off + sd * torch.randn(M, C, generator=g)).half()
        for b in range(B):
            for t in {0, min(63, N - 1), min(64, N - 1), N - 1}:
                x[b * N + t] = x[b * N + t, 0]
        return _with_x(o, x, parts)
    if recipe == "outlier":
        x = o.x.float()
        ch = torch.randint(0, C, (M, 1), generator=g)
        sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
        x.scatter_(1, ch, x.mean(1, keepdim=True) + 30.0 * sign * x.std(1, keepdim=True))
        return _with_x(o, x.half(), parts)
    assert recipe == "peaked", recipe
    top = torch.randint(0, Nk, (B, H, 1), generator=g)
    kb = o.kbias.clone().view(B, H, Nk)
    kb.scatter_add_(2, top, torch.full((B, H, 1), 32.0))
    return cr.Operands(o.x, o.kq, o.colsum, kb.view(B, H * Nk), o.vo, o.bias, o.stats, B, N, C, H, Nk)


def form_table(shape, recipe, form, seed=0):
    """fp32 table [B, N, Nk] of the form (None: plain), and for `weights` the log2 w [B, Nk] the launch is sent."""
    B, N, C, H, Nk, parts = shape
    if form == "plain":
        return None, None
    if form == "weights":
        if recipe == "peaked":
            j = torch.arange(Nk)[None, :]
            b = torch.arange(B)[:, None]
            g = torch.Generator().manual_seed(88000 + C + Nk + seed)
            lw = (3.0 * torch.randn(B, Nk, generator=g)).float()
            lw = torch.where((j + b) % 3 == 1, torch.full_like(lw, -INF), lw)       # Nk >= 2: tokens j = 0 or 1 of every sample stay
        else:
            lw = torch.log2(kr.ctx_weights(B, Nk, 11 + C + seed)).float()
        return lw[:, None, :].expand(B, N, Nk).contiguous(), lw
    assert form == "regions", form
    tab = rr.kernel_case(tuple(shape) + GRIDS[N], seed)["table"].float()
    if recipe == "peaked":
        t = torch.arange(N)
        keep = ((t[None, :] + 3 * torch.arange(B)[:, None]) % Nk)                  # [B, N]
        lone = torch.full((B, N, Nk), -INF).scatter_(2, keep[:, :, None], 0.0)
        tab = torch.where((t % 3 == 0)[None, :, None], lone, tab)
    return tab.contiguous(), None


def next_sample_table(shape, seed=0):
    """regionref's `next_sample` mutation at the shape: sample b takes the table of sample b + 1 (drawn for B + 1 samples)."""
    return rr.kernel_case(tuple(shape) + GRIDS[shape[1]], seed)["next_sample"].float().contiguous()


# ---- reference and bound ---------------------------------------------------------------------------------------------------------------
def reference(o, table=None, eps=EPS):
    """(want, bound, map, map bound) fp64: Y [B * N, C] from LayerNorm(x) itself, the module docstring's bound on every element, the
    head-mean softmax [B, N, Nk] and its own per-element bound (module docstring, "Map")."""
    B, N, H, Nk, C = o.B, o.N, o.H, o.Nk, o.x.shape[1]
    HJ = H * Nk
    x = o.x.double().view(B, N, C)
    kq, cs = o.kq.double(), o.colsum.double()[:, None, :]
    vo, bias = o.vo.double()[:, :, :HJ], o.bias.double()
    tab = torch.zeros(B, N, Nk, dtype=torch.float64) if table is None else table.float().double()
    kb = (o.kbias.double().view(B, 1, H, Nk) + tab[:, :, None, :]).reshape(B, N, HJ)
    live = torch.isfinite(kb)
    kba = torch.where(live, kb.abs(), torch.zeros_like(kb))
    zero = torch.zeros_like(kb)
    # the reference: LayerNorm(x) itself
    mean_x = x.mean(-1, keepdim=True)
    xh = (x - mean_x) / torch.sqrt(((x - mean_x) ** 2).mean(-1, keepdim=True) + eps)
    s_ref = xh @ kq.transpose(1, 2) + kb
    # the statistics as sent
    st = o.stats.double()
    parts = st.shape[0]
    a_s, q_s = st[:, :, 0].sum(0).view(B, N, 1), st[:, :, 1].sum(0).view(B, N, 1)
    d_a = (parts - 1) * U32 * st[:, :, 0].abs().sum(0).view(B, N, 1)
    d_q = (parts - 1) * U32 * st[:, :, 1].abs().sum(0).view(B, N, 1)
    mean_s = a_s / C
    var_s = q_s / C - mean_s * mean_s
    v_s = var_s.clamp_min(0.0) + eps
    rstd_s = v_s ** -0.5
    d_mean = d_a / C
    d_var = d_q / C + 2 * mean_s.abs() * d_mean + d_mean ** 2 + U32 * var_s.abs()
    d_v = d_var + U32 * eps + U32 * v_s
    rho = d_v / (2 * (v_s - d_v)) + 2 * U32
    d_mf = d_mean + U32 * mean_s.abs()
    D = x @ kq.transpose(1, 2)
    core = rstd_s * (D - mean_s * cs)
    nc = (rstd_s * mean_s * cs).abs()
    d_acc = ACC_C * U32 * math.sqrt(C) * (x.abs() @ kq.abs().transpose(1, 2))
    dist = torch.where(live, (core + kb - s_ref).abs(), zero)
    d_s = rho * core.abs() + rstd_s * (1 + rho) * (d_acc + d_mf * cs.abs()) + U32 * (1 + rho) * nc + U32 * (nc + kba) \
        + U32 * ((rstd_s * D).abs() + nc + kba) + U32 * kba + dist
    d_s = torch.where(live, d_s, zero).view(B, N, H, Nk)
    # weights
    s4 = s_ref.view(B, N, H, Nk)
    smax = s4.max(-1, keepdim=True).values
    e = torch.exp2(s4 - smax)
    w = e / e.sum(-1, keepdim=True)
    below = torch.where(live.view(B, N, H, Nk), (s4 - smax).abs(), zero.view(B, N, H, Nk))
    G = torch.expm1(LN2 * (d_s + U32 * below)) + 2 * U32
    kappa = (Nk + 2) * U32
    cw = w * ((1 + G) / (1 - (w * G).sum(-1, keepdim=True)) * (1 + kappa) - 1)
    c = (cw * (1 + U16) + U16 * w + 2.0 ** -25).view(B, N, HJ)
    wf = w.view(B, N, HJ)
    # output
    va = vo.abs().transpose(1, 2)
    term = wf @ vo.transpose(1, 2) + bias
    y = x + term
    d_o = c @ va + ACC_C * U32 * math.sqrt(HJ) * ((wf + c) @ va)
    d_y = d_o * (1 + 2 * U32) + U32 * (term.abs() + y.abs())
    bound = d_y * (1 + U16) + U16 * y.abs() + 2.0 ** -25
    # map: the fp16 weights summed over h in fp32 (H - 1 adds), times the rounded 1 / H (two more roundings)
    up = w + cw
    hulp = torch.exp2(torch.floor(torch.log2(up.clamp_min(2.0 ** -14))) - 11)
    m = w.mean(2)
    m_bound = (cw + hulp).mean(2) * (1 + (H + 1) * U32) + (H + 1) * U32 * m
    return y.view(B * N, C), bound.view(B * N, C), m, m_bound


# ---- the kernel's arithmetic in plain fp32 torch ---------------------------------------------------------------------------------------
FAULTS = ("w16_first", "drop_colsum", "clamp_early", "block2_from_block0", "drop_kbias_column", "log2w_by_head", "map_div_nk")


def _perm(n, order, seed):
    if order == "forward":
        return torch.arange(n)
    if order == "reverse":
        return torch.arange(n - 1, -1, -1)
    assert order == "permuted", order
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 numbers is exact in fp64, and so (but for a double rounding) is the sum."""
    return (a.double() * b.double() + c.double()).float()


def emulate(o, table=None, eps=EPS, order="forward", fault=None, log2w=None):
    """(Y fp16 [B * N, C], map fp32 [B, N, Nk]): ctx_attn_kernel restated in fp32 - the partials summed in order, mean and variance in
    fp64, rsqrt, the two fmaf, the group maximum subtracted, exp2, the sum over Nk in order, one division, the weights rounded to fp16
    once, the fp32 sum over (h, j), + bias, + x, the fp16 store; the map summed over h in order, times the fp32 value 1 / H.  order: the
    summation order of BOTH MFMA sums (over C and over H Nk): forward, reverse, or a seeded permutation.  eps and `fault` plant the
    faults the gate must reject (FAULTS; test_ctxgate_cpu.py says what each one is).  log2w [B, Nk]: what the weighted launch is sent,
    needed by the fault log2w_by_head only."""
    assert fault is None or fault in FAULTS, fault
    B, N, H, Nk, C = o.B, o.N, o.H, o.Nk, o.x.shape[1]
    HJ = H * Nk
    st = o.stats.float()
    a, q = torch.zeros_like(st[0, :, 0]), torch.zeros_like(st[0, :, 1])
    for z in range(st.shape[0]):
        a, q = a + st[z, :, 0], q + st[z, :, 1]
    inv_c = 1.0 / C
    mean = a.double() * inv_c
    var = (q.double() * inv_c - mean * mean).float()
    rstd = torch.rsqrt(var.clamp_min(0.0) + torch.tensor(eps, dtype=torch.float32)).view(B, N, 1)
    nmr = (-(mean.float())).view(B, N, 1) * rstd
    x = o.x.float().view(B, N, C)
    pc = _perm(C, order, 1000 + C)
    acc = x[:, :, pc] @ o.kq.float()[:, :, pc].transpose(1, 2)
    if fault == "block2_from_block0" and HJ > 64:
        acc = acc.clone()
        acc[:, :, 64:HJ] = acc[:, :, :HJ - 64]
    kbias = o.kbias.float()
    if fault == "drop_kbias_column":                                # the column of sample B - 1 with the largest |kbias| among the live tokens
        kbias = kbias.clone()
        live = torch.ones(Nk, dtype=torch.bool) if table is None else torch.isfinite(table[B - 1]).any(0)
        kbias[B - 1, int(torch.argmax(kbias[B - 1].abs() * live.repeat(H)))] = 0.0
    kb = kbias.view(B, 1, H, Nk)
    if table is not None:
        tab = table.float()
        if fault == "clamp_early":                                  # min(row0 + r, tokens - 2): a sample's last row reads the row before
            tab = tab[:, torch.arange(N).clamp_max(max(N - 2, 0))]
        tab4 = tab.view(B, N, 1, Nk)
        if fault == "log2w_by_head" and log2w is not None:           # column c = (h, j) takes log2w[c / Nk] instead of log2w[c % Nk]
            col = torch.arange(HJ)
            tab4 = log2w.float()[:, (col // Nk) % Nk].view(B, 1, H, Nk)
        kb = kb + tab4                                              # the fp32 add comes first
    kb = kb.expand(B, N, H, Nk).reshape(B, N, HJ)
    cs = o.colsum.float()[:, None, :]
    inner = kb if fault == "drop_colsum" else _fma(nmr.expand(B, N, HJ), cs.expand(B, N, HJ), kb)
    v = _fma(rstd.expand(B, N, HJ), acc, inner).view(B, N, H, Nk)
    mx = v.max(-1, keepdim=True).values
    e = torch.exp2(v - mx)
    if fault == "w16_first":
        e = e.half().float()
    tot = torch.zeros_like(e[..., 0])
    for j in range(Nk):
        tot = tot + e[..., j]
    w = (e * (1.0 / tot)[..., None]).half().float()                 # [B, N, H, Nk], fp16 values
    ph = _perm(HJ, order, 2000 + HJ)
    y = w.view(B, N, HJ)[:, :, ph] @ o.vo.float()[:, :, :HJ][:, :, ph].transpose(1, 2)
    y = ((y + o.bias.float()) + x).half().view(B * N, C)
    m = torch.zeros(B, N, Nk, dtype=torch.float32)
    for h in range(H):
        m = m + w[:, :, h]
    div = Nk if fault == "map_div_nk" else H
    return y, m * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(div), dtype=torch.float32))


# ---- verdicts --------------------------------------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self, ok, ratio, where, text, old_ok, r_got, r_emu):
        self.ok, self.ratio, self.where, self.text, self.old_ok, self.r_got, self.r_emu = ok, ratio, where, text, old_ok, r_got, r_emu

    def __str__(self):
        return self.text


def locate(i, N, C):
    """'sample b, row t, channel c, row tile k' of flat element i of Y [B * N, C]."""
    m, c = divmod(int(i), C)
    b, t = divmod(m, N)
    return f"sample {b}, row {t}, channel {c}, row tile {t // TM}"


def verdict(got, o, table=None, eps=EPS, ref=None, emu=None):
    """The gate on Y `got` (fp16 [B * N, C]): ctxref.verdict's two terms, unchanged, and every element within its bound of the fp64
    reference.  ref / emu: reference(o, table) / emulate(o, table)[0] when the caller has them already (both are of the INTACT
    operands and the right eps, never of what a control changed)."""
    got = got.detach().cpu()
    want, bound = (ref if ref is not None else reference(o, table, eps))[:2]
    if emu is None:
        emu = emulate(o, table, eps)[0]
    old_ok, old_text = cr.verdict(got, want, emu)
    gd = got.double()
    r = torch.where(torch.isfinite(gd), (gd - want).abs() / bound, torch.full_like(want, INF))
    i = int(torch.argmax(r))
    ratio = float(r.view(-1)[i])
    where = locate(i, o.N, want.shape[1])
    finite = bool(torch.isfinite(gd).all())
    text = f"worst err/bound {ratio:.3f} at {where}; {old_text}"
    return Verdict(old_ok and ratio <= 1.0, ratio, where, text, old_ok, rel_l2(got, want) if finite else INF, rel_l2(emu, want))


def map_verdict(got, o, table=None, eps=EPS, ref=None, emu=None):
    """(accepted, worst err/bound, where, text): mapref.verdict, unchanged, of the head-mean map `got` [B, N, Nk] against
    reference(o, table), and every element within the module docstring's map bound."""
    want, m_bound = (ref if ref is not None else reference(o, table, eps))[2:]
    if emu is None:
        emu = emulate(o, table, eps)[1]
    got = got.detach().cpu()
    ok, text = mr.verdict(got, want, emu, None if table is None else table.double())
    gd = got.double()
    r = torch.where(torch.isfinite(gd), (gd - want).abs() / m_bound, torch.full_like(want, INF))
    i = int(torch.argmax(r))
    ratio = float(r.view(-1)[i])
    m, j = divmod(i, o.Nk)
    where = f"sample {m // o.N}, row {m % o.N}, token {j}, row tile {m % o.N // TM}"
    return ok and ratio <= 1.0, ratio, where, f"map worst err/bound {ratio:.3f} at {where}; {text}"


def applies(fault, shape, recipe, form, table=None):
    """Whether a planted fault must be rejected on the case, decided from what the fault is, never from a run (test_ctxgate_cpu.py says
    why for each): elsewhere the verdicts on it are recorded only."""
    B, N, C, H, Nk = shape[:5]
    HJ = H * Nk
    if fault in ("eps0", "eps1e-6"):
        return recipe == "flat"
    if fault == "drop_colsum":
        return recipe != "peaked"
    if fault == "drop_kbias_column":
        return recipe != "peaked"
    if fault == "block2_from_block0":
        if nj_of(shape) != 3 or recipe == "peaked":
            return False
        return table is None or bool(torch.isfinite(table[:, :, torch.arange(64, HJ) % Nk]).any())
    if fault == "log2w_by_head":
        return form == "weights"
    if fault == "map_div_nk":
        return H != Nk
    if fault == "w16_first":
        return H == 1 and recipe not in ("peaked", "far")
    raise AssertionError(fault)


# ---- exact pins ------------------------------------------------------------------------------------------------------------------------
def pin_token(b, t, Nk):
    return (t + 3 * b + t // TM) % Nk


def pin_case(form, shape, seed=0):
    """(Operands, table fp32 or None, log2w or None, expected Y fp64 [B * N, C], expected map fp64 [B, N, Nk]) of an exact pin."""
    B, N, C, H, Nk = shape
    HJ = H * Nk
    g = torch.Generator().manual_seed(91000 + 17 * seed + 3 * C + Nk + FORMS.index(form))
    x = torch.randint(-8, 9, (B * N, C), generator=g).half()
    bias = torch.randint(-8, 9, (C,), generator=g).float()
    vo = torch.randint(-4, 5, (B, C, HJ), generator=g).half()
    if form == "plain":
        assert Nk in (2, 4, 8, 16)
        kq = torch.randint(-1, 2, (B, H, 1, C), generator=g).expand(B, H, Nk, C).reshape(B, HJ, C).half()
        kbias = torch.randint(-3, 4, (B, H, 1), generator=g).expand(B, H, Nk).reshape(B, HJ).float()
    else:
        kq = (torch.randn(B, HJ, C, generator=g) * (2.0 / C ** 0.5)).half()
        kbias = (torch.randn(B, HJ, generator=g) * 0.6).float()
    o = cr.Operands(x, kq, kq.double().sum(-1).float(), kbias, vo, bias, cr.row_partials(x, 1), B, N, C, H, Nk)
    v4 = vo.double().view(B, C, H, Nk)
    xb = x.double().view(B, N, C) + bias.double()
    if form == "plain":
        want = xb + (v4.sum((2, 3)) / Nk)[:, None, :]
        return o, None, None, want.view(B * N, C), torch.full((B, N, Nk), 1.0 / Nk, dtype=torch.float64)
    if form == "weights":
        keep = torch.tensor([(2 * b + 1) % Nk for b in range(B)])[:, None].expand(B, N)
    else:
        keep = torch.tensor([[pin_token(b, t, Nk) for t in range(N)] for b in range(B)])
    table = torch.full((B, N, Nk), -INF).scatter_(2, keep[:, :, None], 0.0)
    per_tok = v4.sum(2)                                                             # [B, C, Nk]
    want = xb + torch.gather(per_tok.transpose(1, 2), 1, keep[:, :, None].expand(B, N, C))
    hot = torch.zeros(B, N, Nk, dtype=torch.float64).scatter_(2, keep[:, :, None], 1.0)
    return o, table, (table[:, 0].contiguous() if form == "weights" else None), want.view(B * N, C), hot
