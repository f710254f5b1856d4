"""Per-element gate for the activation arms of the GEMM / conv epilogue (pbe_amd/csrc/common.h silu_f, quick_gelu_f, gelu_erf_f, apply_act,
apply_act4; applied in igemm_kernel.h stage() and splitk_reduce_kernel): act = 1 SiLU, 2 erf-GELU, 3 quick-GELU, 4 GEGLU.  Helpers imported by
test_actgate_cpu.py, test_actgate_gpu.py and tilecheck.expect().  Not a conftest: plain functions only.

Rounding model.  U32 = 2^-24, U16 = 2^-11, GELU_FIT are tilecheck's.  x is the pre-activation the kernel holds in fp32, y = act(x) in fp64.
v_exp_f32 and v_rcp_f32 are taken at 1 ulp = 2 U32 relative each (EXP_ULP, RCP_ULP; common.h says so of v_rcp_f32, AMD's ISA manuals give
1 ulp for both).  The kernel guides of this project carry no accuracy figure for either instruction and nobody has measured them against
fp64 on an MI355X here: both are assumptions of this model, and the GPU gate is what would show them wrong.

  SiLU (k = 1), quick-GELU (k = 1.702): y = x * rcp(1 + exp2(t)), t = fl(c x), c = fl32(-k log2 e).
      c carries n_c roundings: 1 for SiLU (the literal), 3 for quick-GELU (two literals and their fp32 product, folded at compile time or
      not); the product c x one more: |dt| <= (n_c + 1) U32 |t|, and d(2^t) / 2^t = ln 2 dt with ln 2 |t| = k |x|.
      e = exp2(t): relative (n_c + 1) k |x| U32 + EXP_ULP 2 U32.  s = 1 / (1 + e): |ds / s| = e / (1 + e) |de / e| <= |de / e|, the add
      U32, the reciprocal RCP_ULP 2 U32; the final product x s one U32.
          |d act| <= |y| (6 + (n_c + 1) k |x|) U32 + 2^-120
      i.e. (6 + 2 |x|) for SiLU and (6 + 6.808 |x|) for quick-GELU (counting one rounding in c would give 2 k |x| for both).  2^-120
      covers an intermediate that leaves the fp32 range (e = inf -> s = 0, or s below 2^-126) for |x| <= 256: |y| < |x| 2^-128 there.
  GELU: u = |x|, r = R(u) by four fmaf (Horner, PBE_GELU_R0..4), a = fmaf(-u, r, -1), q = exp2(a), result fmaf(-u, q, max(x, 0)).
      Horner with one rounding per step: |dr| <= 4 U32 P(u) with P(u) = sum |R_i| u^i (R3 < 0: the partial sums cancel, so P and not R);
      |da| <= u |dr| + U32 |a| <= 5 U32 (u P(u) + 1) =: 5 U32 A(u).  q: relative 5 ln 2 A(u) U32 + EXP_ULP 2 U32, plus a flush below
      2^-126.  The last fmaf rounds once: U32 |y|.
          |d act| <= GELU_FIT + u q (5 ln 2 A(u) + 2) U32 + U32 |y| + 2^-126 u,    q = 2^-(u R(u) + 1) (the fit's own q, in fp64)
      (A(u) and not |log2 Phi(-u)|: they agree inside the fitted range up to the cancellation in R, and beyond it q = 0 either way).
      GELU_FIT bounds the fit in exact arithmetic: test_actgate_cpu.py checks it in fp64 over the whole table.
  GEGLU: v * gelu(g): |v| (GELU term of g) + U32 |y| for the product.
  pre-activation error: |d pre| times max |act'|: 1.0998 for SiLU and for quick-GELU (x sigmoid(k x) is SiLU rescaled: the same maximum),
      1.1290 for GELU, on an fp64 grid of step 2^-10 over [-24, 24] (test_actgate_cpu.py); ACT_DMAX rounds them up to accgate's 1.1 and
      tilecheck's 1.13.
  store: U16 |y| + 2^-25 on the fp16 value, and again after the residual add (act -> fp16 -> + resid -> fp16, in the fused epilogue and in
      splitk_reduce_kernel alike; the fp32 sum of two fp16 values adds U32 |out|).

Exact-pre-activation operands.  A[m, k] = 1 where k == m % K else 0, so pre[m, n] = alpha W[n, m % K] + bias + rowvec is ONE product and
two additions of values chosen so that every intermediate is exact in fp32 (assert_exact proves it against fp64 before anything is
launched: then the association, the fusion and the split-K slabs cannot matter) and the bound is the activation term plus the store
alone.  W sweeps TABLE = every finite fp16 value in [-24, 24] (39 938 values: both zeros, the subnormals, the tails where the result is
itself an fp16 subnormal); K = 128 (two k-tiles), N = 328 (off the grid of every BN) gives 41 984 slots.  Variants with a non-zero
addend round the table values below 2^-8 to multiples of 2^-18 (2 + 2^-24 has no fp32), the plain-bias variant passes a +0 bias and keeps
every table value as it is.  M = max(BM, K) + 24: a ragged last row tile, every value in at least two rows of different tiles - BM + 24 for
the 128- and 256-row tiles; the 64-row tiles take 152 as well, since 88 rows would reach only 88 of the 128 k.  Forced split-K needs
>= 4 k-tiles per slice (clamp_splits): K = 256 * splits there, and M = K + 24.  GEGLU (N = 656, pack_geglu rows: value rows of +-1, +-2,
0.5, gate rows sweeping TABLE) is accepted with a column bias only, so it runs the +0 bias and a non-zero column bias with alpha 0.5.

Measured on the CPU (test_actgate_cpu.py; worst |emulation - fp64| / bound over every case's operands, the emulation being the plain fp32
restatement below, never a kernel's output):
  whole bound (store included)    SiLU 0.9995   GELU 0.9993   quick-GELU 0.9995   GEGLU 0.9992   (an fp16 near-tie: TABLE has them all)
  activation term alone (before the fp16 store, on TABLE)
                                  SiLU 0.548    GELU 0.749    quick-GELU 0.444               (GELU: the fit itself, 5.36e-7 of 7.1e-7)
  worst ratio of each mutation (> 1 = rejected): tanh-GELU 187, quick-GELU with k = 1.7 20.7, SiLU clamped below -8 2.0e3, activation after
  the fp16 rounding 7.5, activation skipped on the last column tile 6.8e4, residual before the activation 2.3e3.
"""
from __future__ import annotations

import functools
import math
import os
import re

import torch

from tilecheck import GELU_FIT, ROOT, U16, U32

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
EXP_ULP = RCP_ULP = 1.0          # v_exp_f32 / v_rcp_f32, in ulps (assumed: see the docstring)
ACT_K = {1: 1.0, 3: 1.702}
ACT_NC = {1: 1, 3: 3}            # roundings in the fp32 constant -k log2 e
ACT_DMAX = {1: 1.1, 2: 1.13, 3: 1.1}
ACT_NAME = {1: "silu", 2: "gelu", 3: "quick_gelu", 4: "geglu"}
CLOSE_EPILOGUE = (2e-3, 1e-3)    # test_gemm_epilogue's _close limit (tests/test_ops_gpu.py)


@functools.lru_cache(maxsize=None)
def gelu_coeffs():
    """PBE_GELU_R0..4 of pbe_amd/csrc/common.h as Python floats (the fp32 values)."""
    src = open(os.path.join(ROOT, "pbe_amd", "csrc", "common.h")).read()
    return tuple(float(torch.tensor(float(re.search(rf"#define PBE_GELU_R{k} \(?(-?[0-9.e-]+)f\)?", src).group(1)), dtype=torch.float32))
                 for k in range(5))


# ---- tile geometry (igemm_kernel.h kTiles) -----------------------------------------------------------------------------------------
FORM_BITS = {"F_DENSE": 1, "F_CONV": 2, "F_HALO": 4, "F_EX": 8, "F_F8": 16, "F_ASTAT": 32, "F_FORCED": 64}


@functools.lru_cache(maxsize=None)
def tiles():
    """kTiles as [(bm, bn, nwm, nwn, forms, f8 tile)], read from igemm_kernel.h."""
    src = open(os.path.join(ROOT, "pbe_amd", "csrc", "igemm_kernel.h")).read()
    body = src[src.index("static constexpr TileCfg kTiles[] = {"):]
    body = body[:body.index("static constexpr int kNCfg")]
    rows = []
    for m in re.finditer(r"^\s*\{(\d+), (\d+), (\d+), (\d+), \d+, \d+, [0-9.]+, [0-9.]+, \d+, ([A-Z0-9_| ]+), (\d+)\}", body, re.M):
        forms = sum(FORM_BITS[f.strip()] for f in m.group(5).split("|"))
        rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), forms, int(m.group(6))))
    return rows


def acc_regs(tile):
    """Accumulator registers per lane of a tile: TM * TN * 4 (igemm_kernel: ARMS = TM * TN * 4 <= 96)."""
    bm, bn, nwm, nwn, _, _ = tiles()[tile]
    return (bm // nwm // 16) * (bn // nwn // 16) * 4


def dense_tiles(arms):
    """The F_DENSE tiles whose stage() specialises the activation at compile time (arms) / keeps it a run-time branch (not arms)."""
    return [i for i, t in enumerate(tiles()) if t[4] & FORM_BITS["F_DENSE"] and (acc_regs(i) <= 96) == arms]


def f8_tiles():
    return [i for i, t in enumerate(tiles()) if t[4] & FORM_BITS["F_F8"]]


# ---- fp64 references and bounds ----------------------------------------------------------------------------------------------------
def act64(x, act):
    """act(x) in fp64 (GELU through erfc: no cancellation in the negative tail)."""
    x = x.double()
    if act in (1, 3):
        return x / (1 + torch.exp(-ACT_K[act] * x))
    if act == 2:
        return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    return x


def _gelu_fit64(u):
    """(R(u), P(u)) of the kernel's fit in fp64."""
    c = gelu_coeffs()
    r = torch.full_like(u, c[4])
    p = torch.full_like(u, abs(c[4]))
    for k in (3, 2, 1, 0):
        r, p = r * u + c[k], p * u + abs(c[k])
    return r, p


def act_term(x, act):
    """|d act| of an exact fp32 pre-activation x (fp64 tensor): the docstring's bound, before the store."""
    x = x.double()
    y = act64(x, act).abs()
    if act in (1, 3):
        return y * (2 * EXP_ULP + 2 * RCP_ULP + 2 + (ACT_NC[act] + 1) * ACT_K[act] * x.abs()) * U32 + 2.0 ** -120
    if act == 2:
        u = x.abs()
        r, p = _gelu_fit64(u)
        q = torch.exp2(-(u * r + 1))
        return GELU_FIT + u * q * (5 * LN2 * (u * p + 1) + 2 * EXP_ULP) * U32 + U32 * y + 2.0 ** -126 * u
    return torch.zeros_like(x)


def stored(y, dy, resid=None):
    """(want, bound) of the stored fp16 value from the fp64 result y and its error dy before the store; resid: fp16 values added after it."""
    b = dy * (1 + U16) + U16 * y.abs() + 2.0 ** -25
    if resid is None:
        return y, b
    out = y + resid.double()
    return out, b * (1 + U16) + (U16 + U32) * out.abs() + 2.0 ** -25


def expect_exact(pre, act, resid=None):
    """(want, bound) for an EXACT pre-activation [M, N] (fp64): the activation term and the store only.  act 4: interleaved (value, gate)
    columns, resid ignored (as the kernel does)."""
    if act == 4:
        v, g = pre[:, 0::2], pre[:, 1::2]
        y = v * act64(g, 2)
        return stored(y, v.abs() * act_term(g, 2) + U32 * y.abs())
    return stored(act64(pre, act), act_term(pre, act), resid)


# ---- the kernel's arithmetic in plain fp32 torch (the emulation) --------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    """fmaf: the fp32 product is exact in fp64, the sum is rounded once more there (a double rounding that almost never shows)."""
    return (a.double() * b.double() + c.double()).float()


def silu_f32(x, k=1.0):
    """silu_f / quick_gelu_f: x * rcp(1 + exp2(fl32(-k) fl32(log2 e) x)), every step in fp32."""
    c = _f32(-k) * _f32(LOG2E)
    return x * (1.0 / (1.0 + torch.exp2(c * x)))


def gelu_erf_f32(x):
    c = [_f32(v) for v in gelu_coeffs()]
    u = x.abs()
    r = _fma(c[4].expand_as(u), u, c[3])
    for k in (2, 1, 0):
        r = _fma(r, u, c[k])
    q = torch.exp2(_fma(-u, r, _f32(-1.0)))
    return _fma(-u, q, x.clamp_min(0.0))


def act_f32(x, act):
    return silu_f32(x) if act == 1 else gelu_erf_f32(x) if act == 2 else silu_f32(x, 1.702) if act == 3 else x


MUTATIONS = ("tanh_gelu", "quick_1p7", "silu_clamp", "act_after_round", "skip_last_column_tile", "resid_before_act")
MUTATION_ACT = {"tanh_gelu": 2, "quick_1p7": 3, "silu_clamp": 1, "act_after_round": 1, "skip_last_column_tile": 3, "resid_before_act": 2}


def pre_f32(o):
    """The pre-activation as the fused epilogue forms it: fmaf(acc, alpha [a_scale w_scale], bias + rowvec), then + the per-row bias."""
    M, K = o["M"], o["K"]
    acc = o["Wv"].float()[:, torch.arange(M) % K].t().contiguous()                       # the one-hot A picks W[n, m % K]
    add = torch.zeros(M, o["N"])
    if o["bias"] is not None and not o["bias_per_row"]:
        add = add + o["bias"].float()[None, :]
    if o["rowvec"] is not None:
        add = add + o["rowvec"].float()[torch.arange(M) // o["group_rows"]]
    al = _f32(o["alpha"]).expand(M, 1)
    if o.get("a_scale") is not None:
        al = o["a_scale"].float()[:, None] * al
    v = _fma(acc, al.expand_as(acc), add)
    if o["bias_per_row"]:
        v = v + o["bias"].float()[:, None]
    return v


def emulate(o, act, *, resid=False, mutation=None, bn=64):
    """The epilogue in plain fp32 on the operands o of an exact-pre case: fp16 [M, N] (act 4: [M, N / 2]).  mutation: one of MUTATIONS."""
    v = pre_f32(o)
    res = o["resid"].float() if resid and act != 4 else None
    if act == 4:
        return (v[:, 0::2] * gelu_erf_f32(v[:, 1::2])).half()
    if mutation == "tanh_gelu":
        y = torch.nn.functional.gelu(v, approximate="tanh")
    elif mutation == "quick_1p7":
        y = silu_f32(v, 1.7)
    elif mutation == "silu_clamp":
        y = torch.where(v < -8.0, torch.zeros_like(v), act_f32(v, act))
    elif mutation == "act_after_round":
        y = act_f32(v.half().float(), act)
    elif mutation == "skip_last_column_tile":
        y = act_f32(v, act)
        n0 = (o["N"] - 1) // bn * bn
        y[:, n0:] = v[:, n0:]
    elif mutation == "resid_before_act":
        return act_f32(v + o["resid"].float(), act).half()
    else:
        assert mutation is None, mutation
        y = act_f32(v, act)
    h = y.half()
    return h if res is None else (h.float() + res).half()


# ---- exact-pre-activation operands -------------------------------------------------------------------------------------------------
TABLE_MAX = 24.0
BIAS_SET = (0.0, 0.5, -0.5, 2.0, -2.0)
VALUE_SET = (1.0, -1.0, 2.0, -2.0, 0.5)          # GEGLU value columns
VARIANTS = ("bias", "rowbias", "rv_half", "rv48")        # the dense epilogue variants; each with and without the residual
SPLITK_VARIANTS = ("rv48", "rowbias")
GEGLU_VARIANTS = ("bias", "colbias")                     # pbe_gemm_f16 takes GEGLU with a column bias only (no row vector, residual, per-row bias)


def variants_of(act, splits=1):
    return GEGLU_VARIANTS if act == 4 else VARIANTS if splits == 1 else SPLITK_VARIANTS


@functools.lru_cache(maxsize=None)
def table16():
    """Every finite fp16 value with |x| <= 24, ascending bit pattern per sign (+0 ... +24, -0 ... -24)."""
    t = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.float16)
    return t[torch.isfinite(t) & (t.float().abs() <= TABLE_MAX)].clone()


@functools.lru_cache(maxsize=None)
def table8():
    """Every finite OCP e4m3 code (uint8): all bytes but the two NaNs."""
    t = torch.arange(0, 256, dtype=torch.int32).to(torch.uint8)
    return t[(t & 0x7F) != 0x7F].clone()


def _quantise(w):
    """Table values below 2^-8 rounded to multiples of 2^-18 (exact in fp16): alpha w + bias + rowvec then has an fp32."""
    d = w.double()
    return torch.where(d.abs() < 2.0 ** -8, torch.round(d * 2.0 ** 18) / 2.0 ** 18, d).half()


def _sweep(tab, rows, K, shift=0):
    idx = (torch.arange(rows * K) + shift) % tab.numel()
    return tab[idx].view(rows, K)


def _addends(variant, M, N, bm):
    """(bias fp32, bias_per_row, rowvec fp16 or None, group_rows, alpha) of a dense variant."""
    bs = torch.tensor(BIAS_SET, dtype=torch.float32)
    if variant == "bias":
        return torch.zeros(N), False, None, 0, 1.0
    if variant == "rowbias":
        return bs[torch.arange(M) % 5].contiguous(), True, None, 0, 1.0
    if variant == "colbias":
        return bs[torch.arange(N) % 5].contiguous(), False, None, 0, 0.5
    grp = bm // 2 if variant == "rv_half" else 48
    G = (M + grp - 1) // grp
    rv = (((7 * torch.arange(G)[:, None] + 3 * torch.arange(N)[None, :]) % 33 - 16).float() / 16.0).half()
    return bs[torch.arange(N) % 5].contiguous(), False, rv, grp, 0.5


def _pre64(o):
    M, K = o["M"], o["K"]
    pre = o["alpha"] * o["Wv"].double()[:, torch.arange(M) % K].t().contiguous()
    if o.get("a_scale") is not None:
        pre = pre * o["a_scale"].double()[:, None]
    if o["bias"] is not None:
        pre = pre + (o["bias"].double()[:, None] if o["bias_per_row"] else o["bias"].double()[None, :])
    if o["rowvec"] is not None:
        pre = pre + o["rowvec"].double()[torch.arange(M) // o["group_rows"]]
    return pre


def assert_exact(o):
    """The fp32 evaluation of the pre-activation, in the fused epilogue's association and in splitk_reduce_kernel's (unfused product, then
    the sum), equals the fp64 evaluation bit for bit; the fp64 one is exact (one product of <= 11 + 24 bits, sums inside 2^5 .. 2^-25)."""
    pre = o["pre"]
    assert torch.equal(pre_f32(o).double(), pre), "fused association is not exact on these operands"
    M, K = o["M"], o["K"]
    acc = o["Wv"].float()[:, torch.arange(M) % K].t().contiguous()
    ev = torch.zeros(M, o["N"])
    if o["bias"] is not None:
        ev = ev + (o["bias"].float()[:, None] if o["bias_per_row"] else o["bias"].float()[None, :])
    if o["rowvec"] is not None:
        ev = ev + o["rowvec"].float()[torch.arange(M) // o["group_rows"]]
    scale = _f32(o["alpha"]) if o.get("a_scale") is None else o["a_scale"].float()[:, None] * _f32(o["alpha"])
    assert torch.equal((acc * scale + ev).double(), pre), "reduce-kernel association is not exact on these operands"
    assert torch.isfinite(pre).all()


@functools.lru_cache(maxsize=None)
def dense_operands(bm, variant, geglu=False, splits=1):
    """Operands of one exact-pre fp16 launch (CPU tensors; read-only, shared): A one-hot [M, K], W [N, K] (interleaved for GEGLU), bias,
    rowvec, resid [M, N], the scalars, Wv = the values W holds (fp64-exact) and pre [M, N] in fp64."""
    K = 128 if splits == 1 else 256 * splits
    F_ = 328
    N = 2 * F_ if geglu else F_
    M = max(bm, K) + 24
    tab = table16()
    sweep = _sweep(tab, F_, K, shift=0 if variant == "bias" else 17)
    if variant != "bias":
        sweep = _quantise(sweep)
    if geglu:
        from pbe_amd import ops
        val = torch.tensor(VALUE_SET)[(torch.arange(F_)[:, None] + torch.arange(K)[None, :]) % 5].half()
        W, _ = ops.pack_geglu(torch.cat([val, sweep]).float(), torch.zeros(N))
    else:
        W = sweep.contiguous()
    A = torch.zeros(M, K, dtype=torch.float16)
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    bias, per_row, rv, grp, alpha = _addends(variant, M, N, bm)
    g = torch.Generator().manual_seed(1000 * bm + N + K)
    resid = (torch.randn(M, N, generator=g) * 2).half()
    o = dict(M=M, N=N, K=K, A=A, W=W, Wv=W, bias=bias, bias_per_row=per_row, rowvec=rv, group_rows=grp, alpha=alpha, resid=resid)
    o["pre"] = _pre64(o)
    return o


@functools.lru_cache(maxsize=None)
def f8_operands(bm, geglu=False):
    """Operands of one exact-pre ops.gemm_f8 launch: a8 one-hot 1.0, w8 sweeping every finite e4m3 code, a_scale 2^-1 .. 2^-6 by row,
    w_scale 1, an exact bias; Wv = the dequantised w8."""
    K, F_ = 128, 328
    N = 2 * F_ if geglu else F_
    M = max(bm, K) + 24
    sweep = _sweep(table8(), F_, K)
    if geglu:
        val = torch.tensor(VALUE_SET).to(torch.float8_e4m3fn).view(torch.uint8)[(torch.arange(F_)[:, None] + torch.arange(K)[None, :]) % 5]
        w8 = torch.stack([val, sweep], 1).reshape(N, K).contiguous()
    else:
        w8 = sweep.contiguous()
    a8 = torch.zeros(M, K, dtype=torch.uint8)
    a8[torch.arange(M), torch.arange(M) % K] = 0x38                        # e4m3 1.0
    a_scale = (2.0 ** -(1 + torch.arange(M) % 6).float()).contiguous()
    bias = torch.tensor(BIAS_SET, dtype=torch.float32)[torch.arange(N) % 5].contiguous()
    g = torch.Generator().manual_seed(8000 + bm + N)
    resid = (torch.randn(M, N, generator=g) * 2).half()
    o = dict(M=M, N=N, K=K, a8=a8, w8=w8, a_scale=a_scale, w_scale=torch.ones(N), Wv=w8.view(torch.float8_e4m3fn).float(), bias=bias,
             bias_per_row=False, rowvec=None, group_rows=0, alpha=1.0, resid=resid)
    o["pre"] = _pre64(o)
    return o


def all_operand_sets():
    """(label, operands) of every exact-pre case both test files use."""
    out = []
    for bm in (64, 128, 256):
        for gg in (False, True):
            out += [(f"dense bm{bm} {v}{' geglu' if gg else ''}", dense_operands(bm, v, gg)) for v in variants_of(4 if gg else 1)]
    for bm, splits in ((128, 2), (256, 3)):
        for gg in (False, True):
            out += [(f"split{splits} bm{bm} {v}{' geglu' if gg else ''}", dense_operands(bm, v, gg, splits)) for v in variants_of(4 if gg else 1, splits)]
    for bm in (64, 128):
        out += [(f"f8 bm{bm}{' geglu' if gg else ''}", f8_operands(bm, gg)) for gg in (False, True)]
    return out


# ---- launches (GPU) ----------------------------------------------------------------------------------------------------------------
class forced_tile:
    """ops.tune(1, cfg | splits << 8) with ops._PLANS recording; on exit the knob is reset.  .check() asserts that every launch since the
    last check took the forced tile and split factor."""

    def __init__(self, cfg, splits=1):
        self.cfg, self.splits = cfg, splits

    def __enter__(self):
        from pbe_amd import ops
        ops.tune(1, self.cfg | (self.splits << 8))
        ops._PLANS = []
        return self

    def check(self, what=""):
        from pbe_amd import ops
        plans, ops._PLANS = ops._PLANS, []
        assert plans, f"{what}: no launch was recorded"
        for p in plans:
            assert (p[1], p[2]) == (self.cfg, self.splits), f"{what}: forced tile {self.cfg} split {self.splits}, the plan took {p}"
        return plans

    def __exit__(self, *exc):
        from pbe_amd import ops
        ops.tune(1, -1)
        ops._PLANS = None
        return False


def launch_dense(o, act, dev, resid=False):
    from pbe_amd import ops
    kw = dict(act=act, alpha=o["alpha"], bias_per_row=o["bias_per_row"])
    if o["rowvec"] is not None:
        kw.update(rowvec=o["rowvec"].to(dev), group_rows=o["group_rows"])
    if resid and act != 4:
        kw["resid"] = o["resid"].to(dev)
    return ops.gemm(o["A"].to(dev), o["W"].to(dev), o["bias"].to(dev), **kw)


def launch_f8(o, act, dev, resid=False):
    from pbe_amd import ops
    return ops.gemm_f8(o["a8"].to(dev), o["a_scale"].to(dev), o["w8"].to(dev), o["w_scale"].to(dev), o["bias"].to(dev),
                       resid=o["resid"].to(dev) if resid and act != 4 else None, act=act)


# ---- random-operand cases through tilecheck (LayerNorm fold + act, conv + act) ---------------------------------------------------
PRE_STD = 3.0                    # pre-activation std of the random-operand cases: |pre| reaches 10 and more


def ln_case(tile, act, M=280, N=328, K=320):
    """tilecheck.Case of LayerNorm fold + act on one extended-epilogue tile: rows m % 97 == 0 carry mean >> std."""
    import tilecheck

    class _Case(tilecheck.Case):
        def _fused(self):
            self.ln, self.offset, self.act, self.wscale = True, True, act, PRE_STD
    c = _Case(f"gx:{M}:{N}:{K}:1", tile | (1 << 8))
    return c


def ln_fold_expect(A, W, bias, colsum, act, eps=1e-5):
    """(want, bound) of gemm(ln=...) for the rows A [R, K] (fp16 values) as tilecheck.reference_gemm forms them: W = weights x gain as sent,
    bias = W beta + b, colsum of W; act 4: interleaved columns."""
    from tilecheck import ACC_C, expect
    A, W = A.double(), W.double()
    K = A.shape[1]
    mean = A.mean(1, keepdim=True)
    var = ((A - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    eps_r = ACC_C * U32 * math.sqrt(K) * (A * A).mean(1, keepdim=True) / (var + eps) + 8 * U32
    dmean = ACC_C * U32 * math.sqrt(K) * A.abs().mean(1, keepdim=True)
    return expect(A @ W.t(), A.abs() @ W.abs().t(), K, bias=bias.double(), ln=(rstd, mean, colsum.double(), eps_r, dmean), act=act)


def conv_case(tile, splits, act, shape=(8, 16, 16, 128, 160)):
    """tilecheck.Case of conv3x3(act) with row vector and residual on a forced tile."""
    import tilecheck
    B, H, W, C, Co = shape

    class _Case(tilecheck.Case):
        def _fused(self):
            self.rowvec, self.resid, self.act, self.wscale = True, True, act, PRE_STD
    return _Case(f"c:{B}:{H}:{W}:{C}:0:{Co}:1:1:0", tile | (splits << 8))
