"""Restatement of the DPM-Solver++(2M) sampler (ldm/models/diffusion/dpm_solver.py) and of its update kernel (pbe_dpmpp_update) for the
tests - plain functions, no product code.  The reference repository has no DPM solver; what pins this file to reference-pinned code is
that its first order IS the oracle's DDIM (tests/test_dpm_solver_cpu.py::test_first_order_is_the_oracle_ddim).

  dpm_sample(model, S, ...)      the sampler around a model callable, as oracle.ddim_sample is: the grid of the oracle's DDIM
                                 (ddim_timesteps_uniform / ddim_parameters / schedule_subset), coefficients in fp64 from the solver's
                                 textbook form (Lu et al. 2022, DPM-Solver++, eq. 11 and algorithm 2), tensors in `dtype`, the mask / x0
                                 blend with injected noise of the oracle samplers.
  update_reference(...)          one kernel call in fp64 from the fp16 / fp32 operands the kernel reads (coefficients through fp32,
                                 as the launch passes them), with the magnitude sums S0 / Sn of the terms entering each output.
  update_gate(...)               the per-element bound |got - ref| <= 8 * 2^-24 * S (+ the subnormal floor), the form of the
                                 element-wise edge tests (tests/test_edges_gpu.py::test_axpy_qsample_mul_planes).
  update_emulated(...)           the kernel's fp32 arithmetic on the CPU, fused multiply-adds included (an fp64 product of two fp32
                                 values is exact), optionally with one of two planted faults - what shows that the gate rejects them.

The bound.  u = 2^-24.  The kernel rounds 2 times for e (the difference, the fma), 2 more for x0 (the fma, the product with 1/alpha), and
3 more for x_next (kx x, the fma with k0, the fma with k1).  A rounding's error is at most u times its result, and every result is at most
the sum of the magnitudes of the terms it was formed from; carried to the outputs, each error is at most u times
    S0 = (|x| + |sigma| Se) |1/alpha|,      Se = |e_u| + |cfg| (|e_c| + |e_u|)   (dup 1: Se = |e|)
    Sn = |kx x| + |k0| S0 + |k1 x0_prev|
so |d x0| <= 4 u S0, and |d x_next| <= 6 u Sn (kx x meets 3 of the roundings, k0 x0 the 4 of x0 and 2 more, k1 x0_prev one) to first
order in u.  The gate is 8 u S, the edge tests' form; without the fusing the bounds would be 6 and 9.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle_loader import O

U32 = 2.0 ** -24
FLOOR = 1e-38


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
def _lam(a):
    return 0.5 * (math.log(a) - math.log1p(-a))              # ln(alpha / sigma) of a cumulative alpha


def step_scalars(a, a_prev, a_before, order):
    """One step from cumulative alpha a to a_prev; a_before = the cumulative alpha the PREVIOUS step started from (None: no history, or
    a step that is to be first order).  -> (sigma, alpha, ratio, gain, w) with x' = ratio x + gain [(1 + w) x0 - w x0_previous]."""
    a, a_prev = float(a), float(a_prev)
    h = _lam(a_prev) - _lam(a)
    if not h > 0:
        raise ValueError(f"dpmref: h = {h} <= 0")
    w = 0.0
    if order == 2 and a_before is not None:
        w = 0.5 * h / (_lam(a) - _lam(float(a_before)))      # 1 / (2 r), r = h_previous / h
    return math.sqrt(1.0 - a), math.sqrt(a), math.sqrt(1.0 - a_prev) / math.sqrt(1.0 - a), -math.sqrt(a_prev) * math.expm1(-h), w


def dpm_sample(model, S, x_T, cond, uc, scale, z_inpaint, mask, alphas_cumprod, order=2, timesteps=None, blend=None, dtype=torch.float32):
    """(x_0 latent, info): info['calls'], info['pred_x0'] (every step's data prediction).  The arguments of oracle.ddim_sample; blend =
    (mask, x0, [noise per step]): x = q_sample(x0, step) * mask + (1 - mask) * x before every step."""
    ddim_t = O.ddim_timesteps_uniform(S, alphas_cumprod.shape[0])
    _, a, a_prev = O.ddim_parameters(alphas_cumprod, ddim_t)
    time_range = np.flip(O.schedule_subset(ddim_t, timesteps))
    n = time_range.shape[0]
    b = x_T.shape[0]
    x = x_T.float().to(dtype)
    guided = not (uc is None or scale == 1.0)
    if guided and uc.shape[0] != cond.shape[0]:
        uc = uc.expand(cond.shape[0], *uc.shape[1:])
    calls, preds, x0_before = 0, [], None
    for i, step in enumerate(time_range):
        idx = n - i - 1
        if blend is not None:
            bm, bx0, bnoise = blend
            x = (O.q_sample(bx0, step, bnoise[i], alphas_cumprod) * bm + (1.0 - bm) * x).to(dtype)
        tt = torch.full((b,), int(step), dtype=torch.int64)
        x9 = torch.cat((x.to(z_inpaint.dtype), z_inpaint, mask), dim=1)
        if guided:
            e_u, e_c = model(torch.cat([x9] * 2), torch.cat([tt] * 2), torch.cat((uc, cond))).chunk(2)
            e = e_u.to(dtype) + scale * (e_c.to(dtype) - e_u.to(dtype))
        else:
            e = model(x9, tt, cond).to(dtype)
        calls += 1
        second = order == 2 and 0 < i < n - 1                 # the first step has no history, the last is first order by choice
        sigma, alpha, ratio, gain, w = step_scalars(a[idx], a_prev[idx], a[idx + 1] if second else None, order)
        x0 = (x - sigma * e) / alpha
        d = (1.0 + w) * x0 - w * x0_before if second else x0
        x = ratio * x + gain * d
        x0_before = x0
        preds.append(x0)
    return x, {"calls": calls, "pred_x0": preds}


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


def _halves(eps, dup):
    """eps [dup*B, HW, >= 4] (fp16 values) -> (e_u, e_c) as fp64 [B, 4, HW]; dup 1: (e, None)."""
    e = eps[..., :4].double().transpose(1, 2)
    if dup == 1:
        return e, None
    B = e.shape[0] // 2
    return e[:B], e[B:]


def update_reference(eps, dup, cfg, x, x0_prev, coef5):
    """fp64 (x0, x_next, S0, Sn) of one pbe_dpmpp_update call: eps fp16 [dup*B, HW, >= 4], x / x0_prev fp32 [B, 4, HW]."""
    sigma, ia, kx, k0, k1 = (_f32(c) for c in coef5)
    cfg = _f32(cfg)
    eu, ec = _halves(eps, dup)
    xd = x.double()
    if dup == 2:
        e, se = eu + cfg * (ec - eu), eu.abs() + abs(cfg) * (ec.abs() + eu.abs())
    else:
        e, se = eu, eu.abs()
    x0 = (xd - sigma * e) * ia
    s0 = (xd.abs() + abs(sigma) * se) * abs(ia)
    xn = kx * xd + k0 * x0
    sn = (kx * xd).abs() + abs(k0) * s0
    if x0_prev is not None:
        xn = xn + k1 * x0_prev.double()
        sn = sn + (k1 * x0_prev.double()).abs()
    return x0, xn, s0, sn


def update_gate(got_x0, got_xn, ref, what=""):
    """ref = update_reference(...).  got_x0 may be None (the launch without x0_out).  -> the worst error of each output in units of
    u * S (x0, x_next); raises AssertionError past 8."""
    x0, xn, s0, sn = ref
    worst = []
    for name, got, want, s in (("x0", got_x0, x0, s0), ("x_next", got_xn, xn, sn)):
        if got is None:
            worst.append(0.0)
            continue
        got = got.detach().cpu().double().reshape(want.shape)
        assert torch.isfinite(got).all(), f"{what}: non-finite {name}"
        err = (got - want).abs()
        over = err > 8 * U32 * s + FLOOR
        worst.append(float((err / (U32 * s + FLOOR)).max()))
        assert not over.any(), (f"{what}: {name} misses 8 * 2^-24 * S at {int(over.sum())} of {over.numel()} elements, worst "
                                f"{worst[-1]:.1f} u S, first at {tuple(torch.nonzero(over)[0].tolist())}")
    return tuple(worst)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()     # the product of two fp32 values is exact in fp64: one rounding to fp64, one to fp32


def update_emulated(eps, dup, cfg, x, x0_prev, coef5, fault=None):
    """The kernel's fp32 arithmetic on the CPU -> (x0, x_next) fp32 [B, 4, HW].  fault: None, "swap_halves" (the conditional half read
    where the unconditional belongs and the other way round) or "k1_on_x0" (the second-order term fed this step's x0)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)       # noqa: E731
    sigma, ia, kx, k0, k1 = (f(c) for c in coef5)
    eu, ec = _halves(eps, dup)
    eu = eu.float()
    if dup == 2:
        ec = ec.float()
        if fault == "swap_halves":
            eu, ec = ec, eu
        e = _fma(f(cfg), ec - eu, eu)
    else:
        e = eu
    x0 = _fma(-sigma, e, x) * ia
    xn = _fma(k0, x0, kx * x)
    if x0_prev is not None:
        xn = _fma(k1, x0 if fault == "k1_on_x0" else x0_prev, xn)
    return x0, xn


def plms_form_emulated(eps, dup, cfg, x, coef8):
    """pbe_plms_update without history (one weight of 1) in correctly rounded fp32 on the CPU -> (pred_x0, x_prev): the DDIM form
    sqrt(a') x0 + sqrt(1 - a') e that the first-order DPM form is compared with.  coef8 as ops.plms_update takes it."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)       # noqa: E731
    eu, ec = _halves(eps, dup)
    eu = eu.float()
    e = eu if dup == 1 else _fma(f(cfg), ec.float() - eu, eu)
    x0 = _fma(-f(coef8[4]), e, x) * f(coef8[5])
    return x0, _fma(f(coef8[6]), x0, f(coef8[7]) * e)
