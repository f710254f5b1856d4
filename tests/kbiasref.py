"""References for the key-bias form of the attention kernel (pbe_attention_kbias_f16, include/pbe_hip.h) and for exemplar weights on
the fused cross-attention kernel (pbe_ctx_attention_w_f16).  Helpers imported by test_ctx_weights_cpu.py, test_attention_kbias_gpu.py
and test_ctx_weights_gpu.py.  Not a conftest: plain functions only, on whatever device the operands live.

Semantics (ldm/modules/attention.py:207-230 of the reference with key j of sample b counted w[b, j] >= 0 times): the softmax weight of
key j is proportional to w[b, j] exp(s_j), i.e. bias[b, j] = log2 w[b, j] is added to the score in the kernels' log2 domain; w = 0 is
bias -inf and removes the key.

  reference   fp64 result and per-element bound, built the way accgate.attn_reference builds its own (multiply-add form: the key-bias
              form never keeps the reference maximum in the head-dim padding).  With t_j = s_j + bias_j the biased score, tmax its row
              maximum, Z = sum_j 2^(t_j - tmax), w the softmax weights over t:
                  c_j   = max(2^-11 w_j, 2^-25 / Z) / (1 - 2^-11)
                        + w_j (ln 2 (2^-22 sabs_j + 2^-23 |bias_j| + 2^-24 (|tmax| + 8)) + 2^-22)
                  bound = c @ |v| + |O| sum_j c_j + 2^-20 (w @ |v|) + (2^-11 + 2^-22) |O| + 2^-24
              The two new terms are the fp32 add of the bias: the kernel forms t_j = fma(s_j, scale log2e, bias_j) - one rounding,
              <= 2^-24 (sabs_j + |bias_j|) - and then t_j - m in a second one, <= 2^-24 (|t_j| + |m|) <= 2^-24 (sabs_j + |bias_j| +
              |tmax| + 8) since the reference m lies within ATTN_THR = 8 of tmax.  Absent keys (bias -inf) have w_j = 0 and P = 0 exactly.
  emulate     attention.hip's KB form in plain fp32 torch: accgate.attn_emulate's tile / raise structure with the bias added before the
              maximum, and the kernel's rule for a reference that is still -inf (the reference used is 0 until a live key was seen).
              Mutations the gate must reject: the bias row of sample b + 1, the bias multiplied by `scale`, one absent key given bias 0.
  fold_log2w  ctxref.Operands with log2 w added to kbias (per head), in fp64 or through fp32, and the per-sample operands with the
              absent tokens removed / the integer-weighted tokens repeated - what the unmodified ctxref.reference is run on.
"""
from __future__ import annotations

import math

import torch

import accgate as ag
import ctxref as cr
from accgate import ATTN_THR, KT, LN2

INF = math.inf


# ---- pbe_attention_kbias_f16 ----------------------------------------------------------------------------------------------------------
def kb_reference(q, k, v, bias, scale_log2e, close=None):
    """(want, bound) fp64 [B, Nq, H * D] from fp16-valued q [B, H, Nq, D], k, v [B, H, Nk, D] and bias fp32 [B, Nk] (log2 domain, -inf =
    absent; shared by the heads)."""
    B, H, Nq, D = q.shape
    want = torch.empty(B, Nq, H, D, dtype=torch.float64, device=q.device)
    bound = torch.empty_like(want)
    for b in range(B):
        bd_ = bias[b].double()[None, :]
        babs = torch.where(torch.isinf(bd_), torch.zeros_like(bd_), bd_.abs())
        for h in range(H):
            qd, kd, vd = q[b, h].double(), k[b, h].double(), v[b, h].double()
            va = vd.abs()
            t = (qd @ kd.t()) * scale_log2e + bd_
            sabs = (qd.abs() @ kd.abs().t()) * abs(scale_log2e)
            tmax = t.max(-1, keepdim=True).values
            e = torch.exp2(t - tmax)
            Z = e.sum(-1, keepdim=True)
            w = e / Z
            o = w @ vd
            arg = 2.0 ** -22 * sabs + 2.0 ** -23 * babs + 2.0 ** -24 * (tmax.abs() + ATTN_THR)
            c = torch.maximum(w * 2.0 ** -11, 2.0 ** -25 / Z) / (1 - 2.0 ** -11) + w * (LN2 * arg + 2.0 ** -22)
            bd = c @ va + o.abs() * c.sum(-1, keepdim=True) + 2.0 ** -20 * (w @ va) + (2.0 ** -11 + 2.0 ** -22) * o.abs() + 2.0 ** -24
            want[b, :, h], bound[b, :, h] = o, bd
    want, bound = want.reshape(B, Nq, H * D), bound.reshape(B, Nq, H * D)
    return want, ag.clamp_to_close(want, bound, close or ag.CLOSE["attention"])


def kb_emulate(q, k, v, bias, scale_log2e, *, ones, roll_bias=False, bias_times=None, absent_as_zero=False, stats=None):
    """The KB form of attn_kernel restated in fp32 (module docstring); returns fp16 [B, Nq, H * D].  Mutations: roll_bias - sample b takes
    the bias row of sample b + 1; bias_times = c - the bias is multiplied by c (the softmax scale: a bias added before the scaling);
    absent_as_zero - the first absent key of every sample gets bias 0.  stats: dict that receives the raises seen after the first one
    and whether some query sat at a still-unset reference while a tile was processed."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    sl = float(torch.tensor(scale_log2e, dtype=torch.float32))
    bias = bias.float()
    if roll_bias:
        bias = bias.roll(-1, 0)
    if bias_times is not None:
        bias = bias * float(bias_times)
    if absent_as_zero:
        bias = bias.clone()
        for b in range(B):
            gone = torch.nonzero(torch.isinf(bias[b])).flatten()
            if gone.numel():
                bias[b, gone[0]] = 0.0
    qf, kf, vf = q.float(), k.float(), v.float()
    pad = (-Nq) % 32
    if pad:
        qf = torch.cat([qf, qf.new_zeros(B, H, pad, D)], 2)
    NQ = Nq + pad
    o = qf.new_zeros(B, H, NQ, D)
    l = qf.new_zeros(B, H, NQ, 1)
    m = qf.new_full((B, H, NQ, 1), -INF)
    nt = (Nk + KT - 1) // KT
    raises, unset_tiles = 0, 0

    def group_any(x):                                # the ballot: one decision per 32-query group
        return x.view(B, H, NQ // 32, 32, 1).any(3, keepdim=True).expand(B, H, NQ // 32, 32, 1).reshape(B, H, NQ, 1)
    for t in range(nt):
        kt, vt = kf[:, :, t * KT:(t + 1) * KT], vf[:, :, t * KT:(t + 1) * KT]
        s = (qf @ kt.transpose(-1, -2)) * sl + bias[:, None, None, t * KT:(t + 1) * KT]
        mx = s.max(-1, keepdim=True).values
        hit = group_any(mx - m > ATTN_THR)           # NaN (-inf - -inf) compares false: no raise
        had = torch.isfinite(m)
        m_new = torch.where(hit, torch.maximum(m, mx), m)
        alpha = torch.where(hit, torch.exp2(m - m_new), torch.ones_like(m))
        alpha = torch.where(torch.isnan(alpha), torch.zeros_like(alpha), alpha)       # a raise from -inf to -inf: O = l = 0 either way
        m = m_new
        l, o = l * alpha, o * alpha
        mref = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp2(s - mref)
        if bool((hit & had)[:, :, :Nq].any()):
            raises += 1
        if bool(torch.isinf(m)[:, :, :Nq].any()):
            unset_tiles += 1
        p16 = p.half().float()
        l = l + (p16 if ones else p).sum(-1, keepdim=True)
        o = o + p16 @ vt
    if stats is not None:
        stats.update(raises=raises, unset_tiles=unset_tiles, tiles=nt)
    out = (o * (1.0 / l))[:, :, :Nq].half()
    return out.permute(0, 2, 1, 3).reshape(B, Nq, H * D)


def kb_ones(D):
    """The denominator comes from the ones row of V^T (DV > DP) in the instantiation the key-bias dispatch takes for head dim D."""
    dp = 16 if D <= 16 else 32 if D <= 32 else 48 if D <= 48 else 64 if D <= 64 else 80 if D <= 80 else 128 if D <= 128 else 160
    return (dp + 31) // 32 * 32 > dp


def kb_verdict(got, want, bound, emu):
    """(accepted, text): every element of `got` (fp16 [B, Nq, H D]) finite and within `bound` of the fp64 `want`, and its rel-L2 at most
    REL_L2_FACTOR x that of `emu` = kb_emulate of the same operands."""
    rep = ag.compare(ag.flat(got), ag.flat(want), ag.flat(bound))
    r_got, r_emu = ag.rel_l2(got, want), ag.rel_l2(emu, want)
    text = f"{rep}; rel-L2 {r_got:.3e} (emulation {r_emu:.3e}, limit x{ag.REL_L2_FACTOR})"
    return rep.ratio <= 1.0 and r_got <= ag.REL_L2_FACTOR * r_emu, text


# bias patterns at Nk = 130 (two full tiles and a 2-key ragged one); every sample gets a different row
PATTERNS = ("random", "first_tile_absent", "middle_tile_absent", "ragged_tile_absent", "one_live_key")


def kb_bias(pattern, B, Nk, seed):
    """fp32 [B, Nk]: live keys carry a bias drawn uniformly from +-9 log2 units (another draw per sample), the pattern's keys are -inf;
    one_live_key: bias 0 on one key of the LAST tile (key Nk - 1 - (b % 2) of sample b), -inf elsewhere."""
    g = torch.Generator().manual_seed(seed)
    bias = (torch.rand(B, Nk, generator=g) * 18.0 - 9.0).float()
    nt = (Nk + KT - 1) // KT
    if pattern == "first_tile_absent":
        bias[:, :KT] = -INF
    elif pattern == "middle_tile_absent":
        assert nt >= 3
        bias[:, KT:2 * KT] = -INF
    elif pattern == "ragged_tile_absent":
        assert nt >= 2
        bias[:, (nt - 1) * KT:] = -INF
    elif pattern == "one_live_key":
        bias[:] = -INF
        for b in range(B):
            bias[b, Nk - 1 - (b % 2 if Nk - (nt - 1) * KT > 1 else 0)] = 0.0
    else:
        assert pattern == "random", pattern
    return bias


def counts_bias(counts, Nk):
    """fp32 [B, Nk] of a padded ragged batch: sample b has its first counts[b] keys (bias 0), the rest absent."""
    j = torch.arange(Nk)[None, :]
    return torch.where(j < torch.tensor(list(counts))[:, None], 0.0, -INF).float()


def step_operands(B, H, Nq, Nk, D, seed):
    """Constant-score operands: q and k hold one constant each, so every raw score of a (sample, head) is equal and the bias alone decides
    where the reference is raised; v random.  The bias steps by tile, across ATTN_THR from both sides:
      sample 0: 0 | +7.5 | +16   - tile 1 stays below the threshold (deferred), tile 2 exceeds the tile-0 reference by 16 (raised);
      sample 1: 0 | +8.5 | +16   - tile 1 raises, tile 2 sits 7.5 above the new reference (deferred);
      sample 2: +16 | +8.5 | 0   - descending: nothing after the first tile raises."""
    assert B == 3 and Nk > 2 * KT
    g = torch.Generator().manual_seed(seed)
    q = torch.full((B, Nq, H * D), 0.25).half()
    k = torch.full((B, Nk, H * D), 0.5).half()
    v = torch.randn(B, Nk, H * D, generator=g).half()
    steps = torch.tensor([[0.0, 7.5, 16.0], [0.0, 8.5, 16.0], [16.0, 8.5, 0.0]])
    bias = steps.repeat_interleave(KT, 1)[:, :Nk].float().contiguous()
    return q, k, v, bias


# ---- pbe_ctx_attention_w_f16 ----------------------------------------------------------------------------------------------------------
CTX_SHAPES = [(2, 72, 64, 8, 4, 1), (2, 130, 320, 8, 5, 1), (3, 72, 320, 8, 16, 5), (2, 72, 640, 8, 3, 1)]      # (B, N, C, H, Nk, parts)
COUNTS = (1, 3, 5)


def ctx_weights(B, Nk, seed, counts=COUNTS):
    """fp64 [B, Nk]: exp2(3 randn) on the first min(counts[b], Nk) tokens of sample b, 0 on the rest."""
    g = torch.Generator().manual_seed(seed)
    w = torch.exp2(3.0 * torch.randn(B, Nk, generator=g, dtype=torch.float64))
    j = torch.arange(Nk)[None, :]
    return torch.where(j < torch.tensor([min(counts[b % len(counts)], Nk) for b in range(B)])[:, None], w, torch.zeros_like(w))


def fold_log2w(o, w, through_fp32=False):
    """ctxref.Operands of `o` with log2 w [B, Nk] added to kbias for every head: in fp64 (the algebra), or as the kernel adds it (fp32
    kbias + fp32 log2 w, in fp32)."""
    lw = torch.log2(w.double())
    if through_fp32:
        kb = (o.kbias.float().view(o.B, o.H, o.Nk) + lw.float()[:, None, :].to(o.kbias.device)).view(o.B, o.H * o.Nk)
    else:
        kb = (o.kbias.double().view(o.B, o.H, o.Nk) + lw[:, None, :].to(o.kbias.device)).view(o.B, o.H * o.Nk)
    return cr.Operands(o.x, o.kq, o.colsum, kb, o.vo, o.bias, o.stats, o.B, o.N, o.C, o.H, o.Nk)


def sample_tokens(o, b, tokens):
    """ctxref.Operands of sample b alone whose context is the listed tokens of o's (a token may be listed several times, or not at all)."""
    H, Nk, N = o.H, o.Nk, o.N
    idx = torch.tensor(list(tokens), device=o.kq.device)
    cols = (torch.arange(H, device=o.kq.device)[:, None] * Nk + idx[None, :]).reshape(-1)
    return cr.Operands(o.x[b * N:(b + 1) * N], o.kq[b:b + 1, cols], o.colsum[b:b + 1, cols], o.kbias[b:b + 1, cols], o.vo[b:b + 1][:, :, cols], o.bias,
                       o.stats[:, b * N:(b + 1) * N], 1, N, o.C, H, len(idx))
