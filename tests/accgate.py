"""Per-element accuracy gate for the kernels that run by default next to the tuned tiles: pbe_attention_f16, pbe_groupnorm_f16 /
pbe_groupnorm_apply_f16, pbe_layernorm_f16, pbe_softmax_rows_f16, pbe_geglu_f16, pbe_timestep_embedding_f16.  Helpers imported by
test_accgate_cpu.py and test_accuracy_gpu.py.  Not a conftest: plain functions only, on whatever device the operands live.

For every op: an fp64 reference from the fp16 operands that were sent, a bound per output element from the number formats (fp16: 11
significant bits, fp32: 24) and the kernel text, a plain-torch fp32 restatement of the kernel's arithmetic (the "emulation": what a
correct kernel is expected to do, never a kernel's own output), and the mutations the gate must reject.  Every constant is
tilecheck's (U32, U16, ACC_C, GELU_FIT) or is derived below; none is fitted to a run.

fp16 attention (pbe_amd/csrc/attention.hip), log2 domain: s_j the scores, sabs_j = scale log2e sum_d |q_d k_jd|, w the softmax weights,
Z = sum_j 2^(s_j - smax) (the kernel's reference m never exceeds smax by more than its own rounding, hence sum P >= Z (1 - 2^-11)):
    c_j   = max(2^-11 w_j, 2^-25 / Z) / (1 - 2^-11)                       P rounded to fp16 once (P <= 2^8: ATTN_THR)
          + w_j (ln 2 (2^-22 sabs_j [+ 2^-11 sabs_j] [+ 2^-22 |smax|]) + 2^-22)
    bound = c @ |v| + |O| sum_j c_j + 2^-20 (w @ |v|) + (2^-11 + 2^-22) |O| + 2^-24
[+ 2^-11 sabs_j]: the d = 40 form without q_prescaled rounds q scale log2e to fp16 (attention.hip, "scale log2e folded into Q");
[+ 2^-22 |smax|]: the d = 40 form carries the reference through the MFMA as (-m / 64) * 64 (attention.hip, MPAD).
The worst-case bound assumes every rounding aligns, so the gate also compares rel-L2: kernel <= 1.5 x emulation (REL_L2_FACTOR).

GroupNorm / LayerNorm (norm.hip), n = longest fp32 summation chain of one statistic:
    d_mean = ACC_C U32 sqrt(n) E|x|      eps_r = ACC_C U32 sqrt(n) E[x^2] / (var + eps) + 8 U32
    |d pre| <= |gamma| rstd (|x - mean| eps_r + d_mean) + A
    GroupNorm  A = 3 U32 (|x sc| + |mean sc| + |beta|)   (gn_apply_kernel: sc = rstd gamma, sh = beta - mean sc, x sc + sh in fp32)
    LayerNorm  A = 4 U32 (|pre| + |beta|)                (layernorm_kernel: ((x - mean) rstd gamma + beta), two-pass statistics, n = C)
    SiLU       1.1 |d pre| + 4 U32 |y|                   (v_rcp_f32 and v_exp_f32 at 1 ulp each; |silu'| <= 1.1)
    store      U16 |y| + 2^-25
n of the GroupNorm paths: gn_stats_kernel sums in fp32 inside one block only (rows_per_block rows x C / groups channels; the blocks'
partials meet in fp64 in gn_apply_kernel), gn_small_kernel inside one wave (a quarter of the HW x C / groups slice), a conv's
group_stats partials inside one conv tile (HW / blocks rows x C / groups).

softmax rows: U16 w + 2^-25 + w (ln 2 U32 (2 |x| + |x - xmax|) scale log2e + ACC_C U32 sqrt(cols)); the |x - xmax| term is the rounding
of the subtraction x scale log2e - mx (softmax_rows_kernel), which the row maximum's own product shares.
GEGLU: tilecheck's term with exact operands: GELU_FIT |a| + 4 U32 |y|, then the store.
timestep embedding: fp64 formula of ldm/modules/diffusionmodules/util.py; the kernel's angle t f_k carries U32 |t f_k| from its own
rounding, and f_k = expf(c k) in fp32 carries (4 + 4 |c k|) U32 relative (temb_kernel: expf within 2 ulp = 4 U32; c = -logf(period) /
half is a 1-ulp logf and a division, 3 U32, and the product c k one more), cosf / sinf within 2 ulp = 4 U32 absolute.
"""
from __future__ import annotations

import math

import torch

from tilecheck import ACC_C, GELU_FIT, U16, U32, Report, check, clamp_to_close, compare  # noqa: F401  (re-exported)

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
KT = 64                      # keys per staged tile (AttnTile::KT)
ATTN_THR = 8.0
REL_L2_FACTOR = 1.5
# _close limits (rtol, atol) of the existing test of each op (tests/test_ops_gpu.py)
# ("attention_loose": test_attention_deferred_max_paths' limit for large_logits in the d = 40 form, whose extra fp16 rounding of q is worth
#  2^-11 of +-400 log2 units; the per-element model carries that as its own term, the clamp merely must not cut below what it allows)
CLOSE = {"attention": (4e-3, 2e-3), "attention_loose": (1.2e-2, 2e-3), "norm": (3e-3, 1e-3), "softmax": (3e-3, 1e-6), "geglu": (2e-3, 1e-3), "temb": (1e-3, 2e-3)}


def close_verdict(got, ref, close):
    """(accepted, max|d|, limit) of the whole-tensor _close test of tests/test_ops_gpu.py."""
    rtol, atol = close
    err = (got.double() - ref.double()).abs().max().item()
    lim = rtol * ref.double().abs().max().item() + atol
    return err <= lim, err, lim


def rel_l2(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


def flat(t):
    return t.reshape(-1, t.shape[-1])


# ---- attention: dispatch rule ------------------------------------------------------------------------------------------------------
INSTANTIATIONS = ("16,1", "32,1", "48,1,1,true", "48,2,1,true", "48,2,2,true", "48,1", "48,2", "48,2,2", "64,1", "64,2", "80,1", "80,2",
                  "128,1", "160,1")


def instantiation(B, H, Nq, Nk, D, qw=0, mpad=1):
    """attn_kernel<...> template arguments the dispatch at the end of attention.hip picks (pbe_tune key 3 = qw, key 6 = mpad)."""
    two = (qw == 2) if qw else (((Nq + 255) // 256) * B * H >= 512 and D <= 80)
    if D <= 16:
        return "16,1"
    if D <= 32:
        return "32,1"
    if D == 40 and mpad:
        if qw == 2:
            return "48,2,1,true"
        if qw == 1 or not two:
            return "48,1,1,true"
        return "48,2,2,true"
    if D <= 48:
        return "48,2,2" if qw == 3 else ("48,2" if two else "48,1")
    if D <= 64:
        return "64,2" if two else "64,1"
    if D <= 80:
        return "80,2" if two else "80,1"
    return "128,1" if D <= 128 else "160,1"


def form_of(inst):
    """(DP, mpad, ones): tile head dim, reference-in-the-padding form, denominator from the ones row of V^T (DV > DP)."""
    f = inst.split(",")
    dp = int(f[0])
    return dp, f[-1] == "true", (dp + 31) // 32 * 32 > dp


# ---- attention: fp64 reference and bound -------------------------------------------------------------------------------------------
def heads(t, B, N, H, D):
    """[B, N, H * D] (or [B * N, H * D]) -> [B, H, N, D] view."""
    return t.reshape(B, N, H, D).permute(0, 2, 1, 3)


def attn_reference(q, k, v, scale_log2e, *, mpad, q_prescaled, chunk=2048, close=None):
    """(want, bound), fp64 [B, Nq, H * D], of softmax(q k^T) v in base 2 from fp16-valued q [B, H, Nq, D], k, v [B, H, Nk, D]: one (b, h)
    and `chunk` queries at a time.  The bound is the module docstring's, clamped to the _close limit of the existing test of the case."""
    B, H, Nq, D = q.shape
    want = torch.empty(B, Nq, H, D, dtype=torch.float64, device=q.device)
    bound = torch.empty_like(want)
    for b in range(B):
        for h in range(H):
            kd, vd = k[b, h].double(), v[b, h].double()
            ka, va = kd.abs().t().contiguous(), vd.abs()
            for r0 in range(0, Nq, chunk):
                qd = q[b, h, r0:r0 + chunk].double()
                s = (qd @ kd.t()) * scale_log2e
                sabs = (qd.abs() @ ka) * abs(scale_log2e)
                smax = s.max(-1, keepdim=True).values
                e = torch.exp2(s - smax)
                Z = e.sum(-1, keepdim=True)
                w = e / Z
                o = w @ vd
                arg = 2.0 ** -22 * sabs
                if mpad and not q_prescaled:
                    arg = arg + 2.0 ** -11 * sabs
                if mpad:
                    arg = arg + 2.0 ** -22 * smax.abs()
                c = torch.maximum(w * 2.0 ** -11, 2.0 ** -25 / Z) / (1 - 2.0 ** -11) + w * (LN2 * arg + 2.0 ** -22)
                bd = c @ va + o.abs() * c.sum(-1, keepdim=True) + 2.0 ** -20 * (w @ va) + (2.0 ** -11 + 2.0 ** -22) * o.abs() + 2.0 ** -24
                want[b, r0:r0 + chunk, h], bound[b, r0:r0 + chunk, h] = o, bd
    want, bound = want.reshape(B, Nq, H * D), bound.reshape(B, Nq, H * D)
    return want, clamp_to_close(want, bound, close or CLOSE["attention"])


# ---- attention: the kernel's arithmetic in plain fp32 torch ------------------------------------------------------------------------
def _f16(x):
    return x.half().float()


def attn_emulate(q, k, v, scale_log2e, *, mpad, q_prescaled, ones, reverse=False, den_skip_tile=None, stats=None):
    """attention.hip restated: 64-key tiles, a reference maximum per query that is raised - for a whole 32-query group at once - only when
    some query of the group outgrew it by 2^8, P rounded to fp16, fp32 sums, o * (1 / l), fp16 store.  q [B, H, Nq, D], k, v [B, H, Nk, D],
    fp16-valued; returns fp16 [B, Nq, H * D].  reverse: the keys of every tile in the opposite order (another valid summation order).
    den_skip_tile: mutation - that tile's P never reaches the denominator.  stats: dict that receives the raises seen after tile 0."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    sl = float(torch.tensor(scale_log2e, dtype=torch.float32))
    qf, kf, vf = q.float(), k.float(), v.float()
    if mpad and not q_prescaled:
        qf = _f16(qf * sl)
    pad = (-Nq) % 32
    if pad:
        qf = torch.cat([qf, qf.new_zeros(B, H, pad, D)], 2)
    NQ = Nq + pad
    o = qf.new_zeros(B, H, NQ, D)
    l = qf.new_zeros(B, H, NQ, 1)
    m = qf.new_zeros(B, H, NQ, 1) if mpad else qf.new_full((B, H, NQ, 1), -math.inf)
    raises, last_raise = 0, False
    nt = (Nk + KT - 1) // KT

    def group_any(x):                                # the ballot: one decision per 32-query group
        return x.view(B, H, NQ // 32, 32, 1).any(3, keepdim=True).expand(B, H, NQ // 32, 32, 1).reshape(B, H, NQ, 1)
    for t in range(nt):
        kt, vt = kf[:, :, t * KT:(t + 1) * KT], vf[:, :, t * KT:(t + 1) * KT]
        if reverse:
            kt, vt = kt.flip(2), vt.flip(2)
        raw = qf @ kt.transpose(-1, -2)
        if mpad:
            s = raw - m                              # the MFMA returns q.k + 64 * (-m / 64)
            mx = s.max(-1, keepdim=True).values
            hit = group_any(mx > ATTN_THR) if t else torch.ones_like(mx, dtype=torch.bool)
            tgt = m + (mx if t == 0 else mx.clamp_min(0.0))
            mref = 64.0 * _f16(tgt.clamp(-4.0e6, 4.0e6) * 0.015625)
            d = torch.where(hit, mref - m, torch.zeros_like(m))
            m = m + d
            if t:
                alpha = torch.exp2(-d)
                l, o = l * alpha, o * alpha
            p = torch.exp2(s - d)
        else:
            ms = raw.max(-1, keepdim=True).values * sl
            hit = group_any(ms - m > ATTN_THR)
            m_new = torch.where(hit, torch.maximum(m, ms), m)
            alpha = torch.exp2(m - m_new)
            alpha = torch.where(torch.isnan(alpha), torch.zeros_like(alpha), alpha)
            m = m_new
            l, o = l * alpha, o * alpha
            p = torch.exp2(raw * sl - m)
        if t and bool(hit[:, :, :Nq].any()):
            raises += 1
            last_raise = last_raise or t == nt - 1
        p16 = _f16(p)
        if den_skip_tile != t:
            l = l + (p16 if ones else p).sum(-1, keepdim=True)
        o = o + p16 @ vt
    if stats is not None:
        stats.update(raises=raises, raise_in_last_tile=last_raise, tiles=nt, ragged=Nk % KT != 0)
    out = (o * (1.0 / l))[:, :, :Nq].half()
    return out.permute(0, 2, 1, 3).reshape(B, Nq, H * D)


def attn_operands(B, H, Nq, Nk, D, seed, recipe="randn", device="cpu"):
    """(q, k, v) fp16 [B, N, H * D] drawn on `device`: test_attention's recipe (plain normal operands), or a named forced-branch recipe of
    test_attention_deferred_max_paths (B = 1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randn(B, Nq, H * D, generator=g, device=device)
    k = torch.randn(B, Nk, H * D, generator=g, device=device)
    v = torch.randn(B, Nk, H * D, generator=g, device=device)
    q4, k4 = q.view(B, Nq, H, D), k.view(B, Nk, H, D)
    if recipe == "first_tile_peak":
        k4[0, 5] = q4[0, 40] * 3.0
        k4[0, 9] = q4[0, 200] * 3.0
    elif recipe == "negative_start_then_jump":
        k4[0, :64] = -2.5 * torch.sign(q4[0, 100:101]) * torch.ones(64, H, D, device=device)
        k4[0, 300] = q4[0, 100] * 4.0
    elif recipe == "large_logits":
        q4 *= 7.0
        k4 *= 7.0
    elif recipe == "band_below_threshold":
        for t in range(1, 6):
            k4[0, 64 * t + 3] = q4[0, 7] * (0.25 * t)
    elif recipe == "ragged_jump_in_last_tile":
        k4[0, 325] = q4[0, 33] * 4.0
    else:
        assert recipe == "randn", recipe
    return q.half(), k.half(), v.half()


FORCED = ("first_tile_peak", "negative_start_then_jump", "large_logits", "band_below_threshold", "ragged_jump_in_last_tile")


# ---- attention: exact-integer operands ----------------------------------------------------------------------------------------------
def pin_operands(B, H, Nq, Nk, D, variant, seed):
    """Operands on which every score, every P = 2^(s - m), every fp32 partial sum and the d = 40 form's -m / 64 are exact (call with
    q_prescaled: scale log2e = 1).  q: one nonzero entry per (query, head) at a seeded channel - of the lower half of the head for even
    32-query groups, of the upper half for odd ones; k in {0, +-1, +-2}; v integers in [-4, 4] x 2^e, e in {-1, 0} per (channel, 32-key
    block).
      variant 1  q = 2^a, a in {0, 1}; key 0 = 2 on every channel: every query's maximum sits in tile 0 and no reference is raised later.
      variant 2  q = 1; tile 0 holds only {-1, -2} with key 0 = -1 (first reference -1); key `Nk // 2` rounded down to a tile start + 5 is
                 9 on the lower half-channels and the LAST key is 9 on the upper ones, 0 elsewhere: the even groups rescale by
                 alpha = 2^-10 in a middle tile, the odd groups in the (ragged) last tile; P stays within [2^-11, 2^3].
    Returns q [B, Nq, H * D], k [B, Nk, H * D], v [B, Nk, H * D] as fp16."""
    assert variant in (1, 2) and D % 8 == 0 and (variant == 1 or Nk > 2 * KT)
    g = torch.Generator().manual_seed(seed)
    half = D // 2
    grp = (torch.arange(Nq) // 32) % 2                                       # 0: lower half-channels, 1: upper
    ch = torch.randint(0, 1 << 30, (B, Nq, H), generator=g)
    ch = torch.where(grp[None, :, None] == 0, ch % half, half + ch % (D - half))
    a = torch.randint(0, 2, (B, Nq, H), generator=g).float() if variant == 1 else torch.zeros(B, Nq, H)
    q = torch.zeros(B, Nq, H, D).scatter_(3, ch[..., None], (2.0 ** a)[..., None])
    k = torch.randint(-2, 3, (B, Nk, H, D), generator=g).float()
    if variant == 1:
        k[:, 0] = 2.0
    else:
        k[:, :KT] = torch.randint(-2, 0, (B, min(KT, Nk), H, D), generator=g).float()
        k[:, 0] = -1.0
        mid = (Nk // 2) // KT * KT + 5
        k[:, mid] = 0.0
        k[:, mid, :, :half] = 9.0
        k[:, Nk - 1] = 0.0
        k[:, Nk - 1, :, half:] = 9.0
    nb = (Nk + 31) // 32
    e = torch.randint(-1, 1, (B, nb, H, D), generator=g).float().repeat_interleave(32, 1)[:, :Nk]
    v = torch.randint(-4, 5, (B, Nk, H, D), generator=g).float() * 2.0 ** e
    return q.reshape(B, Nq, H * D).half(), k.reshape(B, Nk, H * D).half(), v.reshape(B, Nk, H * D).half()


def pin_reference(q, k, v, B, H, Nq, Nk, D):
    """fp64 result [B, Nq, H * D] of the exact-integer operands, the bound 0.5 ulp16 (1 + 2^-8) + 2^-24 (the final o * (1 / l) is two fp32
    roundings), and the fp32 evaluation of numerator and denominator in two orders (forward and reversed key order) for the
    exactness proof: (want, bound, num64, den64, [(num32, den32), (num32, den32)])."""
    q4, k4, v4 = (heads(t, B, n, H, D).double() for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    s = q4 @ k4.transpose(-1, -2)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    num, den = p @ v4, p.sum(-1, keepdim=True)
    want = (num / den).permute(0, 2, 1, 3).reshape(B, Nq, H * D)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14)))) * 2.0 ** -10
    bound = 0.5 * ulp * (1 + 2.0 ** -8) + 2.0 ** -24
    p32, v32 = p.float(), v4.float()
    orders = [(p32 @ v32, p32.sum(-1, keepdim=True)),
              (p32.flip(-1) @ v32.flip(-2), p32.flip(-1).cumsum(-1)[..., -1:])]
    return want, bound, num, den, orders


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------
GN_MAX_CHUNKS, GN_SMALL_ROWS = 256, 12


def gn_geometry(HW, C, rows_per_thread=16):
    """(blocks, rows per block) of the two-pass GroupNorm's statistics pass (norm.hip gn_geometry; rows per thread = pbe_tune key 7)."""
    tx = min(C // 8, 256)
    rows = max(32, (256 // tx) * rows_per_thread)
    n = (HW + rows - 1) // rows
    if n > GN_MAX_CHUNKS:
        rows = (HW + GN_MAX_CHUNKS - 1) // GN_MAX_CHUNKS
        n = (HW + rows - 1) // rows
    return n, rows


def gn_small(HW, C, groups=32):
    """True when pbe_groupnorm_f16 takes the single-launch small-map kernel."""
    cg = C // groups
    return cg % 8 == 0 and cg // 8 <= 64 and HW <= GN_SMALL_ROWS * (256 // (cg // 8))


def gn_chain(HW, C, groups=32, rows_per_thread=16, conv_blocks=0):
    """n: the longest fp32 summation chain of one GroupNorm statistic on the path the launch takes."""
    cg = C // groups
    if conv_blocks:
        return (HW + conv_blocks - 1) // conv_blocks * cg
    if gn_small(HW, C, groups):
        return (HW * cg + 3) // 4
    return min(HW, gn_geometry(HW, C, rows_per_thread)[1]) * cg


def _silu64(x):
    return x / (1 + torch.exp(-x))


def gn_reference(x, gamma, beta, eps, silu, n, groups=32, close=None):
    """(want, bound) fp64 [B, HW, C] of GroupNorm(+SiLU) over NHWC x [B, HW, C] (fp16-valued), one sample at a time."""
    B, HW, C = x.shape
    cg = C // groups
    gm, bt = gamma.double().view(1, groups, cg), beta.double().view(1, groups, cg)
    want = torch.empty(B, HW, C, dtype=torch.float64, device=x.device)
    bound = torch.empty_like(want)
    rn = ACC_C * U32 * math.sqrt(n)
    for b in range(B):
        xd = x[b].double().view(HW, groups, cg)
        mean = xd.mean((0, 2), keepdim=True)
        var = ((xd - mean) ** 2).mean((0, 2), keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        d_mean = rn * xd.abs().mean((0, 2), keepdim=True)
        eps_r = rn * (xd * xd).mean((0, 2), keepdim=True) / (var + eps) + 8 * U32
        sc = rstd * gm
        pre = (xd - mean) * sc + bt
        A = 3 * U32 * ((xd * sc).abs() + (mean * sc).abs() + bt.abs())
        dpre = sc.abs() * ((xd - mean).abs() * eps_r + d_mean) + A
        if silu:
            y = _silu64(pre)
            dy = 1.1 * dpre + 4 * U32 * y.abs()
        else:
            y, dy = pre, dpre
        want[b] = y.view(HW, C)
        bound[b] = (dy * (1 + U16) + U16 * y.abs() + 2.0 ** -25).view(HW, C)
    return want, clamp_to_close(want, bound, close or CLOSE["norm"])


def gn_emulate(x, gamma, beta, eps, silu, rows_per_block, groups=32, stats_rows=None, gamma_shift_group=None):
    """The two-pass kernels in plain fp32: per-block (sum, sumsq) in fp32, the blocks' partials and mean / variance / rstd in fp64, sc / sh
    and x sc + sh in fp32, fp16 store.  Mutations: stats_rows - the statistics are those of the first stats_rows rows only;
    gamma_shift_group = g - the channels of group g + 1 take group g's gamma."""
    B, HW, C = x.shape
    cg = C // groups
    xf = x.float().view(B, HW, groups, cg)
    xs = xf if stats_rows is None else xf[:, :stats_rows]
    ta = torch.zeros(B, 1, groups, 1, dtype=torch.float64, device=x.device)
    tq = torch.zeros_like(ta)
    for r0 in range(0, xs.shape[1], rows_per_block):
        blk = xs[:, r0:r0 + rows_per_block]
        ta += blk.sum((1, 3), keepdim=True, dtype=torch.float32).double()
        tq += (blk * blk).sum((1, 3), keepdim=True, dtype=torch.float32).double()
    n = float(xs.shape[1] * cg)
    mean = ta / n
    var = (tq / n - mean * mean).clamp_min(0.0)
    mu, rstd = mean.float(), (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float()
    gm = gamma.float().view(1, 1, groups, cg)
    if gamma_shift_group is not None:
        gm = gm.clone()
        gm[:, :, gamma_shift_group + 1] = gamma.float().view(groups, cg)[gamma_shift_group]
    sc = rstd * gm
    sh = beta.float().view(1, 1, groups, cg) - mu * sc
    f = xf * sc + sh
    if silu:
        f = f * (1.0 / (1.0 + torch.exp2(-LOG2E * f)))
    return f.half().view(B, HW, C)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def ln_terms(x, gamma, beta, eps):
    """(y, dy) fp64 of LayerNorm over the last dim of x [rows, C]: the value and the error of the kernel's fp32 result before any store."""
    C = x.shape[-1]
    xd, gm, bt = x.double(), gamma.double(), beta.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    rn = ACC_C * U32 * math.sqrt(C)
    d_mean = rn * xd.abs().mean(-1, keepdim=True)
    eps_r = rn * (xd * xd).mean(-1, keepdim=True) / (var + eps) + 8 * U32
    pre = (xd - mean) * rstd * gm
    y = pre + bt
    dy = gm.abs() * rstd * ((xd - mean).abs() * eps_r + d_mean) + 4 * U32 * (pre.abs() + bt.abs())
    return y, dy


def ln_reference(x, gamma, beta, eps):
    """(want, bound) fp64 of LayerNorm over the last dim of x [rows, C], fp16 store included."""
    y, dy = ln_terms(x, gamma, beta, eps)
    bound = dy * (1 + U16) + U16 * y.abs() + 2.0 ** -25
    return y, clamp_to_close(y, bound, CLOSE["norm"])


def ln_emulate(x, gamma, beta, eps, var_divisor=None):
    """layernorm_kernel in plain fp32 (mean, centred variance, rsqrt); mutation: the variance divided by var_divisor instead of C."""
    C = x.shape[-1]
    xf = x.float()
    mean = xf.sum(-1, keepdim=True) / C
    d = xf - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / float(var_divisor or C) + eps)
    return (d * rstd * gamma.float() + beta.float()).half()


# ---- softmax rows, GEGLU, timestep embedding --------------------------------------------------------------------------------------
def softmax_reference(x, scale):
    cols = x.shape[-1]
    xd = x.double()
    w = torch.softmax(xd * scale, -1)
    sl = scale * LOG2E
    arg = LN2 * U32 * sl * (2 * xd.abs() + (xd - xd.max(-1, keepdim=True).values).abs())
    bound = U16 * w + 2.0 ** -25 + w * (arg + ACC_C * U32 * math.sqrt(cols))
    return w, clamp_to_close(w, bound, CLOSE["softmax"])


def softmax_emulate(x, scale, scale_fp16=False):
    """softmax_rows_kernel in plain fp32; mutation: `scale` rounded to fp16 before it is used."""
    if scale_fp16:
        scale = float(torch.tensor(scale).half())
    sl = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    xf = x.float()
    mx = xf.max(-1, keepdim=True).values * sl
    e = torch.exp2(xf * sl - mx)
    return (e * (1.0 / e.sum(-1, keepdim=True))).half()


def geglu_reference(h):
    """h [M, 2F] = (value | gate) halves, fp16-valued: (want, bound) of value * gelu(gate)."""
    F_ = h.shape[-1] // 2
    a, g = h[..., :F_].double(), h[..., F_:].double()
    gel = g * 0.5 * (1 + torch.erf(g / math.sqrt(2.0)))
    y = a * gel
    dy = GELU_FIT * a.abs() + 4 * U32 * y.abs()
    return y, clamp_to_close(y, dy * (1 + U16) + U16 * y.abs() + 2.0 ** -25, CLOSE["geglu"])


def geglu_emulate(h):
    F_ = h.shape[-1] // 2
    a, g = h[..., :F_].float(), h[..., F_:].float()
    return (a * (g * 0.5 * (1 + torch.erf(g * 0.7071067811865476)))).half()


def temb_reference(t, dim, max_period=10000.0):
    """fp64 timestep embedding [cos | sin] of integer timesteps t [B] (ldm/modules/diffusionmodules/util.py) and its bound."""
    half = dim // 2
    kk = torch.arange(half, dtype=torch.float64, device=t.device)
    ck = -math.log(max_period) * kk / half
    ang = t.double()[:, None] * torch.exp(ck)[None]
    y = torch.cat([torch.cos(ang), torch.sin(ang)], -1)
    d_ang = U32 * ang.abs() * (5 + 4 * ck.abs())[None]
    dy = torch.cat([d_ang, d_ang], -1) + 4 * U32
    if dim % 2:
        y, dy = torch.cat([y, torch.zeros_like(y[:, :1])], -1), torch.cat([dy, torch.zeros_like(dy[:, :1])], -1)
    return y, clamp_to_close(y, dy * (1 + U16) + U16 * y.abs() + 2.0 ** -25, CLOSE["temb"])


def temb_emulate(t, dim, max_period=10000.0):
    half = dim // 2
    c = torch.tensor(-math.log(max_period), dtype=torch.float32) / float(half)
    f = torch.exp(c * torch.arange(half, dtype=torch.float32, device=t.device))
    ang = t.float()[:, None] * f[None]
    return torch.cat([torch.cos(ang), torch.sin(ang)], -1).half()


# ---- the cases both test files run --------------------------------------------------------------------------------------------------
# 1a: (instantiation, B, H, Nq, Nk, D, qw, mpad).  B * H = 8 with several query blocks takes the XCD grid decoding, B * H = 3 the plain one;
# every Nk has a ragged last tile and at least three tiles; Nq != Nk, off 32 / 64 / 128.
PIN_CASES = [
    ("16,1", 1, 3, 100, 200, 8, 0, 1), ("16,1", 2, 4, 300, 330, 16, 0, 1),
    ("32,1", 1, 3, 130, 200, 24, 0, 1), ("32,1", 2, 4, 300, 203, 32, 0, 1),
    ("48,1,1,true", 2, 4, 300, 330, 40, 0, 1), ("48,1,1,true", 1, 3, 100, 200, 40, 1, 1),
    ("48,2,1,true", 2, 4, 600, 200, 40, 2, 1), ("48,2,1,true", 1, 3, 130, 330, 40, 2, 1),
    ("48,2,2,true", 8, 8, 1900, 200, 40, 0, 1),
    ("48,1", 1, 3, 100, 200, 48, 0, 1), ("48,1", 2, 4, 300, 330, 40, 1, 0),
    ("48,2", 2, 4, 600, 200, 48, 2, 1), ("48,2", 1, 3, 130, 330, 40, 2, 0),
    ("48,2,2", 2, 4, 600, 330, 48, 3, 1), ("48,2,2", 1, 3, 130, 200, 40, 3, 0),
    ("64,1", 1, 3, 100, 200, 56, 0, 1), ("64,1", 2, 4, 300, 330, 64, 1, 1),
    ("64,2", 2, 4, 600, 200, 64, 2, 1), ("64,2", 1, 3, 130, 330, 56, 2, 1),
    ("80,1", 1, 3, 100, 200, 72, 0, 1), ("80,1", 2, 4, 300, 330, 80, 1, 1),
    ("80,2", 2, 4, 600, 200, 80, 2, 1), ("80,2", 1, 3, 130, 330, 72, 2, 1),
    ("128,1", 1, 3, 100, 200, 104, 0, 1), ("128,1", 2, 4, 300, 330, 128, 0, 1),
    ("160,1", 1, 3, 100, 200, 136, 0, 1), ("160,1", 2, 4, 300, 330, 160, 0, 1),
]

# 1b / 1c: (B, H, Nq, Nk, D, recipe, qw, mpad, q_prescaled, sliced).  sliced: q | k are column slices of one [B, N, 2 H D] buffer.
ATTN_CASES = [(B, H, Nq, Nk, D, "randn", 0, 1, False, Nq == Nk) for B, H, Nq, Nk, D in (
    (8, 8, 4096, 4096, 40), (4, 8, 4096, 4096, 40), (8, 8, 1024, 1024, 80), (8, 8, 256, 256, 160), (8, 8, 64, 64, 160), (4, 16, 257, 257, 64),
    (2, 8, 4096, 4096, 40), (2, 8, 9216, 9216, 40), (2, 8, 130, 7, 40))]
ATTN_CASES += [                                      # one per instantiation the shapes above do not reach
    (2, 4, 330, 330, 16, "randn", 0, 1, False, True), (2, 4, 330, 330, 32, "randn", 0, 1, False, True),
    (2, 8, 1000, 1000, 40, "randn", 2, 1, False, True), (2, 8, 1000, 1000, 40, "randn", 2, 1, True, True),
    (2, 4, 330, 330, 48, "randn", 0, 1, False, True), (2, 8, 1000, 1000, 48, "randn", 2, 1, False, True),
    (2, 8, 1000, 1000, 40, "randn", 3, 0, False, True), (2, 8, 1000, 1000, 64, "randn", 2, 1, False, True),
    (2, 8, 1000, 1000, 80, "randn", 2, 1, False, True), (1, 3, 200, 200, 128, "randn", 0, 1, False, True)]
ATTN_CASES += [(1, 2, 330 if r == "ragged_jump_in_last_tile" else 384, 330 if r == "ragged_jump_in_last_tile" else 384, D, r, 0, 1, False, False)
               for D in (40, 64, 80) for r in FORCED]


def attn_case_id(c):
    B, H, Nq, Nk, D, recipe, qw, mpad, pre, sliced = c
    return f"a:{B}:{H}:{Nq}:{Nk}:{D}" + (f"-{recipe}" if recipe != "randn" else "") + (f"-qw{qw}" if qw else "") + ("" if mpad else "-mpad0") + \
        ("-prescaled" if pre else "")


def attn_case_close(c):
    """_close limit of the existing test of the case (test_ops_gpu.py): large_logits in the d = 40 form without q_prescaled has its own."""
    return CLOSE["attention_loose" if c[5] == "large_logits" and c[4] == 40 and c[7] and not c[8] else "attention"]


def attn_case_operands(c, device="cpu"):
    """(q, k, v fp16 [B, N, H D] drawn on `device`, scale_log2e of the reference, scale and q_prescaled of the launch) of an ATTN_CASES entry;
    with q_prescaled the q operand IS round16(q scale log2e) and the reference takes it at scale log2e = 1."""
    B, H, Nq, Nk, D, recipe, qw, mpad, pre, sliced = c
    seed = Nq + D if recipe == "randn" else 17 + D
    q, k, v = attn_operands(B, H, Nq, Nk, D, seed, recipe, device)
    scale = D ** -0.5
    if pre:
        q = (q.float() * (scale * LOG2E)).half()
        return q, k, v, 1.0, scale, True
    return q, k, v, scale * LOG2E, scale, False
