"""References for the multi-token cross-attention kernel (pbe_ctx_attention_f16, include/pbe_hip.h).  Helpers imported by
test_ctx_attention_cpu.py and test_ctx_attention_gpu.py.  Not a conftest: plain functions only, on whatever device the operands live.

  Operands      the kernel's operands: x fp16 [B * N, C], kq fp16 [B, HJ, C], colsum / kbias fp32 [B, HJ], vo fp16 [B, C, HJ], bias fp32 [C],
                HJ = H * Nk, plus the (sum, sumsq) row statistics of x in `parts` partials (as an out-projection epilogue emits them).
  fold          those operands from a BasicTransformerBlock's weights and a context, in a chosen precision (fp64: the algebra alone).
  reference     fp64 x2 = x + attn2 and the attn2 term from the operands AS SENT, written from LayerNorm(x) itself - not from the
                kernel's rstd (acc - mean colsum) form - so a wrong fold shows.
  emulate       the kernel's arithmetic in plain fp32 torch: fp16 kq / vo, fp32 accumulation, the LayerNorm fold from the fp32 partials,
                exp2 with the group maximum subtracted, weights rounded to fp16 once, fp16 store.  Never a kernel's own output.
  gate          rel-L2 of the result <= REL_L2_FACTOR x the emulation's on the same operands, and the whole-tensor _close limit
                CLOSE["attention"] (both constants are accgate's).  Mutations of the emulation must fail it.
"""
from __future__ import annotations

import torch

from accgate import CLOSE, LOG2E, REL_L2_FACTOR, close_verdict, rel_l2

# (B, N, C, H, Nk, partials of the row statistics)
KERNEL_SHAPES = [(2, 72, 64, 8, 4, 1), (2, 130, 320, 8, 5, 1), (1, 64, 1280, 8, 16, 1), (3, 8, 128, 8, 1, 1), (2, 72, 320, 8, 2, 5)]
LARGE_LOGITS_SHAPE = (2, 72, 320, 8, 4, 1)
EPS = 1e-5


class Operands:
    def __init__(self, x, kq, colsum, kbias, vo, bias, stats, B, N, C, H, Nk):
        self.x, self.kq, self.colsum, self.kbias, self.vo, self.bias, self.stats = x, kq, colsum, kbias, vo, bias, stats
        self.B, self.N, self.C, self.H, self.Nk = B, N, C, H, Nk

    def to(self, device):
        return Operands(*(t.to(device) for t in (self.x, self.kq, self.colsum, self.kbias, self.vo, self.bias, self.stats)),
                        self.B, self.N, self.C, self.H, self.Nk)


def row_partials(x, parts):
    """fp32 [parts, M, 2]: (sum, sumsq) of the fp16 rows of x over `parts` column ranges (the layout of a GEMM's row_stats_out)."""
    M, C = x.shape
    edges = [round(i * C / parts) for i in range(parts + 1)]
    xd = x.double()
    return torch.stack([torch.stack([xd[:, a:b].sum(1), (xd[:, a:b] ** 2).sum(1)], 1) for a, b in zip(edges[:-1], edges[1:])]).float()


def random_operands(B, N, C, H, Nk, parts=1, seed=0, logit_scale=2.0):
    """Seeded operands: rows of x with a per-row offset and spread (LayerNorm has something to do), scores of spread about `logit_scale`
    log2 units (LayerNorm(x) has unit variance, kq rows have norm logit_scale)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + Nk)
    HJ = H * Nk
    x = (torch.randn(B * N, C, generator=g) * (0.5 + torch.rand(B * N, 1, generator=g)) + torch.randn(B * N, 1, generator=g)).half()
    kq = (torch.randn(B, HJ, C, generator=g) * (logit_scale / C ** 0.5)).half()
    kbias = torch.randn(B, HJ, generator=g) * 0.3 * logit_scale
    vo = (torch.randn(B, C, HJ, generator=g) * 0.5).half()
    bias = torch.randn(C, generator=g) * 0.1
    return Operands(x, kq, kq.double().sum(-1).float(), kbias, vo, bias, row_partials(x, parts), B, N, C, H, Nk)


def fold(sd, prefix, context, heads, dtype=torch.float64):
    """(kq, colsum, kbias, vo, bias) of `prefix`attn2 / norm2 (state-dict names of BasicTransformerBlock) for context [B, Nk, Dc]: kq and
    vo in `dtype` (fp64: exact algebra; fp16: what the kernel is sent), the rest fp64 -> fp32 when dtype is fp16."""
    W = lambda n: sd[prefix + n].double()      # noqa: E731
    wq, wk, wv, wo, bo = W("attn2.to_q.weight"), W("attn2.to_k.weight"), W("attn2.to_v.weight"), W("attn2.to_out.0.weight"), W("attn2.to_out.0.bias")
    gam, bet = W("norm2.weight"), W("norm2.bias")
    B, Nk, _ = context.shape
    C = wq.shape[1]
    D = wq.shape[0] // heads
    k = (context.double() @ wk.t()).view(B, Nk, heads, D)
    v = (context.double() @ wv.t()).view(B, Nk, heads, D)
    if dtype == torch.float16:                                      # to_k / to_v leave their GEMM as fp16
        k, v = k.half().double(), v.half().double()
    qs = D ** -0.5 * LOG2E
    wqh = (wq * gam[None, :]).view(heads, D, C)
    kq = qs * torch.einsum("bjhd,hdc->bhjc", k, wqh).reshape(B, heads * Nk, C)
    kbias = qs * torch.einsum("bjhd,hd->bhj", k, (wq @ bet).view(heads, D)).reshape(B, heads * Nk)
    vo = torch.einsum("chd,bjhd->bchj", wo.view(C, heads, D), v).reshape(B, C, heads * Nk)
    kq, vo = kq.to(dtype), vo.to(dtype)
    colsum = kq.double().sum(-1)
    if dtype == torch.float16:
        return kq, colsum.float(), kbias.float(), vo, bo.float()
    return kq, colsum, kbias, vo, bo


def reference(o, eps=EPS):
    """fp64 (x2, attn2 term) [B * N, C] from the operands as sent."""
    B, N, H, Nk = o.B, o.N, o.H, o.Nk
    x = o.x.double().view(B, N, -1)
    mean = x.mean(-1, keepdim=True)
    xh = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    s = xh @ o.kq.double().transpose(1, 2) + o.kbias.double()[:, None, :]                     # [B, N, HJ], log2 domain
    s = s.view(B, N, H, Nk)
    w = torch.exp2(s - s.max(-1, keepdim=True).values)
    w = (w / w.sum(-1, keepdim=True)).view(B, N, H * Nk)
    term = w @ o.vo.double()[:, :, :H * Nk].transpose(1, 2) + o.bias.double()
    return (x + term).view(B * N, -1), term.view(B * N, -1)


def emulate(o, eps=EPS, no_max=False, pad_weight=False, drop_colsum=False):
    """The kernel's arithmetic in fp32 (module docstring) -> fp16 [B * N, C].  Mutations: no_max - exp2 of the raw scores; pad_weight - the
    last head's softmax also runs over one padding column (the clamped copy of the last kq row), which then carries weight;
    drop_colsum - the mean * colsum term of the LayerNorm fold is left out."""
    B, N, H, Nk = o.B, o.N, o.H, o.Nk
    HJ = H * Nk
    C = o.x.shape[1]
    st = o.stats.float()
    a, q = torch.zeros_like(st[0, :, 0]), torch.zeros_like(st[0, :, 1])
    for z in range(st.shape[0]):                                    # the partials in order, fp32
        a, q = a + st[z, :, 0], q + st[z, :, 1]
    mean = a.double() / C
    var = (q.double() / C - mean * mean).float()
    rstd = torch.rsqrt(var.clamp_min(0.0) + torch.tensor(eps, dtype=torch.float32, device=st.device))
    nmr = -(mean.float()) * rstd
    x = o.x.float().view(B, N, C)
    acc = x @ o.kq.float().transpose(1, 2)                          # fp32 accumulation
    fold_c = o.kbias.float()[:, None, :] if drop_colsum else nmr.view(B, N, 1) * o.colsum.float()[:, None, :] + o.kbias.float()[:, None, :]
    s = (rstd.view(B, N, 1) * acc + fold_c).view(B, N, H, Nk)
    mx = torch.zeros_like(s[..., :1]) if no_max else s.max(-1, keepdim=True).values
    e = torch.exp2(s - mx)
    den = e.sum(-1, keepdim=True)
    if pad_weight:
        den = den.clone()
        den[:, :, H - 1] += e[:, :, H - 1, Nk - 1:Nk]
    w = (e * (1.0 / den)).half().float().view(B, N, HJ)
    y = w @ o.vo.float()[:, :, :HJ].transpose(1, 2) + o.bias.float() + x
    return y.half().view(B * N, C)


def verdict(got, want, emu):
    """(accepted, text): the gate on `got` (fp16 [M, C]) against the fp64 `want`, `emu` = emulate() of the same operands."""
    if not bool(torch.isfinite(got.float()).all()):
        return False, "non-finite result"
    r_got, r_emu = rel_l2(got, want), rel_l2(emu, want)
    ok_close, err, lim = close_verdict(got, want, CLOSE["attention"])
    text = f"rel_l2 {r_got:.3e} (emulation {r_emu:.3e}, limit x{REL_L2_FACTOR}); max|d| {err:.3e} (limit {lim:.3e})"
    return r_got <= REL_L2_FACTOR * r_emu and ok_close, text
