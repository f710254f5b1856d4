"""References for regional exemplars: a weight per (sample, query row, context token) on the fused cross-attention kernel
(pbe_ctx_attention_rw_f16, include/pbe_hip.h).  Helpers imported by test_ctx_regions_cpu.py and test_ctx_regions_gpu.py.  Not a
conftest: plain functions only, on whatever device the operands live.

Semantics (ldm/modules/attention.py:207-230 of the reference with token j of sample b counted e[b, t, j] >= 0 times at query row t):
the softmax weight of token j at row t is e[b,t,j] exp(s_j) / sum_i e[b,t,i] exp(s_i), i.e. log2 e[b, t, j] joins the score in the
kernel's log2 domain.  e = w[b, j] x (area average of regions[b, j] over the level's grid cell t = y*w + x); a row whose e sums to 0
takes e[b, t, :] = w[b, :].

  level_table     that rule in fp64 -> log2 e [B, h*w, K] (-inf for 0), written independently of ldm.modules.attention.ContextRegions.
  reference       ctxref.reference with the per-row term added to the scores, written from LayerNorm(x).
  emulate         ctxref.emulate with kbias + table formed FIRST in fp32 (the kernel's add order), then the same arithmetic.
  mutations       of the table, which the gate (ctxref.verdict, unchanged constants) must reject: `transposed` - row y*w + x reads entry
                  x*h + y; `next_sample` - sample b takes the table of sample b + 1; `ignored` - zeros; `bare_absent` - the fallback rows
                  left all-absent (-inf on the whole row: a non-finite result).
  regional_oracle a context manager that swaps the loaded oracle module's cross_attention for one that adds ln e to `sim`.
  subset_composition   the unmodified oracle run per distinct token subset on that sub-context, rows gathered by subset: exact for
                  binary e on a depth-1 transformer (only attn1 mixes rows, and it does not see the context).
"""
from __future__ import annotations

import contextlib
import math

import torch

import ctxref as cr
from accgate import LN2

# (B, N, C, H, Nk, partials of the row statistics, h, w) with N = h * w: ragged last row tiles (72, 130), a full H * Nk = 128, several
# statistics partials, non-square grids (a transposed row order cannot pass), the widest C
SHAPES = [(2, 72, 64, 8, 4, 1, 8, 9), (2, 130, 320, 8, 5, 1, 10, 13), (3, 72, 320, 8, 16, 5, 8, 9), (2, 72, 640, 8, 3, 1, 9, 8),
          (1, 64, 1280, 8, 16, 1, 4, 16)]
MUTATIONS = ("transposed", "next_sample", "ignored")
INF = math.inf


def shape_id(s):
    return "B%d-N%d-C%d-H%d-K%d-p%d-%dx%d" % s


def level_weights(regions, weights, h, w, fallback=True):
    """fp64 e [B, h*w, K] from regions [B, K, Hr, Wr] and weights [B, K] (None: ones)."""
    r = torch.as_tensor(regions).double()
    B, K, Hr, Wr = r.shape
    assert Hr % h == 0 and Wr % w == 0, (Hr, Wr, h, w)
    wt = torch.ones(B, K, dtype=torch.float64) if weights is None else torch.as_tensor(weights).double()
    fy, fx = Hr // h, Wr // w
    e = torch.empty(B, h * w, K, dtype=torch.float64)
    for y in range(h):
        for x in range(w):
            e[:, y * w + x, :] = r[:, :, y * fy:(y + 1) * fy, x * fx:(x + 1) * fx].sum((2, 3)) / (fy * fx) * wt
    if fallback:
        for b in range(B):
            bare = e[b].sum(-1) <= 0
            e[b, bare] = wt[b]
    return e


def level_table(regions, weights, h, w, fallback=True):
    """fp64 log2 e [B, h*w, K], -inf where e = 0."""
    return torch.log2(level_weights(regions, weights, h, w, fallback))


def kernel_case(shape, seed=0):
    """The tables of the kernel tests at `shape`: regions at twice the level resolution drawn uniformly from [0, 1) and zeroed below
    0.6, one level cell per sample cleared for every token (a fallback row), weights exp2(2 randn); drawn for B + 1 samples so that
    `next_sample` differs at B = 1 too.  Returns dict(table fp64 [B, N, Nk], bare_absent, next_sample, regions, weights, cells)."""
    B, N, C, H, Nk, parts, h, w = shape
    g = torch.Generator().manual_seed(4000 + 13 * seed + C + Nk)
    r = torch.rand(B + 1, Nk, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    r = torch.where(r < 0.6, torch.zeros_like(r), r)
    cells = []
    for b in range(B + 1):
        y, x = (3 * b + 1) % h, (5 * b + 2) % w
        r[b, :, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = 0.0
        cells.append(y * w + x)
    wt = torch.exp2(2.0 * torch.randn(B + 1, Nk, generator=g, dtype=torch.float64))
    full = level_table(r, wt, h, w)
    bare = level_table(r, wt, h, w, fallback=False)
    return dict(table=full[:B], next_sample=full[1:B + 1], bare_absent=bare[:B], regions=r[:B], weights=wt[:B], cells=cells[:B])


def mutate(case, kind, h, w):
    """The table a wrong kernel / wrong host code would have used (module docstring)."""
    t = case["table"]
    B, N, K = t.shape
    if kind == "transposed":
        return t.view(B, w, h, K).transpose(1, 2).reshape(B, N, K)
    if kind == "next_sample":
        return case["next_sample"]
    if kind == "ignored":
        return torch.zeros_like(t)
    assert kind == "bare_absent", kind
    return case["bare_absent"]


def reference(o, table, eps=cr.EPS):
    """fp64 (x2, attn2 term) [B * N, C] from the operands as sent and the table [B, N, Nk] (log2 domain)."""
    B, N, H, Nk = o.B, o.N, o.H, o.Nk
    x = o.x.double().view(B, N, -1)
    mean = x.mean(-1, keepdim=True)
    xh = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    s = xh @ o.kq.double().transpose(1, 2) + o.kbias.double()[:, None, :]
    s = s.view(B, N, H, Nk) + table.double().to(s.device)[:, :, None, :]
    w = torch.exp2(s - s.max(-1, keepdim=True).values)
    w = (w / w.sum(-1, keepdim=True)).view(B, N, H * Nk)
    term = w @ o.vo.double()[:, :, :H * Nk].transpose(1, 2) + o.bias.double()
    return (x + term).view(B * N, -1), term.view(B * N, -1)


def emulate(o, table, eps=cr.EPS):
    """The RW form's arithmetic in fp32 -> fp16 [B * N, C]: ctxref.emulate with (kbias + table) formed first, in fp32, per row."""
    B, N, H, Nk = o.B, o.N, o.H, o.Nk
    HJ = H * Nk
    C = o.x.shape[1]
    st = o.stats.float()
    a, q = torch.zeros_like(st[0, :, 0]), torch.zeros_like(st[0, :, 1])
    for z in range(st.shape[0]):
        a, q = a + st[z, :, 0], q + st[z, :, 1]
    mean = a.double() / C
    var = (q.double() / C - mean * mean).float()
    rstd = torch.rsqrt(var.clamp_min(0.0) + torch.tensor(eps, dtype=torch.float32, device=st.device))
    nmr = -(mean.float()) * rstd
    x = o.x.float().view(B, N, C)
    acc = x @ o.kq.float().transpose(1, 2)
    kb = (o.kbias.float().view(B, 1, H, Nk) + table.float().to(x.device).view(B, N, 1, Nk)).view(B, N, HJ)       # the fp32 add comes first
    fold_c = nmr.view(B, N, 1) * o.colsum.float()[:, None, :] + kb
    s = (rstd.view(B, N, 1) * acc + fold_c).view(B, N, H, Nk)
    mx = s.max(-1, keepdim=True).values
    e = torch.exp2(s - mx)
    den = e.sum(-1, keepdim=True)
    w = (e * (1.0 / den)).half().float().view(B, N, HJ)
    y = w @ o.vo.float()[:, :, :HJ].transpose(1, 2) + o.bias.float() + x
    return y.half().view(B * N, C)


def verdict(got, o, table):
    """ctxref.verdict of `got` against reference(o, table), with emulate(o, table) as the emulation."""
    return cr.verdict(got, reference(o, table)[0], emulate(o, table))


# ---- module-level tests: binary and soft regions on an h x w grid -----------------------------------------------------------------------
def binary_regions(B, h, w, up=1):
    """[B, 3, up*h, up*w]: token 0 on the left half, token 1 on the right half, token 2 on rows 2-4, and one cell per sample - (6, 7 + b) -
    that nothing covers (a fallback row)."""
    r = torch.zeros(B, 3, h, w, dtype=torch.float64)
    r[:, 0, :, :w // 2] = 1.0
    r[:, 1, :, w // 2:] = 1.0
    r[:, 2, 2:5, :] = 1.0
    for b in range(B):
        r[b, :, 6 % h, (7 + b) % w] = 0.0
    return r.repeat_interleave(up, 2).repeat_interleave(up, 3)


def soft_regions(B, K, h, w, seed, up=1):
    """[B, K, up*h, up*w] fractions: uniform [0, 1) zeroed below 0.4, one level cell per sample cleared for every token."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, K, up * h, up * w, generator=g, dtype=torch.float64)
    r = torch.where(r < 0.4, torch.zeros_like(r), r)
    for b in range(B):
        y, x = (2 * b + 1) % h, (3 * b + 2) % w
        r[b, :, up * y:up * (y + 1), up * x:up * (x + 1)] = 0.0
    return r


def subset_composition(fn, ctx, e):
    """fn(b, context [1, K', Dc]) -> [1, C, h, w] of the UNMODIFIED oracle, run once per distinct token subset of sample b (the tokens with
    e[b, t, :] > 0) and gathered by the positions t = y*w + x that have that subset.  e [B, h*w, K] must be 0 / 1."""
    assert bool(((e == 0) | (e == 1)).all())
    outs = []
    for b in range(ctx.shape[0]):
        keys = [tuple(int(v) for v in row) for row in (e[b] > 0).tolist()]
        out = None
        for key in sorted(set(keys)):
            tok = [j for j, v in enumerate(key) if v]
            y = fn(b, ctx[b:b + 1, tok])
            if out is None:
                out = torch.empty_like(y)
            sel = torch.tensor([k == key for k in keys]).view(1, 1, *y.shape[2:]).expand_as(y)
            out = torch.where(sel, y, out)
        outs.append(out)
    return torch.cat(outs)


@contextlib.contextmanager
def regional_oracle(O, tables):
    """While active, the oracle module O's cross_attention adds ln e[b, t, j] to `sim` whenever a context is given.  tables: the log2-
    domain tables [B, N, K] (level_table) of the levels in play; the one whose N equals the query token count is taken, and a batch
    of twice its size gets [zeros | table] - the unconditional half of a guidance pair carries ones.  Restores the original."""
    by_n = {int(t.shape[1]): t for t in (tables.values() if isinstance(tables, dict) else tables)}
    assert len(by_n) == len(tables), "two tables with one token count"
    orig = O.cross_attention

    def cross_attention(sd, p, x, context, heads):
        if context is None:
            return orig(sd, p, x, None, heads)
        b, n, _ = x.shape
        t = by_n[n]
        if b == 2 * t.shape[0]:
            t = torch.cat([torch.zeros_like(t), t])
        assert t.shape[0] == b and t.shape[2] == context.shape[1], (tuple(t.shape), b, tuple(context.shape))
        q, k, v = O.linear(x, sd, p + "to_q"), O.linear(context, sd, p + "to_k"), O.linear(context, sd, p + "to_v")
        c = q.shape[2]
        d = c // heads
        split = lambda u: u.reshape(b, u.shape[1], heads, d).permute(0, 2, 1, 3)      # noqa: E731
        q, k, v = split(q), split(k), split(v)
        sim = torch.matmul(q, k.transpose(-1, -2)) * (d ** -0.5) + (t * LN2).to(q.dtype)[:, None, :, :]
        out = torch.matmul(sim.softmax(dim=-1), v).permute(0, 2, 1, 3).reshape(b, n, c)
        return O.linear(out, sd, p + "to_out.0")
    O.cross_attention = cross_attention
    try:
        yield
    finally:
        O.cross_attention = orig
