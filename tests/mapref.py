"""References for exemplar attribution maps: the head-mean softmax weights that the fused cross-attention kernel brings out as a side
output (pbe_ctx_attention_map_f16, include/pbe_hip.h).  Helpers imported by test_ctx_maps_cpu.py and test_ctx_maps_gpu.py; ctxref,
regionref and kbiasref are imported, not edited.  Not a conftest: plain functions only, on whatever device the operands live.

The map of sample b is m[b, t, j] = (1 / H) sum_h p[b, t, h, j], p the softmax over the Nk context tokens of head h at query row t
(ldm/modules/attention.py:207-230 of the reference: `sim.softmax(dim=-1)`), with the exemplar weights / regional table in the scores.
One `table` [B, N, Nk] (log2 domain, -inf = absent) stands for all three launch forms: zeros are the plain launch, log2 w[b, j] on every
row the weighted launch, a regional table the row-weight launch (the kernel's own bit identities, tests/test_ctx_regions_gpu.py).

  reference     fp64: mean over the heads of softmax_j(LayerNorm(x) . kq + kbias + table), written from LayerNorm(x) itself.
  emulate       the kernel's arithmetic in fp32: regionref.emulate's scores (kbias + table formed FIRST), the weights rounded to fp16
                once, the heads summed in the order h = 0 .. H-1 in fp32, times the fp32 value 1 / H.  Mutations the verdict must reject:
                no_div - the head sum not divided by H; fewer_heads - the mean of the first H - 1 heads.
  verdict       accepts a map [B, N, Nk] when
                  * every element is finite;
                  * every element is within ABS_BOUND = 2^-11 of the reference.  Derived: each fp16 weight <= 1 is within a half-ulp
                    2^-12 of the fp32 weight, and so is their mean over the heads; the same again is allowed for the fp32 scores and the
                    hardware exp2.  (The emulation's worst element over the twelve shape-and-table cases is 1.6e-4 = 0.32 of it.)
                  * rel-L2 <= ctxref.REL_L2_FACTOR x the emulation's on the same operands;
                  * every row sums to 1 within ROW_BOUND = 2^-10 (Nk <= 16 weights whose half-ulps sum to <= 2^-11, doubled as above);
                  * a token whose effective weight is 0 at a row (table = -inf) maps to exactly 0 there.
  oracle_maps   a context manager around the loaded oracle module: its cross_attention is swapped for one that does the same arithmetic
                (regionref.regional_oracle's body, with or without tables) and records the head-mean softmax of every context call.
"""
from __future__ import annotations

import contextlib

import torch

import ctxref as cr
import regionref as rr
from accgate import LN2, rel_l2

# (B, N, C, H, Nk, partials of the row statistics): a ragged last tile, a single ragged tile, HJ = 128 full, HJ = 15 < 32, odd Nk, H not a
# power of two, several statistics partials, every k-tile count
SHAPES = [(2, 72, 64, 8, 4, 1), (2, 130, 320, 8, 5, 1), (3, 72, 320, 8, 16, 5), (2, 72, 640, 8, 3, 1), (1, 64, 1280, 8, 16, 1), (1, 40, 64, 5, 3, 1)]
GRIDS = {72: (8, 9), 130: (10, 13), 64: (4, 16), 40: (5, 8)}       # N -> the (h, w) grid of the regional table (non-square)
ABS_BOUND = 2.0 ** -11
ROW_BOUND = 2.0 ** -10


def shape_id(s):
    return "B%d-N%d-C%d-H%d-K%d-p%d" % tuple(s)


def region_case(shape, seed=0):
    """regionref.kernel_case at `shape` on its GRIDS grid."""
    return rr.kernel_case(tuple(shape) + GRIDS[shape[1]], seed)


def zeros_table(o):
    return torch.zeros(o.B, o.N, o.Nk, dtype=torch.float64)


def weights_table(o, w):
    """The table of the weighted launch: log2 w[b, j] on every row (fp64; -inf for weight 0)."""
    return torch.log2(w.double())[:, None, :].expand(o.B, o.N, o.Nk).contiguous()


def reference(o, table, eps=cr.EPS):
    """fp64 [B, N, Nk]."""
    B, N, H, Nk = o.B, o.N, o.H, o.Nk
    x = o.x.double().view(B, N, -1)
    mean = x.mean(-1, keepdim=True)
    xh = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    s = xh @ o.kq.double().transpose(1, 2) + o.kbias.double()[:, None, :]
    s = s.view(B, N, H, Nk) + table.double().to(s.device)[:, :, None, :]
    w = torch.exp2(s - s.max(-1, keepdim=True).values)
    return (w / w.sum(-1, keepdim=True)).mean(2)


def emulate(o, table, eps=cr.EPS, no_div=False, fewer_heads=False):
    """fp32 [B, N, Nk]: the AM form's arithmetic (module docstring)."""
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
    s = (rstd.view(B, N, 1) * acc + (nmr.view(B, N, 1) * o.colsum.float()[:, None, :] + kb)).view(B, N, H, Nk)
    e = torch.exp2(s - s.max(-1, keepdim=True).values)
    w = (e * (1.0 / e.sum(-1, keepdim=True))).half().float()                                                     # [B, N, H, Nk], fp16 values
    heads = H - 1 if fewer_heads else H
    m = torch.zeros(B, N, Nk, dtype=torch.float32, device=w.device)
    for h in range(heads):                                                                                       # fixed order, fp32
        m = m + w[:, :, h]
    return m if no_div else m * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(heads), dtype=torch.float32)).to(m.device)


def verdict(got, want, emu, table=None):
    """(accepted, text) of the map `got` [B, N, Nk] against the fp64 `want` = reference(...), `emu` = emulate(...) of the same operands,
    `table` the log2-domain table the scores carried (None: no token is absent)."""
    got = got.detach().cpu()
    if got.shape != want.shape:
        return False, f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not bool(torch.isfinite(got.float()).all()):
        return False, "non-finite map"
    gd = got.double()
    err = float((gd - want.cpu()).abs().max())
    r_got, r_emu = rel_l2(got, want.cpu()), rel_l2(emu.cpu(), want.cpu())
    rows = float((gd.sum(-1) - 1.0).abs().max())
    dead = 0
    if table is not None:
        gone = torch.isinf(table.cpu()) & (table.cpu() < 0)
        dead = int((gd[gone] != 0).sum())
    text = (f"max|d| {err:.3e} (bound {ABS_BOUND:.3e}); rel-L2 {r_got:.3e} (emulation {r_emu:.3e}, limit x{cr.REL_L2_FACTOR}); "
            f"|row sum - 1| {rows:.3e} (bound {ROW_BOUND:.3e}); {dead} non-zero entries of absent tokens")
    return err <= ABS_BOUND and r_got <= cr.REL_L2_FACTOR * r_emu and rows <= ROW_BOUND and dead == 0, text


def gather_numpy(acc, grid, out_hw, scale=1.0, div=1.0):
    """numpy restatement of pbe_ctx_map_gather_f32's store form: acc [B, h*w, K] -> fp32 [B, K, Hl, Wl], every step rounded to fp32."""
    import numpy as np
    h, w = grid
    Hl, Wl = out_hw
    a = np.asarray(acc, dtype=np.float32).reshape(acc.shape[0], h, w, acc.shape[2])
    a = np.repeat(np.repeat(a, Hl // h, 1), Wl // w, 2).transpose(0, 3, 1, 2)
    return (np.float32(scale) * (a / np.float32(div)).astype(np.float32)).astype(np.float32)


@contextlib.contextmanager
def oracle_maps(O, tables=None):
    """While active, the oracle module O's cross_attention records, for every call WITH a context, (query tokens n, head-mean softmax
    fp64 [b, n, K]) into the yielded list, in call order.  tables: as regionref.regional_oracle (log2-domain [B, N, K] per level; a batch
    of twice the size gets [zeros | table]) or None: the unmodified scores.  The arithmetic is the oracle's own, restated as
    regionref.regional_oracle restates it; restores the original on exit."""
    by_n = {} if tables is None else {int(t.shape[1]): t for t in (tables.values() if isinstance(tables, dict) else tables)}
    orig = O.cross_attention
    rec = []

    def cross_attention(sd, p, x, context, heads):
        if context is None:
            return orig(sd, p, x, None, heads)
        b, n, _ = x.shape
        q, k, v = O.linear(x, sd, p + "to_q"), O.linear(context, sd, p + "to_k"), O.linear(context, sd, p + "to_v")
        c = q.shape[2]
        d = c // heads
        split = lambda u: u.reshape(b, u.shape[1], heads, d).permute(0, 2, 1, 3)      # noqa: E731
        q, k, v = split(q), split(k), split(v)
        sim = torch.matmul(q, k.transpose(-1, -2)) * (d ** -0.5)
        if by_n:
            t = by_n[n]
            if b == 2 * t.shape[0]:
                t = torch.cat([torch.zeros_like(t), t])
            assert t.shape[0] == b and t.shape[2] == context.shape[1], (tuple(t.shape), b, tuple(context.shape))
            sim = sim + (t * LN2).to(q.dtype)[:, None, :, :]
        attn = sim.softmax(dim=-1)
        rec.append((n, attn.double().mean(1)))
        out = torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(b, n, c)
        return O.linear(out, sd, p + "to_out.0")
    O.cross_attention = cross_attention
    try:
        yield rec
    finally:
        O.cross_attention = orig
