"""Numerical gate for the tuned tile table (pbe_amd/tuned_mi355x.json): helpers imported by test_tuned_table_gpu.py and
test_tilecheck_cpu.py.  Not a conftest: plain functions only.

case_of(key) turns a table key into a launch description - shapes, epilogue, operand builders, sampled output rows - by this rule:

  g:M:N:K:1      bias + fp16 residual; N == 8K (the feed-forward projection) takes GEGLU (act 4) instead of the residual
  g:M:N:K:b>1    strided batch, W shared over the batch (sW = 0), bias
  g8:...         ops.gemm_f8 on e4m3 operands quantised by pack_linear_f8 (batch 1: the g rule; batch > 1: the V^T layout, A shared)
  gx:M:N:K:1     N == 8K: LayerNorm fold + GEGLU; N == 3K: LayerNorm fold + alpha on the q columns + V^T columns (vt_col0 = 2K, tokens
                 per sample of the U-Net level: K 320 -> 4096, 640 -> 1024, 1280 -> 256, or 64 for the 8x8 level where 256 does not
                 divide M); N == K: residual + row vector (group_rows = tokens) + row_stats.  Rows m % 97 == 0 of A get +6.0 (mean
                 >> std, the cancellation case of the fold)
  c:B:H:W:C1:C2:Cout:stride:pad:ups
                 C2 > 0 reads a two-source concat; ups == 2 is pack_conv3x3_up_phases, ups == 1 upsamples in the gather; stride 1
                 without upsampling: bias + row vector + residual + group_stats=32 (Cout % 32 == 0); everything else bias only

If the fused epilogue makes the planner pick another (tile, split-K) than the table names, the case falls back to the plain epilogue
(bias only; gx: the LayerNorm fold alone, or row_stats alone) and its id says so ("<key>|plain").

Reference: fp64 over ALL N columns and the full K for sampled output rows only, from the fp16 (or dequantised fp8) operands that
were sent to the device.  GEMM: the whole first and last M-tile of the planned BM and 256 seeded rows (first and last batch).
Conv: whole output image rows - first and last row of the first and last sample, the rows on each side of the first tile
boundary, and seeded rows - by F.conv2d in fp64 on the matching input crop.

Per-element bound (rounding model; u32 = 2^-24, u16 = 2^-11, S = (|A| @ |W|^T) of the element):
  accumulation      ACC_C * u32 * sqrt(K) * S                                   (fp32 sums in any order, incl. split-K slabs)
  epilogue in fp32  2 u32 per operation of the magnitudes involved (alpha, bias, row vector)
  LayerNorm fold    rstd * (acc term + 4 u32 (|acc| + |mean colsum|) + d_mean |colsum|) + |pre| * eps_r, with the one-pass fp32 row
                    statistics' errors d_mean = ACC_C u32 sqrt(K) E|x| and eps_r = ACC_C u32 sqrt(K) E[x^2] / (var + eps) (relative, rstd)
  GEGLU             |gelu(g)| d_v + 1.13 |v| d_g + 7.1e-7 |v| (the kernel's GELU fit)
  act 1 / 2 / 3     max |act'| (1.1 SiLU and quick-GELU, 1.13 GELU) times the pre-activation's error + the arm's own rounding (actref.py)
  fp16 stores       u16 |value| + 2^-25 for the stored value, and again after the residual add
and never looser than the limit of the existing _close test of the same op (rtol * max|ref| + atol over the sampled elements).
"""
from __future__ import annotations

import json
import math
import os
import zlib

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "pbe_amd", "tuned_mi355x.json")

U32, U16 = 2.0 ** -24, 2.0 ** -11
ACC_C = 8.0                 # the small multiple of the accumulation term
GELU_FIT = 7.1e-7           # |gelu_erf_f - gelu| (pbe_amd/csrc/common.h)
TOKENS = {320: 4096, 640: 1024, 1280: 256}
LN_OFFSET = 6.0
RANDOM_ROWS = 256           # GEMM: seeded rows besides the first and last M-tile
RANDOM_IMAGE_ROWS = 6       # conv: seeded output image rows
QSCALE = 0.2281             # alpha of the q columns (the attention scale the model folds in)
GROUPS = 32
# _close limits (rtol, atol) of the existing test of each op (tests/test_ops_gpu.py)
CLOSE = {"gemm": (2e-3, 1e-3), "ln": (3e-3, 3e-3), "f8": (1.5e-3, 1.5e-3), "conv": (2e-3, 1e-3)}


def load_table():
    with open(TABLE_PATH) as f:
        return json.load(f)


def seed_of(key: str) -> int:
    return zlib.crc32(key.encode()) & 0x7FFFFFFF


# ---- launch descriptions ----------------------------------------------------------------------------------------------------------
class Case:
    """One table entry as a launch: form, dims, the epilogue flags, the table's (tile, split-K) and the planned BM / BN."""

    def __init__(self, key, value):
        self.key, self.value = key, int(value)
        self.tile, self.splits = self.value & 255, max(1, self.value >> 8)
        self.form, *f = key.split(":")
        f = list(map(int, f))
        self.fallback = False
        self.bias, self.resid, self.rowvec, self.act = True, False, False, 0
        self.ln = self.vt = self.row_stats = False
        self.group_stats, self.alpha, self.alpha_cols, self.tokens, self.offset = 0, 1.0, 0, 0, False
        self.wscale = 1.0                        # weights are drawn at wscale / sqrt(K): the pre-activation's std (actref.py raises it to 3)
        if self.form == "c":
            self.B, self.H, self.W, self.C1, self.C2, self.Cout, self.stride, self.pad, self.ups = f
            hv, wv = (2 * self.H, 2 * self.W) if self.ups else (self.H, self.W)
            extra = 2 if self.pad else 1
            self.Ho, self.Wo = (hv + extra - 3) // self.stride + 1, (wv + extra - 3) // self.stride + 1
            self.K = 4 * self.C1 if self.ups == 2 else 9 * (self.C1 + self.C2)
        else:
            self.M, self.N, self.K, self.batch = f
        self._fused()
        self.bm = self.bn = 0

    def _fused(self):
        if self.form in ("g", "g8"):
            if self.batch == 1:
                if self.N == 8 * self.K:
                    self.act = 4
                else:
                    self.resid = True
            else:
                self.bias = self.form == "g"
        elif self.form == "gx":
            self.offset = True
            if self.N == 8 * self.K:
                self.ln, self.act = True, 4
            elif self.N == 3 * self.K:
                self.ln, self.vt, self.alpha, self.alpha_cols = True, True, QSCALE, self.K
                t = TOKENS[self.K]
                self.tokens = t if self.M % t == 0 else 64
            elif self.N == self.K:
                self.resid = self.rowvec = self.row_stats = True
                self.tokens = TOKENS[self.K]
            else:
                raise ValueError(f"{self.key}: no gx epilogue rule for N / K = {self.N / self.K}")
        else:
            if self.stride == 1 and not self.ups:
                self.rowvec = self.resid = True
                self.group_stats = GROUPS if self.Cout % GROUPS == 0 else 0

    def _plain(self):
        self.fallback = True
        self.resid = self.rowvec = False
        self.act, self.group_stats = 0, 0
        if self.form == "gx":
            if self.vt:                          # LayerNorm fold alone
                self.vt, self.alpha, self.alpha_cols = False, 1.0, 0
            elif not self.ln:                    # row statistics alone
                self.row_stats = True

    @property
    def id(self):
        return self.key + ("|plain" if self.fallback else "")

    @property
    def out_cols(self):
        return self.N // 2 if self.act == 4 else (2 * self.K if self.vt else self.N)

    @property
    def close(self):
        if self.form == "c":
            return CLOSE["conv"]
        if self.form == "g8":
            return CLOSE["f8"]
        return CLOSE["ln"] if self.ln else CLOSE["gemm"]

    def describe(self):
        e = [n for n, on in (("bias", self.bias), ("resid", self.resid), ("rowvec", self.rowvec), ("geglu", self.act == 4), ("ln", self.ln),
                             ("vt", self.vt), ("row_stats", self.row_stats), (f"group_stats{self.group_stats}", self.group_stats)) if on]
        return f"{self.id} tile {self.tile} split {self.splits} [{'+'.join(e) or 'none'}]"


# ---- host-side plans (pbe_gemm_plan / pbe_conv3x3_plan: nothing is launched) ------------------------------------------------------
_FAKE = 1 << 20


def descriptor(case: Case, tile_cfg=None):
    """The descriptor ops.gemm / ops.gemm_f8 / ops.conv3x3 would build for this case, with non-null aligned fake pointers."""
    import ctypes
    from pbe_amd import lib, ops
    cfg = case.value if tile_cfg is None else tile_cfg
    if case.form == "c":
        d = lib.Conv3x3Desc()
        d.X, d.Wp, d.Y = _FAKE, _FAKE, _FAKE
        d.X2 = _FAKE if case.C2 else None
        d.bias = _FAKE if case.bias else None
        d.rowvec = _FAKE if case.rowvec else None
        d.resid = _FAKE if case.resid else None
        d.B, d.H, d.W, d.C1, d.C2, d.Cout = case.B, case.H, case.W, case.C1, case.C2, case.Cout
        d.stride, d.pad, d.upsample = case.stride, case.pad, case.ups
        d.ldv = case.Cout if case.rowvec else 0
        d.act, d.workspace, d.workspace_bytes, d.tile_cfg, d.kblock = case.act, _FAKE, ops.SPLITK_WS_BYTES, cfg, 64
        if case.group_stats:
            case._gs_blocks = ctypes.c_int32(0)
            d.group_stats_out, d.group_stats_groups = _FAKE, case.group_stats
            d.group_stats_blocks = ctypes.cast(ctypes.pointer(case._gs_blocks), ctypes.c_void_p)
        return d
    M, N, K, b = case.M, case.N, case.K, case.batch
    d = lib.GemmDesc()
    d.A, d.W, d.C = _FAKE, _FAKE, _FAKE
    d.bias = _FAKE if case.bias else None
    d.M, d.N, d.K, d.K1, d.lda, d.ldw, d.ldc = M, N, K, K, K, K, case.out_cols
    d.batch, d.alpha, d.act, d.tile_cfg = b, case.alpha, case.act, cfg
    d.group_rows = 1
    if case.resid:
        d.resid, d.ldr = _FAKE, N
    if case.rowvec:
        d.rowvec, d.ldv, d.group_rows = _FAKE, N, case.tokens
    if case.form == "g8":
        d.operand_dtype, d.a_scale, d.w_scale = 1, _FAKE, _FAKE
        if b > 1:                                # V^T layout: A (and its scale) shared, W per sample
            d.strideA, d.strideW, d.strideC, d.w_scale_stride = 0, N * K, M * N, N
    else:
        d.workspace, d.workspace_bytes = _FAKE, ops.SPLITK_WS_BYTES
        if b > 1:                                # W shared over the batch
            d.strideA, d.strideW, d.strideC = M * K, 0, M * N
    if case.form == "gx":
        d.alpha_cols = case.alpha_cols
        if case.ln:
            d.ln_stats, d.ln_parts, d.ln_stats_ld, d.ln_colsum, d.ln_eps = _FAKE, 1, M, _FAKE, 1e-5
        if case.vt:
            d.VT, d.vt_col0, d.vt_tokens, d.vt_bs, d.vt_rs = _FAKE, 2 * K, case.tokens, K * case.tokens, case.tokens
        if case.row_stats:
            d.row_stats_out, d.row_stats_ld = _FAKE, M
    return d


def plan(case: Case, tile_cfg=None):
    """(tile, split-K, BM, BN, workgroups, parts) the library plans for the case's launch."""
    import ctypes
    from pbe_amd import lib
    d = descriptor(case, tile_cfg)
    out, need = (ctypes.c_int32 * 6)(), ctypes.c_size_t()
    fn = lib.load().pbe_conv3x3_plan if case.form == "c" else lib.load().pbe_gemm_plan
    assert fn(ctypes.byref(d), out, ctypes.byref(need)) == 0, lib.load().pbe_last_error()
    return list(out)


def case_of(key: str, value=None) -> Case:
    """The launch of a table entry (value: the table's tile | split-K << 8; default the committed table)."""
    if value is None:
        value = load_table()[key]
    case = Case(key, value)
    p = plan(case)
    if (p[0], p[1]) != (case.tile, case.splits):
        case._plain()
        p = plan(case)
    case.planned = (p[0], p[1])
    case.bm, case.bn = p[2], p[3]
    return case


# ---- sampled rows ------------------------------------------------------------------------------------------------------------------
def gemm_rows(M: int, bm: int, seed: int, n_random: int = RANDOM_ROWS):
    """Sorted row indices: the whole first and last (possibly ragged) M-tile and n_random seeded rows."""
    bm = max(1, bm)
    last0 = ((M - 1) // bm) * bm
    rows = set(range(min(bm, M))) | set(range(last0, M))
    g = torch.Generator().manual_seed(seed)
    rows |= set(torch.randint(0, M, (n_random,), generator=g).tolist())
    return sorted(rows)


def conv_rows(case: Case, seed: int, n_random: int = RANDOM_IMAGE_ROWS):
    """Sorted (sample, output row): first and last row of the first and last sample, the rows on each side of the first tile
    boundary (pixel BM - 1 | BM), seeded rows."""
    B, Ho, Wo = case.B, case.Ho, case.Wo
    sel = {(0, 0), (0, Ho - 1), (B - 1, 0), (B - 1, Ho - 1)}
    for p in (case.bm - 1, case.bm):
        if 0 <= p < B * Ho * Wo:
            sel.add((p // (Ho * Wo), (p % (Ho * Wo)) // Wo))
    g = torch.Generator().manual_seed(seed)
    for _ in range(n_random):
        sel.add((int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, Ho, (1,), generator=g))))
    return sorted(sel)


# ---- rounding model ----------------------------------------------------------------------------------------------------------------
def expect(acc, S, K, *, alpha=None, bias=None, rowvec=None, ln=None, act=0, resid=None):
    """(want, bound) in fp64 of the stored output from the fp64 product acc = A @ W^T, S = |A| @ |W|^T ([R, N]).
    alpha [N] or None; bias [N]; rowvec [R, N]; ln = (rstd [R, 1], mean [R, 1], colsum [N], eps_r [R, 1], dmean [R, 1]) with eps_r the
    relative error of rstd and dmean the error of the mean from the fp32 row statistics; resid [R, N'] (fp16 values)."""
    da = ACC_C * U32 * math.sqrt(K) * S
    if ln is None:
        pre, dpre = acc.clone(), da
    else:
        rstd, mean, colsum, eps_r, dmean = ln
        mc = mean * colsum[None, :]
        pre = rstd * (acc - mc)
        dpre = rstd * (da + 4 * U32 * (acc.abs() + mc.abs()) + dmean * colsum.abs()[None, :]) + pre.abs() * eps_r
    if alpha is not None:
        pre, dpre = pre * alpha[None, :], dpre * alpha.abs()[None, :] + 2 * U32 * (pre * alpha[None, :]).abs()
    for v in (bias[None, :] if bias is not None else None, rowvec):
        if v is not None:
            dpre = dpre + 2 * U32 * (pre.abs() + v.abs())
            pre = pre + v
    if act in (1, 2, 3):                         # SiLU / erf-GELU / quick-GELU: the slope times |d pre|, and the arm's own rounding (actref.py)
        import actref
        y = actref.act64(pre, act)
        dy = actref.ACT_DMAX[act] * dpre + actref.act_term(pre, act)
    elif act == 4:                               # interleaved (value, gate) columns
        v, gt, dv, dg = pre[:, 0::2], pre[:, 1::2], dpre[:, 0::2], dpre[:, 1::2]
        gel = gt * 0.5 * (1 + torch.erf(gt / math.sqrt(2.0)))
        y = v * gel
        dy = gel.abs() * dv + 1.13 * v.abs() * dg + GELU_FIT * v.abs() + 4 * U32 * y.abs()
    else:
        y, dy = pre, dpre
    b = dy * (1 + U16) + U16 * y.abs() + 2.0 ** -25
    if resid is None:
        return y, b
    out = y + resid
    return out, b * (1 + U16) + U16 * out.abs() + 2.0 ** -25


def clamp_to_close(want, bound, close):
    """No element's bound looser than rtol * max|ref| + atol of the op's existing _close test."""
    rtol, atol = close
    return torch.clamp(bound, max=rtol * want.abs().max().item() + atol)


class Report:
    def __init__(self, what, ratio, where, got, want, bound, n):
        self.what, self.ratio, self.where, self.got, self.want, self.bound, self.n = what, ratio, where, got, want, bound, n

    def __str__(self):
        return (f"{self.what}: worst |got - want| / bound = {self.ratio:.3g} at {self.where}: got {self.got:.6g}, want {self.want:.6g}, "
                f"bound {self.bound:.3g} ({self.n} elements)")


def compare(got, want, bound, what="", rows=None):
    """Per-element check: Report of the worst element (ratio > 1 = rejected; a non-finite value is ratio inf)."""
    got = got.double()
    d = (got - want).abs()
    r = torch.where(torch.isfinite(got), d / bound, torch.full_like(d, math.inf))
    i = int(torch.argmax(r).item())
    row, col = divmod(i, want.shape[1])
    label = rows[row] if rows is not None else row
    return Report(what, float(r.view(-1)[i]), f"row {label}, column {col}", float(got.view(-1)[i]), float(want.view(-1)[i]),
                  float(bound.view(-1)[i]), want.numel())


def check(got, want, bound, what="", rows=None) -> Report:
    rep = compare(got, want, bound, what, rows)
    assert rep.ratio <= 1.0, str(rep)
    return rep


# ---- operands and launches (GPU) ---------------------------------------------------------------------------------------------------
def _randn(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, device=dev) * scale).half()


def _zero_last_kslice(w):
    w = w.clone()
    w[..., -64:] = 0
    return w


def run_gemm(case: Case, dev, *, mutate=False):
    """Launch the case (W with its last 64-wide k-slice zeroed when mutate) and return the launch record plus what the check needs."""
    from pbe_amd import ops
    seed = seed_of(case.key)
    gen = torch.Generator(device=dev).manual_seed(seed)
    M, N, K, b = case.M, case.N, case.K, case.batch
    t = {}
    if case.form == "g8":
        cg = torch.Generator().manual_seed(seed)
        if b == 1:
            a = torch.randn(M, K, generator=cg) * torch.rand(M, 1, generator=cg) * 3
            w = torch.randn(N, K, generator=cg) / math.sqrt(K)
        else:
            a = torch.randn(M, K, generator=cg) / math.sqrt(K)          # the shared weight operand
            w = torch.randn(b * N, K, generator=cg)
        a8, sa = ops.pack_linear_f8(a)
        w8, sw = ops.pack_linear_f8(w)
        t["A"] = a8.view(torch.float8_e4m3fn).double() * sa.double()[:, None]
        t["W"] = w8.view(torch.float8_e4m3fn).double() * sw.double()[:, None]
        w8d = w8.to(dev)
        if mutate:
            w8d = w8d.clone()
            w8d[:, -64:] = 0
        if b == 1:
            bias = torch.randn(N, generator=cg)
            res = torch.randn(M, N, generator=cg).half() if case.resid else None
            t["bias"], t["resid"] = bias.double(), None if res is None else res.double()
            out = ops.gemm_f8(a8.to(dev), sa.to(dev), w8d, sw.to(dev), bias.to(dev), resid=None if res is None else res.to(dev), act=case.act)
        else:
            out = ops.gemm_f8(a8.to(dev).unsqueeze(0).expand(b, -1, -1), sa.to(dev), w8d.view(b, N, K), sw.to(dev).view(b, N))
            t["W"] = t["W"].view(b, N, K)
        t["out"] = out
        return t
    a = _randn((b, M, K) if b > 1 else (M, K), gen, dev, 1.3 if case.form == "gx" else 1.0)
    if case.offset:
        a = a.clone()
        a[::97] += LN_OFFSET
    w = _randn((N, K), gen, dev, case.wscale / math.sqrt(K))
    bias = torch.randn(N, generator=gen, device=dev) * 0.5
    t["A"], t["bias"] = a, bias
    kw = {}
    if case.ln:
        gamma = 1 + 0.1 * torch.randn(K, generator=gen, device=dev)
        beta = 0.1 * torch.randn(K, generator=gen, device=dev)
        wg, c2, c1 = ops.pack_linear_ln(w.float(), bias, gamma, beta)
        w, bias = wg, c2
        t["bias"], t["colsum"] = c2, c1
        kw["ln"] = (ops.row_stats(a), c1, 1e-5)
    t["W"] = w
    if case.resid:
        t["resid"] = _randn((M, N), gen, dev, 2.0)
        kw["resid"] = t["resid"]
    if case.rowvec:
        t["rowvec"] = _randn(((M + case.tokens - 1) // case.tokens, N), gen, dev)
        kw.update(rowvec=t["rowvec"], group_rows=case.tokens)
    wl = _zero_last_kslice(w) if mutate else w
    if b > 1:
        out = ops.gemm(a, wl.unsqueeze(0), bias, **kw)
    elif case.vt:
        qk = torch.empty((M, 2 * K), dtype=torch.float16, device=dev)
        vt = torch.empty((M // case.tokens, K, case.tokens), dtype=torch.float16, device=dev)
        ops.gemm(a, wl, bias, alpha=case.alpha, alpha_cols=case.alpha_cols, out=qk, vt=vt, vt_col0=2 * K, vt_tokens=case.tokens, **kw)
        out, t["vt_buf"] = qk, vt
    elif case.row_stats:
        out, t["stats"] = ops.gemm(a, wl, bias, act=case.act, row_stats=True, **kw)
    else:
        out = ops.gemm(a, wl, bias, act=case.act, **kw)
    t["out"] = out
    return t


def reference_gemm(case: Case, t, rows_by_batch):
    """(got, want, bound, row labels) over the sampled rows: fp64 on the host from the operands that were sent."""
    gots, wants, bounds, labels = [], [], [], []
    for bi, rows in rows_by_batch:
        ri = torch.tensor(rows, dtype=torch.long)
        A = t["A"][bi] if t["A"].dim() == 3 else t["A"]
        A = A.index_select(0, ri.to(A.device)).double().cpu()
        W = t["W"]
        W = (W[bi] if W.dim() == 3 else W).double().cpu()
        acc, S = A @ W.t(), A.abs() @ W.abs().t()
        kw = dict(act=case.act)
        if t.get("bias") is not None:
            kw["bias"] = t["bias"].double().cpu()
        if case.ln:
            mean = A.mean(1, keepdim=True)
            var = ((A - mean) ** 2).mean(1, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + 1e-5)
            eps_r = ACC_C * U32 * math.sqrt(case.K) * (A * A).mean(1, keepdim=True) / (var + 1e-5) + 8 * U32
            dmean = ACC_C * U32 * math.sqrt(case.K) * A.abs().mean(1, keepdim=True)
            kw["ln"] = (rstd, mean, t["colsum"].double().cpu(), eps_r, dmean)
        if case.alpha_cols:
            al = torch.ones(case.N, dtype=torch.float64)
            al[: case.alpha_cols] = case.alpha
            kw["alpha"] = al
        if case.rowvec:
            kw["rowvec"] = t["rowvec"].index_select(0, (ri // case.tokens).to(t["rowvec"].device)).double().cpu()
        if t.get("resid") is not None:
            kw["resid"] = t["resid"].index_select(0, ri.to(t["resid"].device)).double().cpu()
        want, bound = expect(acc, S, case.K, **kw)
        out = t["out"][bi] if t["out"].dim() == 3 else t["out"]
        got = out.index_select(0, ri.to(out.device)).double().cpu()
        if case.vt:
            T = case.tokens
            vt = t["vt_buf"]                                              # [M / T, K, T]: column 2K + c of row m at vt[m // T, c, m % T]
            got = torch.cat([got, vt[(ri // T).to(vt.device), :, (ri % T).to(vt.device)].double().cpu()], 1)
        gots.append(got), wants.append(want), bounds.append(bound)
        labels += [f"{bi}:{r}" if case.batch > 1 else r for r in rows]
    want = torch.cat(wants)
    return torch.cat(gots), want, clamp_to_close(want, torch.cat(bounds), case.close), labels


def run_conv(case: Case, dev, *, mutate=False):
    from pbe_amd import ops
    gen = torch.Generator(device=dev).manual_seed(seed_of(case.key))
    B, H, W, C1, C2, Co = case.B, case.H, case.W, case.C1, case.C2, case.Cout
    t = {"x1": _randn((B, H, W, C1), gen, dev), "x2": _randn((B, H, W, C2), gen, dev) if C2 else None}
    w = torch.randn(Co, C1 + C2, 3, 3, generator=gen, device=dev) * (case.wscale / math.sqrt(9 * (C1 + C2)))
    bias = torch.randn(Co, generator=gen, device=dev) * 0.5
    t["bias"] = bias
    kw = {"act": case.act} if case.act else {}
    if case.ups == 2:
        wp = ops.pack_conv3x3_up_phases(w)                               # [4, Co, 4 * C1], the fp16 weights sent
        t["wp"] = wp
        if mutate:
            wp = wp.view(4, Co, C1 // 64, 4, 64).clone()
            wp[:, :, -1] = 0
            wp = wp.view(4, Co, 4 * C1)
        out = ops.conv3x3(t["x1"], wp, bias, upsample=True)
    else:
        w = w.half()
        t["w"] = w
        wm = w.clone() if mutate else w
        if mutate:                               # the last input-channel block (of the second source when there is one)
            wm[:, -64:] = 0
        wp = ops.pack_conv3x3(wm.float(), split=(C1, C2) if C2 else None)
        if case.rowvec:
            t["rowvec"] = _randn((B, Co), gen, dev, 0.5)
            kw["rowvec"] = t["rowvec"]
        if case.resid:
            t["resid"] = _randn((B, case.Ho, case.Wo, Co), gen, dev)
            kw["resid"] = t["resid"]
        if case.group_stats:
            kw["group_stats"] = case.group_stats
        t["kw"], t["wpacked"] = kw, wp
        out = ops.conv3x3(t["x1"], wp, bias, x2=t["x2"], stride=case.stride, pad=case.pad, upsample=bool(case.ups), **kw)
    t["out"] = out
    return t


def _vrow(x, b, r, case):
    """Row r of the virtual (upsampled when ups == 1) input of sample b, zero outside the image: [C, Wv] fp64 on the host."""
    hv = 2 * case.H if case.ups == 1 else case.H
    C = x.shape[-1]
    wv = 2 * case.W if case.ups == 1 else case.W
    if r < 0 or r >= hv:
        return torch.zeros(C, wv, dtype=torch.float64)
    row = x[b, r // 2 if case.ups == 1 else r].double().cpu().t()        # [C, W]
    return row.repeat_interleave(2, 1) if case.ups == 1 else row


def _unpack_phases(wp, C1):
    """pack_conv3x3_up_phases output [4, Co, 4 C1] -> per phase (py, px) a [Co, C1, 2, 2] fp64 weight (ty, tx)."""
    Co = wp.shape[1]
    w = wp.double().cpu().view(4, Co, C1 // 64, 2, 2, 64).permute(0, 1, 2, 5, 3, 4).reshape(4, Co, C1, 2, 2)
    return w


def reference_conv(case: Case, t, sel):
    """(got, want, bound, labels) over whole sampled output rows [rows * Wo, Co]."""
    crops = []
    for b, oy in sel:
        if case.ups == 2:
            y, py = divmod(oy, 2)
            rows = [y - 1 + py + ty for ty in (0, 1)]
            src = t["x1"]
            crops.append(torch.stack([_vrow(src, b, r, case) for r in rows], 1))   # [C, 2, W]
        else:
            base = oy * case.stride - (1 if case.pad else 0)
            parts = []
            for src in ([t["x1"]] if t["x2"] is None else [t["x1"], t["x2"]]):
                parts.append(torch.stack([_vrow(src, b, base + ky, case) for ky in range(3)], 1))
            crops.append(torch.cat(parts, 0))                             # [C1 + C2, 3, Wv]
    X = torch.stack(crops, 0)
    Co, Wo = case.Cout, case.Wo
    if case.ups == 2:
        wph = _unpack_phases(t["wp"], case.C1)
        Xp = F.pad(X, (1, 1))                                              # source column j at j + 1
        acc = torch.empty(X.shape[0], Co, 2 * case.W, dtype=torch.float64)
        S = torch.empty_like(acc)
        for i, (b, oy) in enumerate(sel):
            py = oy % 2
            for px in (0, 1):
                xi = Xp[i:i + 1, :, :, px:px + case.W + 1]
                wi = wph[2 * py + px]
                acc[i, :, px::2] = F.conv2d(xi, wi)[0, :, 0]
                S[i, :, px::2] = F.conv2d(xi.abs(), wi.abs())[0, :, 0]
    else:
        w = t["w"].double().cpu()
        if case.pad:
            acc, S = (F.conv2d(X, w, stride=(1, case.stride), padding=(0, 1)), F.conv2d(X.abs(), w.abs(), stride=(1, case.stride), padding=(0, 1)))
        else:
            Xq = F.pad(X, (0, 1))
            acc, S = F.conv2d(Xq, w, stride=(1, case.stride)), F.conv2d(Xq.abs(), w.abs(), stride=(1, case.stride))
        acc, S = acc[:, :, 0], S[:, :, 0]
    # [R, Co, Wo] -> [R * Wo, Co]
    acc = acc.permute(0, 2, 1).reshape(-1, Co)
    S = S.permute(0, 2, 1).reshape(-1, Co)
    bidx = torch.tensor([b for b, _ in sel for _ in range(Wo)])
    kw = dict(bias=t["bias"].double().cpu(), act=case.act)
    if t.get("rowvec") is not None:
        kw["rowvec"] = t["rowvec"].double().cpu()[bidx]
    if t.get("resid") is not None:
        kw["resid"] = torch.cat([t["resid"][b, oy].double().cpu() for b, oy in sel])
    want, bound = expect(acc, S, case.K, **kw)
    got = torch.cat([t["out"][b, oy].double().cpu() for b, oy in sel])
    labels = [f"{b}:{oy}:{ox}" for b, oy in sel for ox in range(Wo)]
    return got, want, clamp_to_close(want, bound, case.close), labels


# ---- one table entry end to end (GPU) ----------------------------------------------------------------------------------------------
def run_case(case: Case, dev, *, mutate=False):
    return run_conv(case, dev, mutate=mutate) if case.form == "c" else run_gemm(case, dev, mutate=mutate)


def sampled(case: Case, t, bm: int):
    """(got, want, bound, labels) of the sampled output rows for the planned BM."""
    seed = seed_of(case.key)
    if case.form == "c":
        case.bm = bm
        return reference_conv(case, t, conv_rows(case, seed))
    rows = gemm_rows(case.M, bm, seed)
    batches = [(0, rows)] + ([(case.batch - 1, rows)] if case.batch > 1 else [])
    return reference_gemm(case, t, batches)


def sensitivity_key(table, form: str) -> str:
    """The entry of a form the sensitivity test mutates: the smallest launch with split-K if the form has one, else the smallest."""
    def work(k):
        c = Case(k, table[k])
        if c.form == "c":
            return c.B * c.Ho * c.Wo * c.Cout * c.K
        return c.M * c.N * c.K * c.batch
    keys = [k for k in table if k.split(":")[0] == form and Case(k, table[k]).K > 64]
    split = [k for k in keys if table[k] >> 8 > 1]
    return min(split or keys, key=work)
