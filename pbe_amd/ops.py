"""Tensor-level wrappers over the C-ABI (include/pbe_hip.h): the model and sampler path (GEMM / conv launches, norms, attention, the
MX-fp8 forms, sampler updates, noise, weight packing).  The wrappers around uint8 pictures and masks live in ops_picture.py and are
re-exported at the end of this file, so every wrapper is ``ops.X``; opsbase.py holds what both modules share.

torch is used for device memory and the current HIP stream only; every arithmetic step is a
kernel of libpbe_hip.so.  All wrappers raise if handed CPU tensors — there is no fallback.
Activations are fp16; ``[B, H, W, C]`` / ``[rows, C]`` (channels last, contiguous).
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Tuple

import torch

from . import lib as _l
from .opsbase import _f, _h, _p, _req, _stream, _ws, workspace  # noqa: F401  (ops._ws is the one scratch dict: tests poison it by key)

ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU, ACT_GEGLU = 0, 1, 2, 3, 4
SPLITK_WS_BYTES = 64 << 20

# ---- per-shape tile choice measured on MI355X (tools/autotune.py writes the table) -------------
import json as _json
import os as _os

_TUNED_PATH = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "tuned_mi355x.json")
try:
    if _os.environ.get("PBE_NO_TUNED"):          # evaluate the built-in heuristic (tools / tests only)
        raise OSError("tuned table disabled by PBE_NO_TUNED")
    with open(_TUNED_PATH) as _tuned_file:
        _TUNED = _json.load(_tuned_file)
except (OSError, ValueError):
    _TUNED = {}
_RECORD = None            # set to a dict by tools/autotune.py to collect the shapes a workload uses
_PLANS = None             # set to a list by tools/layer_diff.py: (key, tile config, split-K factor, BM, BN, workgroups) per GEMM / conv launch
_PIN_SCALE = 1            # see pinned_batch_scale
_PIN_CACHE = {}           # the tile decisions of _tile that take a plan query (pinned_batch_scale, MX-fp8 tile rule)
_PIN_MISSES = []         # (key, tile, split-K planned at the scaled batch, tile, split-K the sub-batch launch takes instead)


class pinned_batch_scale:
    """Inside this context every GEMM / conv is launched with the tile config and split-K factor the library would pick for
    the SAME layer at `scale` times the batch.  The k order of a tile does not depend on the tile shape; only the split-K
    factor changes the fp32 summation order, so a sub-batch evaluated this way reproduces the bits of the full batch
    (used by the shared guidance prefix: B samples evaluated once must equal the 2B duplicated evaluation)."""

    def __init__(self, scale: int):
        self.scale = int(scale)

    def __enter__(self):
        global _PIN_SCALE
        self.prev, _PIN_SCALE = _PIN_SCALE, self.scale

    def __exit__(self, *exc):
        global _PIN_SCALE
        _PIN_SCALE = self.prev
        return False


_TIMES = None             # set to a dict by tools/shape_profile.py: key -> [(start event, end event), ...] around each launch


class _timed:
    """Bracket one launch with events when shape profiling is on (no-op otherwise)."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        if _TIMES is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _TIMES is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _TIMES.setdefault(self.key, []).append((self.e0, e1))
        return False


_FORCE_CFG = None         # set by tools/autotune_insitu.py: every GEMM / conv launch takes this tile_cfg (A/B inside the real sampler)


def _tile_cfg(key: str) -> int:
    if _RECORD is not None:
        _RECORD[key] = _RECORD.get(key, 0) + 1
    if _FORCE_CFG is not None:
        return int(_FORCE_CFG)
    return int(_TUNED.get(key, -1))


# ---- tiled launches, kind "gemm" / "batch" (2-D / 3-D strided batch pbe_gemm_f16), "conv" (pbe_conv3x3_f16), "mx8" (pbe_gemm_mx8out_f16),
#      "gn" (pbe_gemm_gnfold_f16); mx = the second descriptor of the last two ----
def _key(kind: str, d, stats: bool = False) -> str:
    """Shape key of a launch (tuned table, _RECORD, _PLANS); stats: the GEMM also writes row statistics (row_stats_out is set later)."""
    if kind == "conv":
        return f"c:{d.B}:{d.H}:{d.W}:{d.C1}:{d.C2}:{d.Cout}:{d.stride}:{d.pad}:{d.upsample}"
    ex = stats or d.alpha_cols or d.ln_stats or d.VT                # the extended-epilogue tiles are tuned under their own keys
    return f"{'g8' if d.operand_dtype else 'gx' if ex else 'g'}:{d.M}:{d.N}:{d.K}:{d.batch}"


def _plan(kind: str, d, mx=None) -> list:
    """Host-only plan query: [tile config, split-K factor, BM, BN, workgroups, column tiles]; raises where the library refuses."""
    out, lib = (C.c_int32 * 6)(), _l.load()
    if kind == "mx8":
        rc = lib.pbe_gemm_mx8out_plan(C.byref(d), C.byref(mx), out)
    elif kind == "gn":
        rc = lib.pbe_gemm_gnfold_plan(C.byref(d), C.byref(mx), out)
    else:
        rc = (lib.pbe_conv3x3_plan if kind == "conv" else lib.pbe_gemm_plan)(C.byref(d), out, C.byref(C.c_size_t()))
    _l.check(rc, f"plan ({kind})")
    return list(out)


@functools.lru_cache(maxsize=None)
def _layout(cls):
    """Masks over a descriptor type's bits, nested ranges included: (all but bits 4..63 of each pointer, those bits, the bit after each)."""
    def ptrs(t, base):
        for f, ft in t._fields_:
            o = base + getattr(t, f).offset
            if issubclass(ft, C.Array):
                yield from (p for i in range(ft._length_) for p in ptrs(ft._type_, o + i * C.sizeof(ft._type_)))
            elif ft is C.c_void_p:
                yield o
    offs = list(ptrs(cls, 0))
    hi = sum((2 ** 64 - 16) << 8 * o for o in offs)
    return (1 << 8 * C.sizeof(cls)) - 1 - hi, hi, sum(1 << 8 * o + 64 for o in offs)


def _desc_key(d):
    """A descriptor as a planner can read it: every field, each pointer reduced to its address mod 16 and whether it is null, i.e. below 16
    (adding bits 4..63 of a pointer to themselves carries out of the pointer exactly where they are not all zero)."""
    keep, hi, after = _layout(type(d))
    x = int.from_bytes(d, "little")
    return x & keep, ((x & hi) + hi) & after


def _mx8_tile(d, mx, cfg: int) -> int:
    """cfg where the MX copy-out of d takes it, else -1: a tile that splits an MX block is refused when requested, -1 plans an aligned one."""
    t = type(d).from_buffer_copy(d)
    t.tile_cfg = cfg
    try:
        _plan("mx8", t, mx)
        return cfg
    except _l.PbeError:
        return -1


def _pinned(kind: str, d, mx=None, stats: bool = False) -> int:
    """tile_cfg under pinned_batch_scale: the tile and split-K factor planned for the launch at _PIN_SCALE times the batch - M of a 2-D GEMM
    (statistics planes as long as its rows), the batch count of a strided batch, B of a conv, M and every range's B of an MX copy-out (MX
    rule applied).  A launch that cannot take that pair, or whose row-statistics partials come from column tiles of another width (other
    fp32 summation order, still correct) is recorded in _PIN_MISSES and warned."""
    s, big = _PIN_SCALE, type(d).from_buffer_copy(d)
    bmx = None if mx is None else type(mx).from_buffer_copy(mx)
    if kind == "conv":
        big.B *= s
    elif kind == "batch":
        big.batch *= s
    else:
        big.M *= s
        if big.ln_stats:
            big.ln_stats_ld = max(big.ln_stats_ld, big.M)
        if big.row_stats_out:
            big.row_stats_ld = max(big.row_stats_ld, big.M)
        for i in range(bmx.nranges if kind == "mx8" else 0):
            bmx.r[i].B *= s
    key = _key(kind, big, stats)
    big.tile_cfg = int(_FORCE_CFG) if _FORCE_CFG is not None else int(_TUNED.get(key, -1))
    if kind == "mx8":
        big.tile_cfg = _mx8_tile(big, bmx, big.tile_cfg)
    pl = _plan(kind, big, bmx)
    hit = pl[0] | (max(1, pl[1]) << 8)
    small = type(d).from_buffer_copy(d)
    small.tile_cfg = hit
    got = _plan(kind, small, mx)
    if got[1] != max(1, pl[1]) or (kind in ("gemm", "gn") and small.row_stats_out and got[3] != pl[3]):      # (row statistics: one partial per column tile of BN)
        import warnings
        _PIN_MISSES.append((key, pl[0], pl[1], got[0], got[1]))
        warnings.warn(f"pinned_batch_scale({s}): {key} plans tile {pl[0]} / split-K {pl[1]} at the scaled batch but the "
                      f"sub-batch launch runs tile {got[0]} / split-K {got[1]} (different fp32 summation order)")
    return hit


def _tile(kind: str, d, key: str, mx=None, stats: bool = False) -> int:
    """tile_cfg of a launch: `key`'s forced or tuned tile (counted in _RECORD), under the MX rule (_mx8_tile), or pinned (_pinned; not fp8
    operands, which never split K).  Decisions that take plan queries are cached per shape key, descriptor, forced tile and scale."""
    cfg = _tile_cfg(key)
    pin = _PIN_SCALE != 1 and (kind == "conv" or not d.operand_dtype)
    if not pin and (kind != "mx8" or cfg < 0):
        return cfg
    ck = (key, cfg, _FORCE_CFG, _PIN_SCALE if pin else 1, _desc_key(d), None if mx is None else _desc_key(mx))
    hit = _PIN_CACHE.get(ck)
    if hit is None:
        hit = _PIN_CACHE[ck] = _pinned(kind, d, mx, stats) if pin else _mx8_tile(d, mx, cfg)
    return hit


def _mx8_tile_cfg(d, mx, key: str, D: int) -> int:
    """_tile of an MX copy-out outside pinned_batch_scale (D, the head dim, is that of mx's ranges)."""
    with pinned_batch_scale(1):
        return _tile("mx8", d, key, mx)


def _launch(kind: str, d, mx=None, row_stats=None):
    """Launch a filled descriptor (but for tile_cfg: _tile).  row_stats (GEMM): called with the planned column-tile count once the tile is
    settled, returns the RowStats the epilogue fills; _launch returns it.  The row-statistics form is set BEFORE the tile is chosen: every
    plan query of _tile / _pinned (and the _PIN_CACHE key) then sees the extended-epilogue problem that launches, not a plain dense one."""
    if row_stats is not None:
        d.row_stats_out, d.row_stats_ld = 8, 0  # (any non-null value: the plans only need to know the form)
    key = _key(kind, d, row_stats is not None)
    d.tile_cfg = _tile(kind, d, key, mx, row_stats is not None)
    stats = None
    if row_stats is not None:                   # one partial per column tile of the plan this launch will take
        stats = row_stats(_plan(kind, d, mx)[5])
        d.row_stats_out, d.row_stats_ld = stats.ptr(), stats.ld
    if _PLANS is not None:
        _PLANS.append((key, *_plan(kind, d, mx)[:5]))
    if _TIMES is not None:                      # the _TIMES key: shape key + epilogue form
        key += "" if kind == "conv" else "|mx8" if kind == "mx8" else \
            f"|a{d.act}{'r' * bool(d.resid)}{'v' * bool(d.rowvec)}{'L' * bool(d.ln_stats)}{'S' * (stats is not None)}{'T' * bool(d.VT)}{'G' * (kind == 'gn')}"
    with _timed(key):
        if kind == "mx8":
            _l.check(_l.load().pbe_gemm_mx8out_f16(C.byref(d), C.byref(mx), _stream()), "pbe_gemm_mx8out_f16")
        elif kind == "gn":
            _l.check(_l.load().pbe_gemm_gnfold_f16(C.byref(d), C.byref(mx), _stream()), "pbe_gemm_gnfold_f16")
        elif kind == "conv":
            _l.check(_l.load().pbe_conv3x3_f16(C.byref(d), _stream()), "pbe_conv3x3_f16")
        else:
            _l.check(_l.load().pbe_gemm_f16(C.byref(d), _stream()), "pbe_gemm_f16")
    return stats


@functools.lru_cache(maxsize=None)
def qkv_fusable(inner: int, tokens: int = 8) -> bool:
    """Can the fused q | k | V^T projection (gemm(..., vt=..., vt_col0=2 * inner) with N = 3 * inner) run at this inner width and this
    many tokens per sample?  Asked of the library's planner on a stand-in descriptor (host only, nothing is launched): the V^T columns
    must start on a column tile, so 2 * inner has to be a multiple of some extended-epilogue tile width - pbe_gemm_plan refuses the rest."""
    fake = 1 << 20                               # 16-byte aligned stand-in address, never read
    d = _l.GemmDesc(fake, None, fake, fake, None, None, None, tokens, 3 * inner, 8, 8, 8, 0, 8, 2 * inner, 0, 0, 0, 0, 0, 0, 0, 1, 1.0, 0, 0,
                    None, 0, -1)
    d.alpha_cols, d.VT, d.vt_col0, d.vt_tokens, d.vt_bs, d.vt_rs = inner, fake, 2 * inner, tokens, inner * tokens, tokens
    try:
        _plan("gemm", d)
        return True
    except _l.PbeError:
        return False


def _splitk_ws(device):
    """Per-device scratch for split-K partial sums (fp32 slabs); ops on one stream run in order, so one buffer is enough."""
    return workspace(device, "splitk", SPLITK_WS_BYTES)


def _rows(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """(rows, cols, ld) of a 2-D view whose last dim is contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise _l.PbeError(f"{what}: expected a 2-D tensor with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


# ---------------------------------------------------------------------------------------------
class RowStats:
    """Partial (sum, sum of squares) of every row of a [M, C] tensor: `buf` fp32 [parts, ld, 2], as a GEMM epilogue (row_stats=True)
    or pbe_row_stats_f16 wrote them; what a LayerNorm-folding GEMM consumes (ln=...)."""
    __slots__ = ("buf", "parts", "ld", "row0")

    def __init__(self, buf, parts, ld, row0=0):
        self.buf, self.parts, self.ld, self.row0 = buf, parts, ld, row0

    def ptr(self) -> int:
        return self.buf.data_ptr() + 8 * self.row0


def row_stats(x: torch.Tensor) -> RowStats:
    """One-partial row statistics of a contiguous-row fp16 [M, C] tensor (the fallback when x's producer did not emit them)."""
    _h(x, "row_stats x")
    M, Cc, ldx = _rows(x, "row_stats x")
    buf = torch.empty((1, M, 2), dtype=torch.float32, device=x.device)
    with _timed(f"rs:{M}:{Cc}"):
        _l.check(_l.load().pbe_row_stats_f16(_p(x), _p(buf), M, Cc, ldx, _stream()), "pbe_row_stats_f16")
    return RowStats(buf, 1, M)


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, a2: Optional[torch.Tensor] = None,
         rowvec: Optional[torch.Tensor] = None, group_rows: int = 0, resid: Optional[torch.Tensor] = None, act: int = ACT_NONE,
         alpha: float = 1.0, bias_per_row: bool = False, out: Optional[torch.Tensor] = None, alpha_cols: int = 0, ln=None,
         row_stats=False, vt: Optional[torch.Tensor] = None, vt_col0: int = 0, vt_tokens: int = 0, gn=None):
    """out[m, n] = act(alpha * sum_k [a | a2][m, k] w[n, k] + bias + rowvec[m // group_rows, n]) + resid[m, n].
    2-D operands, or 3-D [batch, rows, cols] for a strided batch (w may have batch 1).

    Extended epilogue (2-D operands; include/pbe_hip.h, pbe_gemm_desc): alpha_cols = alpha on columns < alpha_cols only;
    ln = (RowStats of a's rows, colsum fp32 [N], eps): LayerNorm(a) is folded in (w = W * gamma, bias = W beta + b);
    row_stats = True (or a RowStats to fill, e.g. a slice of a shared buffer): also returns the RowStats of the output rows -> (out, stats);
    vt [B, N - vt_col0, >= vt_tokens]: columns >= vt_col0 are written transposed there (V^T), `out` then has vt_col0 columns.
    gn = (GroupStats of a's tensor, gamma, beta, eps[, tokens per sample]): a holds RAW rows and the result is that of
    gemm(GroupNorm(a), ...), bit for bit - folded into the A operand (pbe_gemm_gnfold_f16) where a tile's rows divide a sample's tokens
    (default: M / samples), else by the separate normalisation pass."""
    _h(a, "gemm a"); _h(w, "gemm w")
    fold = None
    if gn is not None:
        if a.dim() != 2 or a2 is not None or ln is not None or vt is not None or alpha_cols or act == ACT_GEGLU:
            raise _l.PbeError("gemm: gn takes a 2-D problem with one source and no LayerNorm fold, V^T, column alpha or GEGLU")
        gst, g_gamma, g_beta, g_eps = gn[:4]
        g_tok = int(gn[4]) if len(gn) > 4 else a.shape[0] // gst.batch
        _f(g_gamma, "gemm gn gamma"); _f(g_beta, "gemm gn beta")
        if not a.is_contiguous() or g_tok <= 0 or a.shape[0] > gst.batch * g_tok or g_gamma.numel() != a.shape[1] or g_beta.numel() != a.shape[1]:
            raise _l.PbeError("gemm: gn needs contiguous rows of the statistics' samples and affine vectors of a's width")
        fold = _l.GnFoldDesc(0, 2 * a.shape[1], g_tok)
    batch = 1
    sA = sW = sC = sR = 0
    if a.dim() == 3:
        batch = a.shape[0]
        if a.stride(2) != 1 or w.dim() != 3 or w.stride(2) != 1 or w.shape[0] not in (1, batch):
            raise _l.PbeError("gemm: bad batched operands")
        M, K, lda, sA = a.shape[1], a.shape[2], a.stride(1), a.stride(0)
        N, Kw, ldw = w.shape[1], w.shape[2], w.stride(1)
        sW = w.stride(0) if w.shape[0] == batch else 0
        if out is None:
            out = torch.empty((batch, M, N), dtype=torch.float16, device=a.device)
        ldc, sC = out.stride(1), out.stride(0)
        ldr = 0
        if resid is not None:
            _h(resid, "gemm resid")
            ldr = resid.stride(-2)
            sR = resid.stride(0) if (resid.dim() == 3 and resid.shape[0] == batch) else 0
    else:
        M, K, lda = _rows(a, "gemm a")
        N, Kw, ldw = _rows(w, "gemm w")
        if out is None:
            out = torch.empty((M, vt_col0 if vt is not None else (N // 2 if act == ACT_GEGLU else N)), dtype=torch.float16, device=a.device)
        ldc = _rows(out, "gemm out")[2]
        ldr = 0
        if resid is not None:
            ldr = _rows(_h(resid, "gemm resid"), "gemm resid")[2]
    K1, lda2 = K, 0
    if a2 is not None:
        _, K2, lda2 = _rows(_h(a2, "gemm a2"), "gemm a2")
        K = K1 + K2
    if Kw != K:
        raise _l.PbeError(f"gemm: K mismatch, activations {K} vs weights {Kw}")
    if bias is not None:
        _f(bias, "gemm bias")
        if bias.numel() != (M if bias_per_row else N):
            raise _l.PbeError("gemm: bias length mismatch")
    ldv = 0
    if rowvec is not None:
        _h(rowvec, "gemm rowvec")
        ldv = rowvec.stride(0) if rowvec.dim() == 2 else 0
        if group_rows <= 0:
            raise _l.PbeError("gemm: rowvec needs group_rows")
    d = _l.GemmDesc(_p(a), _p(a2), _p(w), _p(_h(out, "gemm out")), _p(bias), _p(rowvec), _p(resid), M, N, K, K1, lda, lda2, ldw, ldc, ldr,
                    ldv, group_rows, sA, sW, sC, sR, batch, float(alpha), act, 1 if bias_per_row else 0,
                    _splitk_ws(a.device).data_ptr(), SPLITK_WS_BYTES, -1)
    if alpha_cols or ln is not None or row_stats is not False or vt is not None:
        if a.dim() != 2:
            raise _l.PbeError("gemm: the extended epilogue takes 2-D operands")
        d.alpha_cols = int(alpha_cols)
        if ln is not None:
            st, colsum, eps = ln
            _f(colsum, "gemm ln colsum")
            if colsum.numel() != N or st.ld - st.row0 < M:
                raise _l.PbeError("gemm: LayerNorm fold needs colsum [N] and row statistics for every row of a")
            d.ln_stats, d.ln_parts, d.ln_stats_ld, d.ln_colsum, d.ln_eps = st.ptr(), st.parts, st.ld, _p(colsum), float(eps)
        if vt is not None:
            _h(vt, "gemm vt")
            if vt.dim() != 3 or vt.stride(2) != 1 or vt.shape[1] != N - vt_col0 or vt.shape[0] * vt_tokens != M:
                raise _l.PbeError(f"gemm: vt must be [M / vt_tokens, N - vt_col0, >= vt_tokens], got {tuple(vt.shape)}")
            d.VT, d.vt_col0, d.vt_tokens, d.vt_bs, d.vt_rs = _p(vt), int(vt_col0), int(vt_tokens), vt.stride(0), vt.stride(1)

    def fill(parts):                            # the RowStats of the output rows, `parts` partials
        if not isinstance(row_stats, RowStats):
            return RowStats(torch.empty((parts, M, 2), dtype=torch.float32, device=a.device), parts, M)
        if row_stats.parts < parts:
            raise _l.PbeError(f"gemm: row_stats buffer holds {row_stats.parts} partials, the plan writes {parts}")
        return RowStats(row_stats.buf, parts, row_stats.ld, row_stats.row0)
    if fold is not None:
        Cc = a.shape[1]
        d.tile_cfg, fold.table = -1, 16
        if row_stats is not False:
            d.row_stats_out = 8
        try:                                    # eligible?  (host-only plan query on the form that would launch)
            _plan("gn", d, fold)
        except _l.PbeError:
            fold = None
        d.row_stats_out = None
        if fold is None:                        # the separate normalisation pass, then the plain launch
            if M != gst.batch * g_tok:
                raise _l.PbeError("gemm: gn without the fold needs every row of the statistics' samples")
            a = _groupnorm_apply(a, gst, g_gamma, g_beta, g_eps, False)      # (bound to `a`: alive until the launch is queued)
            d.A = _p(a)
        else:
            table = torch.empty((gst.batch, 2 * Cc), dtype=torch.float32, device=a.device)
            with _timed(f"nt:{gst.batch}:{g_tok}:{Cc}"):
                _l.check(_l.load().pbe_groupnorm_table_f32(_p(gst.buf), gst.blocks, _p(g_gamma), _p(g_beta), _p(table), gst.batch, g_tok, Cc, gst.groups,
                                                           float(g_eps), _stream()), "pbe_groupnorm_table_f32")
            fold.table = table.data_ptr()
    stats = _launch("gn" if fold is not None else "batch" if a.dim() == 3 else "gemm", d, mx=fold, row_stats=None if row_stats is False else fill)
    return (out, stats) if row_stats is not False else out


def conv_out_hw(h: int, w: int, stride: int, pad: int, upsample: bool) -> Tuple[int, int]:
    hv, wv = (h * 2, w * 2) if upsample else (h, w)
    extra = 2 if pad else 1
    return (hv + extra - 3) // stride + 1, (wv + extra - 3) // stride + 1


def conv3x3(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], *, x2: Optional[torch.Tensor] = None,
            rowvec: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, stride: int = 1, pad: int = 1,
            upsample: bool = False, act: int = ACT_NONE, group_stats: int = 0) -> torch.Tensor:
    """NHWC 3x3 conv on the matrix cores; ``wp`` is the packed [Cout, 9*Cin] weight (pack_conv3x3).
    group_stats = G > 0: the output feeds a GroupNorm(G) - where the planned tile can, the copy-out also leaves the norm's partial
    statistics (include/pbe_hip.h, group_stats_out) and the returned tensor carries them (`_pbe_gstats`); ops.groupnorm then runs its
    normalisation pass only."""
    _h(x, "conv3x3 x"); _h(wp, "conv3x3 w")
    if x.dim() != 4 or not x.is_contiguous():
        raise _l.PbeError("conv3x3: x must be a contiguous [B,H,W,C] tensor")
    B, H, W, C1 = x.shape
    C2 = ldv = 0
    phase = wp.dim() == 3                        # pack_conv3x3_up_phases: the upsampling conv as four 2x2 convs on the source grid (4 / 9 of the MACs)
    if phase:
        if not upsample or x2 is not None or resid is not None or rowvec is not None or stride != 1 or pad != 1:
            raise _l.PbeError("conv3x3: phase-packed weights are for the plain nearest-2x upsampling conv")
        if wp.shape[0] != 4 or not wp.is_contiguous() or wp.shape[2] != 4 * C1:
            raise _l.PbeError(f"conv3x3: phase-packed weight must be [4, Cout, {4 * C1}], got {tuple(wp.shape)}")
        Cout = wp.shape[1]
    else:
        if x2 is not None:
            _h(x2, "conv3x3 x2")
            if x2.dim() != 4 or not x2.is_contiguous() or x2.shape[:3] != x.shape[:3]:
                raise _l.PbeError("conv3x3: x2 must match x in [B,H,W]")
            C2 = x2.shape[3]
        Cout = wp.shape[0]
        if wp.dim() != 2 or not wp.is_contiguous() or wp.shape[1] != 9 * (C1 + C2):
            raise _l.PbeError(f"conv3x3: packed weight must be [Cout, {9 * (C1 + C2)}], got {tuple(wp.shape)}")
    Ho, Wo = conv_out_hw(H, W, stride, pad, upsample)
    y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float16, device=x.device)
    if rowvec is not None:
        _h(rowvec, "conv3x3 rowvec")
        if rowvec.dim() != 2 or rowvec.shape[0] != B or rowvec.stride(1) != 1:
            raise _l.PbeError("conv3x3: rowvec must be [B, >=Cout] with unit inner stride")
        ldv = rowvec.stride(0)
    if resid is not None:
        _h(resid, "conv3x3 resid")
        if tuple(resid.shape) != tuple(y.shape) or not resid.is_contiguous():
            raise _l.PbeError("conv3x3: resid must match the output shape")
    if bias is not None:
        _f(bias, "conv3x3 bias")
    d = _l.Conv3x3Desc(_p(x), _p(x2), _p(wp), _p(y), _p(bias), _p(rowvec), _p(resid), B, H, W, C1, C2, Cout, stride, pad,
                       2 if phase else int(bool(upsample)), ldv, act, _splitk_ws(x.device).data_ptr(), SPLITK_WS_BYTES, -1, conv_kblock(C1, C2))
    gs_buf = gs_blocks = None
    if group_stats > 0 and USE_CONV_GROUP_STATS and not phase and Cout % group_stats == 0 and Ho * Wo >= 64:
        gs_buf = torch.empty((B, (Ho * Wo) // 64, group_stats, 2), dtype=torch.float32, device=x.device)       # room for the smallest row block (64)
        gs_blocks = C.c_int32(0)
        d.group_stats_out, d.group_stats_groups, d.group_stats_blocks = gs_buf.data_ptr(), group_stats, C.cast(C.pointer(gs_blocks), C.c_void_p)
    _launch("conv", d)
    if gs_blocks is not None and gs_blocks.value > 0:
        y._pbe_gstats = GroupStats(gs_buf, B, int(gs_blocks.value), group_stats, y._version)
    return y


def conv3x3_small(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], *, stride: int = 1, pad: int = 1,
                  act: int = ACT_NONE, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 conv for tiny Cin (channel-padded NHWC input, Cp in {8,16}): im2col + GEMM."""
    _h(x, "conv3x3_small x")
    B, H, W, Cp = x.shape
    Ho, Wo = conv_out_hw(H, W, stride, pad, False)
    cols = torch.empty((B * Ho * Wo, 9 * Cp), dtype=torch.float16, device=x.device)
    _l.check(_l.load().pbe_im2col3x3_f16(_p(x), _p(cols), B, H, W, Cp, stride, pad, _stream()), "pbe_im2col3x3_f16")
    y = gemm(cols, wp, bias, act=act, resid=None if resid is None else resid.reshape(B * Ho * Wo, -1))
    return y.view(B, Ho, Wo, wp.shape[0])


USE_CONV_GROUP_STATS = True      # conv3x3(group_stats=G): let the conv's copy-out produce the following GroupNorm's statistics (tools flip it for A/B)


class GroupStats:
    """Partial (sum, sumsq) per (sample, row block, group) of a conv output, written by the conv's copy-out: the first B * blocks * groups * 2
    floats of `buf`, laid out [B][blocks][groups][2] (pbe_groupnorm_f16's partial layout)."""
    __slots__ = ("buf", "blocks", "groups", "batch", "version")

    def __init__(self, buf, batch, blocks, groups, version):
        self.buf, self.batch, self.blocks, self.groups, self.version = buf, batch, blocks, groups, version      # version: the tensor's _version when written

    def view(self):
        return self.buf.view(-1)[: self.batch * self.blocks * self.groups * 2].view(self.batch, self.blocks, self.groups, 2)


def group_stats_of(x: torch.Tensor, groups: int = 32) -> Optional[GroupStats]:
    """The statistics x's producing conv left on it (conv3x3(group_stats=G)) while they still describe it, else None."""
    st = getattr(x, "_pbe_gstats", None)
    ok = st is not None and st.groups == groups and st.batch == x.shape[0] and st.version == x._version      # (an in-place edit since the conv voids them)
    return st if ok else None


def _groupnorm_apply(x, st, gamma, beta, eps, silu):
    """The normalisation pass alone, from a producer's statistics (one read, one write): x holds st.batch whole samples, channels last."""
    B, C1 = st.batch, x.shape[-1]
    HW = x.numel() // (B * C1)
    y = torch.empty_like(x)
    with _timed(f"n:{B}:{HW}:{C1}:0"):
        _l.check(_l.load().pbe_groupnorm_apply_f16(_p(x), _p(st.buf), st.blocks, _p(gamma), _p(beta), _p(y), B, HW, C1, st.groups, float(eps),
                                                   1 if silu else 0, _stream()), "pbe_groupnorm_apply_f16")
    return y


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, silu: bool, *, x2: Optional[torch.Tensor] = None,
              groups: int = 32) -> torch.Tensor:
    """GroupNorm(+SiLU) of NHWC x (optionally the channel concat x | x2); output has C1+C2 channels."""
    _h(x, "groupnorm x"); _f(gamma, "groupnorm gamma"); _f(beta, "groupnorm beta")
    if not x.is_contiguous():
        raise _l.PbeError("groupnorm: x must be contiguous")
    B, C1 = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C1)
    C2 = 0
    if x2 is not None:
        _h(x2, "groupnorm x2")
        C2 = x2.shape[-1]
        if not x2.is_contiguous() or x2.numel() != B * HW * C2:
            raise _l.PbeError("groupnorm: x2 shape mismatch")
    if gamma.numel() != C1 + C2 or beta.numel() != C1 + C2:
        raise _l.PbeError("groupnorm: affine length mismatch")
    lib = _l.load()
    st = group_stats_of(x, groups) if x2 is None else None
    if st is not None:                          # the producing conv left this tensor's statistics: normalisation pass only
        return _groupnorm_apply(x, st, gamma, beta, eps, silu)
    ws = workspace(x.device, "gn", lib.pbe_groupnorm_workspace_bytes(B, HW), 1 << 21)
    y = torch.empty(tuple(x.shape[:-1]) + (C1 + C2,), dtype=torch.float16, device=x.device)
    with _timed(f"n:{B}:{HW}:{C1}:{C2}"):
        _l.check(lib.pbe_groupnorm_f16(_p(x), _p(x2), _p(gamma), _p(beta), _p(y), B, HW, C1, C2, groups, float(eps), 1 if silu else 0,
                                       _p(ws), ws.numel(), _stream()), "pbe_groupnorm_f16")
    return y


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    _h(x, "layernorm x"); _f(gamma, "layernorm gamma"); _f(beta, "layernorm beta")
    x2 = x.reshape(-1, x.shape[-1])
    rows, Cc, ldx = _rows(x2, "layernorm x")
    y = torch.empty((rows, Cc), dtype=torch.float16, device=x.device)
    with _timed(f"l:{rows}:{Cc}"):
        _l.check(_l.load().pbe_layernorm_f16(_p(x2), _p(gamma), _p(beta), _p(y), rows, Cc, ldx, Cc, float(eps), _stream()), "pbe_layernorm_f16")
    return y.view(x.shape)


def layernorm_f8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """LayerNorm with an fp8 (OCP e4m3) output: returns (y8 uint8 [rows, C], row_scale fp32 [rows]); y = y8 * row_scale[:, None]."""
    _h(x, "layernorm_f8 x"); _f(gamma, "layernorm_f8 gamma"); _f(beta, "layernorm_f8 beta")
    x2 = x.reshape(-1, x.shape[-1])
    rows, Cc, ldx = _rows(x2, "layernorm_f8 x")
    y = torch.empty((rows, Cc), dtype=torch.uint8, device=x.device)
    sc = torch.empty((rows,), dtype=torch.float32, device=x.device)
    with _timed(f"l8:{rows}:{Cc}"):
        _l.check(_l.load().pbe_layernorm_f8(_p(x2), _p(gamma), _p(beta), _p(y), _p(sc), rows, Cc, ldx, Cc, float(eps), _stream()), "pbe_layernorm_f8")
    return y, sc


def gemm_f8(a8: torch.Tensor, a_scale: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
            resid: Optional[torch.Tensor] = None, act: int = ACT_NONE, alpha: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m, n] = act(alpha * a_scale[m] * w_scale[n] * sum_k a8[m, k] w8[n, k] + bias) + resid with OCP e4m3 operands (uint8
    tensors) and fp16 output.  2-D operands, or 3-D [batch, rows, K] for a strided batch (w8 / w_scale may have batch 1)."""
    _req(a8, torch.uint8, "gemm_f8 a8"); _req(w8, torch.uint8, "gemm_f8 w8"); _f(a_scale, "gemm_f8 a_scale"); _f(w_scale, "gemm_f8 w_scale")
    batch = 1
    sA = sW = sC = 0
    ssa = ssw = 0
    if a8.dim() == 3:
        batch = a8.shape[0] if a8.stride(0) != 0 else max(a8.shape[0], w8.shape[0])
        if a8.stride(2) != 1 or w8.dim() != 3 or w8.stride(2) != 1:
            raise _l.PbeError("gemm_f8: bad batched operands")
        M, K, lda, sA = a8.shape[1], a8.shape[2], a8.stride(1), a8.stride(0)
        N, Kw, ldw, sW = w8.shape[1], w8.shape[2], w8.stride(1), w8.stride(0)
        ssa = a_scale.stride(0) if a_scale.dim() == 2 else 0
        ssw = w_scale.stride(0) if w_scale.dim() == 2 else 0
        if out is None:
            out = torch.empty((batch, M, N), dtype=torch.float16, device=a8.device)
        ldc, sC = out.stride(1), out.stride(0)
    else:
        M, K, lda = _rows(a8, "gemm_f8 a8")
        N, Kw, ldw = _rows(w8, "gemm_f8 w8")
        if out is None:
            out = torch.empty((M, N // 2 if act == ACT_GEGLU else N), dtype=torch.float16, device=a8.device)
        ldc = _rows(out, "gemm_f8 out")[2]
    if Kw != K:
        raise _l.PbeError(f"gemm_f8: K mismatch, activations {K} vs weights {Kw}")
    if a_scale.numel() < M or w_scale.numel() < N:
        raise _l.PbeError("gemm_f8: scale vectors too short")
    ldr = 0
    if resid is not None:
        ldr = _rows(_h(resid, "gemm_f8 resid"), "gemm_f8 resid")[2]
    if bias is not None:
        _f(bias, "gemm_f8 bias")
    d = _l.GemmDesc(_p(a8), None, _p(w8), _p(_h(out, "gemm_f8 out")), _p(bias), None, _p(resid), M, N, K, K, lda, 0, ldw, ldc, ldr,
                    0, 0, sA, sW, sC, 0, batch, float(alpha), act, 0, None, 0, -1, _p(a_scale), _p(w_scale), ssa, ssw, 1)
    _launch("batch" if a8.dim() == 3 else "gemm", d)
    return out


def pack_linear_f8(w: torch.Tensor):
    """[N, K] fp32 weight -> (OCP e4m3 bytes uint8 [N, K], fp32 scale [N]) with one scale per output channel: w ~ w8 * scale[:, None].
    One-off, at pack time (BASELINE configs[4]).  A non-zero row's scale is floored at 2^-100 (pbe_layernorm_f8 has the same floor): below
    448 * 2^-128 the quotient 1 / scale overflows, and the row's bytes would come out NaN."""
    w2 = w.detach().reshape(w.shape[0], -1).float()
    amax = w2.abs().amax(1)
    scale = torch.where(amax > 0, (amax / 448.0).clamp(min=2.0 ** -100), torch.ones_like(amax))
    w8 = (w2 / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return w8, scale.contiguous()


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, B: int, H: int, Nq: int, Nk: int, D: int, scale: float, *,
              q_strides: Tuple[int, int], k_strides: Tuple[int, int], vt_strides: Tuple[int, int],
              out: Optional[torch.Tensor] = None, q_prescaled: bool = False, key_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T scale) v -> [B, Nq, H*D].  q/k: element (b,n,h,d) at b*bs + n*rs + h*D + d of the given
    (possibly sliced) tensors; vt: element (b,h,d,n) at b*bs + (h*D+d)*rs + n.  strides = (bs, rs) in elements.
    key_bias: fp32 [B, Nk] added to the logits of key n of sample b in the LOG2 domain (log2 of a token weight, -inf = absent), for
    every head (pbe_attention_kbias_f16, launch key `ab:`); None: pbe_attention_f16, launch key `a:`."""
    _h(q, "attention q"); _h(k, "attention k"); _h(vt, "attention vt")
    if out is None:
        out = torch.empty((B, Nq, H * D), dtype=torch.float16, device=q.device)
    d = _l.AttnDesc(_p(q), _p(k), _p(vt), _p(out), B, H, Nq, Nk, D, q_strides[0], q_strides[1], k_strides[0], k_strides[1],
                    vt_strides[0], vt_strides[1], out.stride(0), out.stride(1), float(scale), 1 if q_prescaled else 0)
    if key_bias is not None:
        _f(key_bias, "attention key_bias")
        if tuple(key_bias.shape) != (B, Nk) or key_bias.stride(1) != 1:
            raise _l.PbeError(f"attention: key_bias must be [{B}, {Nk}] with unit stride over the keys, got {tuple(key_bias.shape)}")
        with _timed(f"ab:{B}:{H}:{Nq}:{Nk}:{D}"):
            _l.check(_l.load().pbe_attention_kbias_f16(C.byref(d), _p(key_bias), key_bias.stride(0), _stream()), "pbe_attention_kbias_f16")
        return out
    with _timed(f"a:{B}:{H}:{Nq}:{Nk}:{D}"):
        _l.check(_l.load().pbe_attention_f16(C.byref(d), _stream()), "pbe_attention_f16")
    return out


CTX_MAX_TOKENS, CTX_MAX_HJ, CTX_MAX_C = 16, 128, 1280        # what pbe_ctx_attention_f16 takes (include/pbe_hip.h)


class CtxOperands:
    """The per-context operands of pbe_ctx_attention_f16 (include/pbe_hip.h): kq fp16 [B, HJ, C], colsum / kbias fp32 [B, HJ], vo fp16
    [B, C, HJP] (rows padded to a multiple of 8 columns, zeros), bias fp32 [C]; HJ = H * Nk.  Computed once per context
    (BasicTransformerBlock.context_operands); a slice of the batch (`rows`) serves one half of a guidance pair.  log2w: fp32 [B, Nk]
    log2 of the exemplar weights (-inf: token absent) or None; it rides beside the folded operands, which do not depend on it.
    log2rw: fp32 [B, tokens, Nk] (unit stride over the Nk tokens of the context) log2 of the weight of token j at query row t, for
    regional exemplars (pbe_ctx_attention_rw_f16), or None.  It REPLACES log2w - the host has multiplied the exemplar weights in.
    amap: the attribution-map target of pbe_ctx_attention_map_f16 or None: (fp32 [Bm, tokens, Nk], accumulate, b0) - the head-mean
    softmax weights of samples b0 .. b0 + Bm - 1 are stored to / added to it (ctx_attention launches it when it covers every sample
    of the launch; a caller whose map covers some of the samples launches per range of `rows`)."""
    __slots__ = ("kq", "colsum", "kbias", "vo", "bias", "B", "H", "Nk", "C", "log2w", "log2rw", "amap")

    def __init__(self, kq, colsum, kbias, vo, bias, H, Nk, log2w=None, log2rw=None, amap=None):
        self.kq, self.colsum, self.kbias, self.vo, self.bias, self.H, self.Nk = kq, colsum, kbias, vo, bias, int(H), int(Nk)
        self.B, self.C = kq.shape[0], kq.shape[2]
        self.log2w, self.log2rw, self.amap = log2w, log2rw, amap

    def rows(self, b0: int, b1: int) -> "CtxOperands":
        amap = None
        if self.amap is not None:                         # the part of the range the map covers must be all of it or none of it
            t, acc, m0 = self.amap
            m1 = m0 + t.shape[0]
            if m0 <= b0 and b1 <= m1:
                amap = (t[b0 - m0:b1 - m0], acc, 0)
            elif not (b1 <= m0 or m1 <= b0):
                raise _l.PbeError(f"CtxOperands.rows({b0}, {b1}): the attribution map covers samples {m0}..{m1 - 1}, a part of that range")
        return CtxOperands(self.kq[b0:b1], self.colsum[b0:b1], self.kbias[b0:b1], self.vo[b0:b1], self.bias, self.H, self.Nk,
                           None if self.log2w is None else self.log2w[b0:b1], None if self.log2rw is None else self.log2rw[b0:b1], amap)

    def with_row_weights(self, log2rw) -> "CtxOperands":
        """The same folded operands with the per-row table in place of the per-sample weights (nothing is re-folded)."""
        return CtxOperands(self.kq, self.colsum, self.kbias, self.vo, self.bias, self.H, self.Nk, None, log2rw, self.amap)

    def with_map(self, amap, accumulate=True, b0=0) -> "CtxOperands":
        """The same folded operands (and weights / table) with an attribution-map target for samples b0 .. (nothing is re-folded)."""
        return CtxOperands(self.kq, self.colsum, self.kbias, self.vo, self.bias, self.H, self.Nk, self.log2w, self.log2rw,
                           None if amap is None else (amap, bool(accumulate), int(b0)))

    def map_ranges(self):
        """The sample ranges [(b0, b1), ..] one launch each must cover so that the map target covers all of a launch or none of it."""
        if self.amap is None:
            return [(0, self.B)]
        m0, m1 = self.amap[2], self.amap[2] + self.amap[0].shape[0]
        return [r for r in ((0, m0), (m0, m1), (m1, self.B)) if r[1] > r[0]]


def ctx_attention_check(C_: int, H: int, Nk: int, tokens: int, M: int) -> None:
    """Host validation of a pbe_ctx_attention_f16 launch (no GPU needed): raises PbeError naming the limit that was broken."""
    if C_ % 64 or not 64 <= C_ <= CTX_MAX_C:
        raise _l.PbeError(f"ctx_attention: C = {C_} must be a multiple of 64 in 64..{CTX_MAX_C}")
    if not 1 <= Nk <= CTX_MAX_TOKENS:
        raise _l.PbeError(f"ctx_attention: {Nk} context tokens, the fused kernel takes 1..{CTX_MAX_TOKENS}")
    if H < 1 or H * Nk > CTX_MAX_HJ:
        raise _l.PbeError(f"ctx_attention: heads * context tokens = {H * Nk}, the fused kernel takes <= {CTX_MAX_HJ}")
    if tokens < 1 or M < 1 or M % tokens:
        raise _l.PbeError(f"ctx_attention: {M} rows are not whole samples of {tokens} tokens")


def ctx_attention_map_check(amap, B: int, tokens: int, Nk: int, device=None):
    """Host validation of an attribution-map target (no GPU needed): (tensor, accumulate) with tensor fp32 [B, tokens, Nk], unit stride
    over the context tokens, rows of >= Nk floats, on `device`.  Raises PbeError naming what is wrong; returns (tensor, accumulate)."""
    if not isinstance(amap, (tuple, list)) or len(amap) != 2 or not isinstance(amap[0], torch.Tensor):
        raise _l.PbeError("ctx_attention: attn_map must be (fp32 tensor [B, tokens, Nk], accumulate)")
    t, acc = amap
    if t.dtype != torch.float32:
        raise _l.PbeError(f"ctx_attention: attn_map must be fp32, got {t.dtype}")
    if t.dim() != 3 or tuple(t.shape) != (B, int(tokens), Nk):
        raise _l.PbeError(f"ctx_attention: attn_map must be [{B}, {int(tokens)}, {Nk}] (samples, tokens, context tokens), got {tuple(t.shape)}")
    if t.stride(2) != 1 or t.stride(1) < Nk or t.stride(0) < 0:
        raise _l.PbeError(f"ctx_attention: attn_map needs unit stride over the context tokens and rows of >= {Nk} floats, got strides {tuple(t.stride())}")
    if device is not None and t.device != device:
        raise _l.PbeError(f"ctx_attention: attn_map is on {t.device}, x on {device}")
    return t, bool(acc)


def ctx_attention(x: torch.Tensor, ops_ctx: CtxOperands, stats: "RowStats", eps: float, *, tokens: int, out: Optional[torch.Tensor] = None,
                  row_stats=True, attn_map=None):
    """y = x + attn2(LayerNorm(x), context) for a context of 1..16 tokens in one launch (pbe_ctx_attention_f16): x [M, C] fp16 is the RAW
    residual stream, `stats` the RowStats of its rows, ops_ctx the context's CtxOperands (sample b serves rows b * tokens ..).
    Returns (y, RowStats of y's rows - one partial; row_stats may be a RowStats to fill, or False: (y, None)).
    attn_map = (fp32 [B, tokens, Nk], accumulate) (default: ops_ctx.amap, which must then cover every sample): the launch is
    pbe_ctx_attention_map_f16 - the same y and statistics bit for bit, and the head-mean softmax weights stored to (accumulate False)
    or added to (True) the tensor; timing keys xam / xawm / xarm."""
    if not isinstance(ops_ctx, CtxOperands):
        raise _l.PbeError("ctx_attention: ops_ctx must be a CtxOperands")
    o = ops_ctx
    M, Cc, ldx = _rows(x, "ctx_attention x") if isinstance(x, torch.Tensor) and x.dim() == 2 else (0, 0, 0)
    if not M:
        raise _l.PbeError("ctx_attention: x must be a 2-D [M, C] tensor")
    ctx_attention_check(Cc, o.H, o.Nk, int(tokens), M)
    HJ = o.H * o.Nk
    if M // tokens != o.B or o.C != Cc:
        raise _l.PbeError(f"ctx_attention: operands are for {o.B} samples of width {o.C}, x holds {M // tokens} samples of width {Cc}")
    _h(x, "ctx_attention x"); _h(o.kq, "ctx_attention kq"); _h(o.vo, "ctx_attention vo")
    _f(o.colsum, "ctx_attention colsum"); _f(o.kbias, "ctx_attention kbias"); _f(o.bias, "ctx_attention bias")
    if tuple(o.kq.shape[1:]) != (HJ, Cc) or o.kq.stride(2) != 1 or tuple(o.vo.shape[:2]) != (o.B, Cc) or o.vo.shape[2] < HJ or o.vo.stride(2) != 1:
        raise _l.PbeError(f"ctx_attention: need kq [B, {HJ}, {Cc}] and vo [B, {Cc}, >= {HJ}], got {tuple(o.kq.shape)} / {tuple(o.vo.shape)}")
    if tuple(o.colsum.shape) != (o.B, HJ) or tuple(o.kbias.shape) != (o.B, HJ) or o.colsum.stride(1) != 1 or o.kbias.stride(1) != 1 \
            or o.colsum.stride(0) != o.kbias.stride(0) or o.bias.numel() != Cc or not o.bias.is_contiguous():
        raise _l.PbeError(f"ctx_attention: need colsum / kbias [B, {HJ}] with equal strides and bias [{Cc}]")
    if stats.ld - stats.row0 < M:
        raise _l.PbeError("ctx_attention: row statistics for every row of x are required")
    if out is None:
        out = torch.empty((M, Cc), dtype=torch.float16, device=x.device)
    if _rows(_h(out, "ctx_attention out"), "ctx_attention out")[:2] != (M, Cc):
        raise _l.PbeError(f"ctx_attention: out must be [{M}, {Cc}]")
    rs = None
    if row_stats is not False:
        rs = row_stats if isinstance(row_stats, RowStats) else RowStats(torch.empty((1, M, 2), dtype=torch.float32, device=x.device), 1, M)
        if rs.ld - rs.row0 < M:
            raise _l.PbeError("ctx_attention: row_stats buffer too short")
        rs = RowStats(rs.buf, 1, rs.ld, rs.row0)
    d = _l.CtxAttnDesc(_p(x), _p(out), _p(o.kq), _p(o.colsum), _p(o.kbias), _p(o.vo), _p(o.bias), stats.ptr(), None if rs is None else rs.ptr(),
                       M, Cc, int(tokens), o.H, o.Nk, ldx, out.stride(0), o.kq.stride(0), o.kq.stride(1), o.vo.stride(0), o.vo.stride(1),
                       o.colsum.stride(0), stats.parts, stats.ld, float(eps))
    am = None
    if attn_map is None and o.amap is not None:
        if o.amap[2] != 0 or o.amap[0].shape[0] != o.B:
            raise _l.PbeError(f"ctx_attention: the operands' attribution map covers samples {o.amap[2]}..{o.amap[2] + o.amap[0].shape[0] - 1} of {o.B}: "
                              "launch per range (CtxOperands.map_ranges / rows)")
        attn_map = o.amap[:2]
    if attn_map is not None:
        am = ctx_attention_map_check(attn_map, o.B, int(tokens), o.Nk, x.device)

    def launch(name, key, lw, rw):
        """One of the three forms, with the map when there is one: lw / rw are (pointer, strides..) or None."""
        lib = _l.load()
        if am is not None:
            with _timed(f"{key}m:{M}:{Cc}:{o.H}:{o.Nk}"):
                _l.check(lib.pbe_ctx_attention_map_f16(C.byref(d), *(lw or (None, 0)), *(rw or (None, 0, 0)), _p(am[0]), am[0].stride(0), am[0].stride(1),
                                                       1 if am[1] else 0, _stream()), "pbe_ctx_attention_map_f16")
            return
        with _timed(f"{key}:{M}:{Cc}:{o.H}:{o.Nk}"):
            if rw is not None:
                _l.check(lib.pbe_ctx_attention_rw_f16(C.byref(d), *rw, _stream()), name)
            elif lw is not None:
                _l.check(lib.pbe_ctx_attention_w_f16(C.byref(d), *lw, _stream()), name)
            else:
                _l.check(lib.pbe_ctx_attention_f16(C.byref(d), _stream()), name)
    if o.log2rw is not None:
        if o.log2w is not None:
            raise _l.PbeError("ctx_attention: log2rw replaces log2w (the row table holds the exemplar weights already): give one of them")
        t = _f(o.log2rw, "ctx_attention log2rw")
        if t.device != x.device:
            raise _l.PbeError(f"ctx_attention: log2rw is on {t.device}, x on {x.device}")
        if t.dim() != 3 or tuple(t.shape) != (o.B, int(tokens), o.Nk):
            raise _l.PbeError(f"ctx_attention: log2rw must be [{o.B}, {int(tokens)}, {o.Nk}] (samples, tokens, context tokens), got {tuple(t.shape)}")
        if t.stride(2) != 1 or t.stride(1) < o.Nk or t.stride(0) < 0:
            raise _l.PbeError(f"ctx_attention: log2rw needs unit stride over the context tokens and rows of >= {o.Nk} floats, got strides {tuple(t.stride())}")
        launch("pbe_ctx_attention_rw_f16", "xar", None, (_p(t), t.stride(0), t.stride(1)))
        return out, rs
    if o.log2w is not None:
        _f(o.log2w, "ctx_attention log2w")
        if tuple(o.log2w.shape) != (o.B, o.Nk) or o.log2w.stride(1) != 1:
            raise _l.PbeError(f"ctx_attention: log2w must be [{o.B}, {o.Nk}] with unit stride over the tokens, got {tuple(o.log2w.shape)}")
        launch("pbe_ctx_attention_w_f16", "xaw", (_p(o.log2w), o.log2w.stride(0)), None)
        return out, rs
    launch("pbe_ctx_attention_f16", "xa", None, None)
    return out, rs


def ctx_map_gather(acc: torch.Tensor, grid, scale: float = 1.0, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                   div: float = 1.0) -> torch.Tensor:
    """A level's attribution accumulator acc fp32 [B, h*w, K] (rows in NHWC order) with grid = (h, w) -> fp32 [B, K, Hl, Wl] planes
    (pbe_ctx_map_gather_f32): out[b, j, y, x] (+)= scale * (acc[b, (y / fy) * w + (x / fx), j] / div), fy = Hl / h, fx = Wl / w whole
    numbers; out None: the level's own grid (fy = fx = 1).  accumulate: add to `out` instead of storing.  div > 0: the launch count."""
    _f(acc, "ctx_map_gather acc")
    h, w = int(grid[0]), int(grid[1])
    if acc.dim() != 3 or not acc.is_contiguous() or acc.shape[1] != h * w or h < 1 or w < 1:
        raise _l.PbeError(f"ctx_map_gather: acc must be a contiguous [B, {h} * {w}, K] tensor, got {tuple(acc.shape)}")
    B, _, K = acc.shape
    if not float(div) > 0.0:
        raise _l.PbeError(f"ctx_map_gather: div must be > 0, got {div}")
    if out is None:
        if accumulate:
            raise _l.PbeError("ctx_map_gather: accumulate needs an `out` to add to")
        out = torch.empty((B, K, h, w), dtype=torch.float32, device=acc.device)
    _f(out, "ctx_map_gather out")
    if out.dim() != 4 or tuple(out.shape[:2]) != (B, K) or not out.is_contiguous() or out.shape[2] % h or out.shape[3] % w or out.device != acc.device:
        raise _l.PbeError(f"ctx_map_gather: out must be a contiguous [{B}, {K}, Hl, Wl] tensor on {acc.device} with Hl, Wl whole multiples of "
                          f"{h}, {w}, got {tuple(out.shape)}")
    _l.check(_l.load().pbe_ctx_map_gather_f32(_p(acc), _p(out), B, K, h, w, out.shape[2] // h, out.shape[3] // w, float(scale), float(div), 1 if accumulate else 0,
                                              _stream()), "pbe_ctx_map_gather_f32")
    return out


MX8_TOKENS, MX8_VT = 0, 1          # include/pbe_hip.h PBE_MX8_*: q / k rows (contraction = channel) and V^T rows (contraction = token)


class Mx8:
    """An MX-fp8 operand as pbe_quant_mx8_f16 wrote it: e4m3 bytes + E8M0 scales (uint8 tensors) in the layout of `mode`."""

    def __init__(self, data, scale, mode, B, H, N, D):
        self.data, self.scale, self.mode, self.B, self.H, self.N, self.D = data, scale, mode, B, H, N, D


def _extent_ok(t: torch.Tensor, elems: int) -> bool:
    """t's storage holds `elems` elements from t's first element on (the kernel reads that far through raw pointers)."""
    return t.storage_offset() * t.element_size() + elems * t.element_size() <= t.untyped_storage().nbytes()


def quant_mx8(x: torch.Tensor, B: int, H: int, N: int, D: int, *, rs: int, vt: bool = False, alpha: float = 1.0) -> Mx8:
    """fp16 rows -> MX-fp8 (OCP e4m3, one power-of-two scale per 32 contraction elements of one head), include/pbe_hip.h.
    vt=False: element (b, n, h, d) at x[(b*N + n)*rs + h*D + d] (q or k, e.g. a column slice of the q | k projection);
    vt=True:  element (b, h, d, n) at x[((b*H + h)*D + d)*rs + n] (V^T).  alpha multiplies the values before rounding."""
    _h(x, "quant_mx8 x")
    if D % 8 or rs % 8 or B <= 0 or H <= 0 or N <= 0 or D <= 0:
        raise _l.PbeError(f"quant_mx8: need D % 8 == 0 and rs % 8 == 0 (D={D}, rs={rs})")
    NP = (N + 63) // 64 * 64
    if vt:
        if rs < (N + 7) // 8 * 8 or not _extent_ok(x, (B * H * D - 1) * rs + N):
            raise _l.PbeError("quant_mx8: V^T rows out of the tensor's storage")
        DV = (D // 32 + 1) * 32
        data = torch.empty((B * H * D, NP), dtype=torch.uint8, device=x.device)
        scale = torch.empty((B, H, NP // 32, DV), dtype=torch.uint8, device=x.device)
    else:
        if rs < H * D or not _extent_ok(x, (B * N - 1) * rs + H * D):
            raise _l.PbeError("quant_mx8: token rows out of the tensor's storage")
        DP = (D + 63) // 64 * 64
        data = torch.empty((B * N, H * DP), dtype=torch.uint8, device=x.device)
        scale = torch.empty((B, H, DP // 32, NP), dtype=torch.uint8, device=x.device)
    mode = MX8_VT if vt else MX8_TOKENS
    with _timed(f"q8:{mode}:{B}:{H}:{N}:{D}"):
        _l.check(_l.load().pbe_quant_mx8_f16(_p(x), _p(data), _p(scale), mode, B, H, N, D, rs, float(alpha), _stream()), "pbe_quant_mx8_f16")
    return Mx8(data, scale, mode, B, H, N, D)


def attention_mx8(q: Mx8, k: Mx8, vt: Mx8, scale_log2e: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(scale_log2e / log2(e) * q k^T) v -> [B, Nq, H*D] fp16 on the MX-fp8 core (pbe_attention_mx8).  q / k from
    quant_mx8(vt=False), vt from quant_mx8(vt=True); pass scale_log2e = 1 when q was quantised with alpha = scale * log2(e)."""
    for t, m, what in ((q, MX8_TOKENS, "q"), (k, MX8_TOKENS, "k"), (vt, MX8_VT, "vt")):
        if not isinstance(t, Mx8) or t.mode != m:
            raise _l.PbeError(f"attention_mx8: {what} must be a quant_mx8 result of mode {m}")
        _req(t.data, torch.uint8, f"attention_mx8 {what}")
    B, H, D = q.B, q.H, q.D
    if (k.B, k.H, k.D) != (B, H, D) or (vt.B, vt.H, vt.D) != (B, H, D) or vt.N != k.N:
        raise _l.PbeError("attention_mx8: q / k / vt shapes disagree")
    if out is None:
        out = torch.empty((B, q.N, H * D), dtype=torch.float16, device=q.data.device)
    _h(out, "attention_mx8 out")
    if out.dim() != 3 or out.shape != (B, q.N, H * D) or out.stride(2) != 1:
        raise _l.PbeError("attention_mx8: out must be [B, Nq, H*D] with unit stride in the last dim")
    d = _l.AttnMx8Desc(_p(q.data), _p(q.scale), _p(k.data), _p(k.scale), _p(vt.data), _p(vt.scale), _p(out), B, H, q.N, k.N, D,
                       out.stride(0), out.stride(1), float(scale_log2e))
    with _timed(f"a8:{B}:{H}:{q.N}:{k.N}:{D}"):
        _l.check(_l.load().pbe_attention_mx8(C.byref(d), _stream()), "pbe_attention_mx8")
    return out


def _mx8_target(mode, B, H, N, D, device, out=None) -> Mx8:
    """MX-fp8 operand of quant_mx8's shape (N % 64 == 0: no token padding): `out` if given (checked), else empty tensors."""
    if out is not None:
        ref = _mx8_target(mode, B, H, N, D, "meta")
        if not isinstance(out, Mx8) or out.mode != mode or (out.B, out.H, out.N, out.D) != (B, H, N, D):
            raise _l.PbeError(f"MX-fp8 output: expected an Mx8 of mode {mode} for B={B} H={H} N={N} D={D}")
        for t, r, what in ((out.data, ref.data, "data"), (out.scale, ref.scale, "scale")):
            _req(t, torch.uint8, f"MX-fp8 output {what}")
            if t.shape != r.shape or not t.is_contiguous():
                raise _l.PbeError(f"MX-fp8 output {what}: expected a contiguous {tuple(r.shape)} tensor, got {tuple(t.shape)}")
        return out
    if mode == MX8_VT:
        return Mx8(torch.empty((B * H * D, N), dtype=torch.uint8, device=device),
                   torch.empty((B, H, N // 32, (D // 32 + 1) * 32), dtype=torch.uint8, device=device), MX8_VT, B, H, N, D)
    DP = (D + 63) // 64 * 64
    return Mx8(torch.empty((B * N, H * DP), dtype=torch.uint8, device=device),
               torch.empty((B, H, DP // 32, N), dtype=torch.uint8, device=device), MX8_TOKENS, B, H, N, D)


def _mx8_desc(ranges, channel_rows: bool):
    mx = _l.Mx8OutDesc()
    mx.nranges, mx.channel_rows = len(ranges), 1 if channel_rows else 0
    for i, (t, col0, alpha) in enumerate(ranges):
        mx.r[i] = _l.Mx8OutRange(_p(t.data), _p(t.scale), t.mode, int(col0), float(alpha), t.B, t.H, t.N, t.D)
    return mx


def qkv_mx8(x2d: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, ln, B: int, H: int, N: int, D: int,
            alpha: float = 1.0, alpha_cols: int = 0, out=None):
    """The LayerNorm-folded q | k | v projection of gemm(x2d, w, bias, ln=ln, alpha=alpha, alpha_cols=alpha_cols, vt=..., vt_col0=2*H*D,
    vt_tokens=N) with its output written as MX-fp8 (pbe_gemm_mx8out_f16): returns (q, k, vt) Mx8 operands, byte for byte what
    quant_mx8 makes of that gemm's fp16 q | k and V^T (alpha 1).  out: optional (q, k, vt) Mx8 targets to write into."""
    _h(x2d, "qkv_mx8 x"); _h(w, "qkv_mx8 w")
    M, K, lda = _rows(x2d, "qkv_mx8 x")
    Nw, Kw, ldw = _rows(w, "qkv_mx8 w")
    inner = H * D
    if Kw != K or Nw != 3 * inner or M != B * N:
        raise _l.PbeError(f"qkv_mx8: need w [3*H*D, K] and x [B*N, K], got {tuple(w.shape)} / {tuple(x2d.shape)}")
    if bias is not None:
        _f(bias, "qkv_mx8 bias")
    st, colsum, eps = ln
    _f(colsum, "qkv_mx8 ln colsum")
    if colsum.numel() != Nw or st.ld - st.row0 < M:
        raise _l.PbeError("qkv_mx8: LayerNorm fold needs colsum [3*H*D] and row statistics for every row of x")
    q, k, v = (_mx8_target(m, B, H, N, D, x2d.device, o) for m, o in zip((MX8_TOKENS, MX8_TOKENS, MX8_VT), out or (None,) * 3))
    d = _l.GemmDesc(_p(x2d), None, _p(w), None, _p(bias), None, None, M, Nw, K, K, lda, 0, ldw, 0, 0, 0, 1, 0, 0, 0, 0, 1, float(alpha), ACT_NONE, 0,
                    None, 0, -1)
    d.alpha_cols = int(alpha_cols)
    d.ln_stats, d.ln_parts, d.ln_stats_ld, d.ln_colsum, d.ln_eps = st.ptr(), st.parts, st.ld, _p(colsum), float(eps)
    d.vt_col0, d.vt_tokens = 2 * inner, N
    _launch("mx8", d, _mx8_desc([(q, 0, 1.0), (k, inner, 1.0), (v, 2 * inner, 1.0)], False))
    return q, k, v


def qkv_mx8_f8(x8: torch.Tensor, sx: torch.Tensor, wqk8: torch.Tensor, sqk: torch.Tensor, wv8: torch.Tensor, sv: torch.Tensor, *,
               B: int, H: int, N: int, D: int, q_alpha: float, out=None):
    """The two fp8-operand projections of the linear-fp8 self-attention with MX-fp8 output: q | k = gemm_f8(x8, sx, wqk8, sqk) and
    V^T = gemm_f8(wv8 per sample, sv, x8 per sample, sx) -> (q, k, vt) Mx8 operands, byte for byte quant_mx8 of those fp16 outputs
    (q with alpha q_alpha).  out: optional (q, k, vt) Mx8 targets to write into."""
    for t, what in ((x8, "x8"), (wqk8, "wqk8"), (wv8, "wv8")):
        _req(t, torch.uint8, f"qkv_mx8_f8 {what}")
    for t, what in ((sx, "sx"), (sqk, "sqk"), (sv, "sv")):
        _f(t, f"qkv_mx8_f8 {what}")
    M, K, lda = _rows(x8, "qkv_mx8_f8 x8")
    Nqk, Kw, ldw = _rows(wqk8, "qkv_mx8_f8 wqk8")
    Nv, Kv, ldv = _rows(wv8, "qkv_mx8_f8 wv8")
    inner = H * D
    if Kw != K or Kv != K or Nqk != 2 * inner or Nv != inner or M != B * N or sx.numel() < M or sqk.numel() < Nqk or sv.numel() < Nv:
        raise _l.PbeError("qkv_mx8_f8: need x8 [B*N, K], wqk8 [2*H*D, K], wv8 [H*D, K], sx [B*N], sqk [2*H*D], sv [H*D]")
    q, k, v = (_mx8_target(m, B, H, N, D, x8.device, o) for m, o in zip((MX8_TOKENS, MX8_TOKENS, MX8_VT), out or (None,) * 3))
    d = _l.GemmDesc(_p(x8), None, _p(wqk8), None, None, None, None, M, Nqk, K, K, lda, 0, ldw, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1.0, ACT_NONE, 0,
                    None, 0, -1, _p(sx), _p(sqk), 0, 0, 1)
    _launch("mx8", d, _mx8_desc([(q, 0, q_alpha), (k, inner, 1.0)], False))
    # swapped operands: rows = channels, columns = tokens, one sample per batch entry
    d = _l.GemmDesc(_p(wv8), None, _p(x8), None, None, None, None, inner, N, K, K, ldv, 0, lda, 0, 0, 0, 0, 0, N * lda, 0, 0, B, 1.0, ACT_NONE, 0,
                    None, 0, -1, _p(sv), _p(sx), 0, N, 1)
    _launch("mx8", d, _mx8_desc([(v, 0, 1.0)], True))
    return q, k, v


def softmax_rows(x: torch.Tensor, scale: float) -> torch.Tensor:
    _h(x, "softmax_rows x")
    x2 = x.reshape(-1, x.shape[-1])
    rows, cols, ldx = _rows(x2, "softmax_rows x")
    y = torch.empty((rows, cols), dtype=torch.float16, device=x.device)
    _l.check(_l.load().pbe_softmax_rows_f16(_p(x2), _p(y), rows, cols, ldx, cols, float(scale), _stream()), "pbe_softmax_rows_f16")
    return y.view(x.shape)


def geglu(h: torch.Tensor) -> torch.Tensor:
    _h(h, "geglu h")
    if not h.is_contiguous():
        raise _l.PbeError("geglu: h must be contiguous")
    F = h.shape[-1] // 2
    M = h.numel() // (2 * F)
    y = torch.empty(tuple(h.shape[:-1]) + (F,), dtype=torch.float16, device=h.device)
    _l.check(_l.load().pbe_geglu_f16(_p(h), _p(y), M, F, _stream()), "pbe_geglu_f16")
    return y


def timestep_embedding(t: torch.Tensor, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    _req(t, torch.int64, "timestep_embedding t")
    t = t.contiguous()
    y = torch.empty((t.shape[0], dim), dtype=torch.float16, device=t.device)
    _l.check(_l.load().pbe_timestep_embedding_f16(_p(t), _p(y), t.shape[0], dim, float(max_period), _stream()), "pbe_timestep_embedding_f16")
    return y


def nchw_to_nhwc(x: torch.Tensor, cp: Optional[int] = None) -> torch.Tensor:
    """fp32 NCHW -> fp16 NHWC with the channel dim zero-padded to cp."""
    _f(x, "nchw_to_nhwc x")
    x = x.contiguous()
    B, Cc, H, W = x.shape
    cp = Cc if cp is None else cp
    y = torch.empty((B, H, W, cp), dtype=torch.float16, device=x.device)
    _l.check(_l.load().pbe_nchw_f32_to_nhwc_f16(_p(x), _p(y), B, Cc, H * W, cp, _stream()), "pbe_nchw_f32_to_nhwc_f16")
    return y


def nhwc_to_nchw(x: torch.Tensor, c: Optional[int] = None) -> torch.Tensor:
    """fp16 NHWC [B,H,W,ld] -> fp32 NCHW of the first c channels."""
    _h(x, "nhwc_to_nchw x")
    if x.dim() != 4 or not x.is_contiguous():
        raise _l.PbeError(f"nhwc_to_nchw: x must be contiguous fp16 NHWC [B, H, W, ld], got {tuple(x.shape)}")
    B, H, W, ld = x.shape
    c = ld if c is None else int(c)
    if not 1 <= c <= ld:
        raise _l.PbeError(f"nhwc_to_nchw: c = {c} channels of a tensor with {ld}")
    y = torch.empty((B, c, H, W), dtype=torch.float32, device=x.device)
    _l.check(_l.load().pbe_nhwc_f16_to_nchw_f32(_p(x), _p(y), B, c, H * W, ld, _stream()), "pbe_nhwc_f16_to_nchw_f32")
    return y


def plms_pack_input(x: torch.Tensor, z_inpaint: torch.Tensor, mask: torch.Tensor, dup: int) -> torch.Tensor:
    _f(x, "plms x"); _f(z_inpaint, "plms z_inpaint"); _f(mask, "plms mask")
    B, _, H, W = x.shape
    if tuple(z_inpaint.shape) != (B, 4, H, W) or tuple(mask.shape) != (B, 1, H, W):
        raise _l.PbeError(f"plms_pack_input: shape mismatch x={tuple(x.shape)} z={tuple(z_inpaint.shape)} mask={tuple(mask.shape)}")
    x9 = torch.empty((dup * B, H, W, 16), dtype=torch.float16, device=x.device)
    _l.check(_l.load().pbe_plms_pack_input(_p(x.contiguous()), _p(z_inpaint.contiguous()), _p(mask.contiguous()), _p(x9), B, H * W, dup,
                                           _stream()), "pbe_plms_pack_input")
    return x9


def _step_operands(what: str, eps_out: torch.Tensor, dup: int, x: torch.Tensor) -> Tuple[int, int, int, int]:
    """(B, H, W, ld) of a sampler update's x (contiguous fp32 NCHW [B, 4, H, W]) and of the U-Net output it consumes, eps_out (contiguous
    fp16 NHWC [dup * B, H, W, ld >= 4] on x's device); the dtypes and dup are the caller's to check first."""
    if x.dim() != 4 or x.shape[1] != 4 or not x.is_contiguous():
        raise _l.PbeError(f"{what}: x must be contiguous fp32 NCHW [B, 4, H, W], got {tuple(x.shape)}")
    B, _, H, W = x.shape
    if eps_out.dim() != 4 or tuple(eps_out.shape[:3]) != (dup * B, H, W) or eps_out.shape[3] < 4 or not eps_out.is_contiguous() or eps_out.device != x.device:
        raise _l.PbeError(f"{what}: eps_out must be contiguous fp16 NHWC [{dup * B}, {H}, {W}, ld >= 4] on x's device, got {tuple(eps_out.shape)}")
    return B, H, W, eps_out.shape[3]


def plms_update(eps_out: torch.Tensor, dup: int, cfg_scale: float, x: torch.Tensor, hist, coef8, want_e_t: bool = True,
                want_pred: bool = True):
    """Fused CFG combine + multistep weights + x_prev / pred_x0 (plms.py:188-189, 202-219, 230-244)."""
    _h(eps_out, "plms eps_out"); _f(x, "plms x")
    if dup not in (1, 2) or len(coef8) != 8 or len(hist) > 3:
        raise _l.PbeError(f"plms_update: dup must be 1 or 2, coef8 eight floats and hist at most 3 tensors, got dup={dup}, {len(coef8)} coefficients, "
                          f"{len(hist)} history tensors")
    B, H, W, ld = _step_operands("plms_update", eps_out, dup, x)
    h = [None, None, None]
    for i, t in enumerate(hist):
        h[i] = _f(t, "plms history")
        if t.shape != x.shape or not t.is_contiguous() or t.device != x.device:
            raise _l.PbeError(f"plms_update: history tensor {i} must match x ({tuple(x.shape)}, contiguous, same device), got {tuple(t.shape)}")
    e_t = torch.empty_like(x) if want_e_t else None
    pred = torch.empty_like(x) if want_pred else None
    x_prev = torch.empty_like(x)
    arr = (C.c_float * 8)(*[float(v) for v in coef8])
    _l.check(_l.load().pbe_plms_update(_p(eps_out), ld, dup, float(cfg_scale), _p(x), _p(h[0]), _p(h[1]), _p(h[2]), arr, _p(e_t),
                                       _p(x_prev), _p(pred), B, H * W, _stream()), "pbe_plms_update")
    return x_prev, pred, e_t


def dpmpp_update(eps_out: torch.Tensor, dup: int, cfg_scale: float, x: torch.Tensor, x0_prev: Optional[torch.Tensor], coef5,
                 want_pred: bool = True):
    """One DPM-Solver++(2M) step in one launch: CFG combine, x0 = (x - sigma_t e) / alpha_t, x_next = kx x + k0 x0 [+ k1 x0_prev].
    eps_out fp16 NHWC [dup*B, H, W, ld >= 4], x / x0_prev fp32 NCHW [B, 4, H, W] (x0_prev None: first-order step, k1 must be 0),
    coef5 = (sigma_t, 1/alpha_t, kx, k0, k1) -> (x_next, x0); x0 is None with want_pred=False (the last step keeps no history)."""
    _h(eps_out, "dpmpp eps_out"); _f(x, "dpmpp x")
    if dup not in (1, 2) or len(coef5) != 5:
        raise _l.PbeError(f"dpmpp_update: dup must be 1 or 2 and coef5 five floats, got dup={dup}, {len(coef5)} coefficients")
    B, H, W, ld = _step_operands("dpmpp_update", eps_out, dup, x)
    if x0_prev is not None:
        _f(x0_prev, "dpmpp x0_prev")
        if x0_prev.shape != x.shape or not x0_prev.is_contiguous() or x0_prev.device != x.device:
            raise _l.PbeError(f"dpmpp_update: x0_prev must match x ({tuple(x.shape)}, contiguous, same device), got {tuple(x0_prev.shape)}")
    elif float(coef5[4]) != 0.0:
        raise _l.PbeError("dpmpp_update: k1 != 0 needs x0_prev")
    x0 = torch.empty_like(x) if want_pred else None
    x_next = torch.empty_like(x)
    arr = (C.c_float * 5)(*[float(v) for v in coef5])
    _l.check(_l.load().pbe_dpmpp_update(_p(eps_out), ld, dup, float(cfg_scale), _p(x), _p(x0_prev), arr, _p(x0), _p(x_next),
                                        B, H * W, _stream()), "pbe_dpmpp_update")
    return x_next, x0


def axpy_(y: torch.Tensor, a: float, x: torch.Tensor) -> torch.Tensor:
    """y += a * x in place (fp32): the sigma_t * noise term of a stochastic DDIM step (ddim.py:236-238)."""
    _f(y, "axpy y"); _f(x, "axpy x")
    if not y.is_contiguous() or not x.is_contiguous() or x.numel() != y.numel():
        raise _l.PbeError("axpy_: contiguous tensors of equal size")
    _l.check(_l.load().pbe_axpy_f32(_p(y), float(a), _p(x), y.numel(), _stream()), "pbe_axpy_f32")
    return y


# ---- noise as a function of per-sample seeds (csrc/noise.hip; the stream plan lives in pbe_amd.noise) ----
def seed_words(seeds) -> list:
    """Python ints in [0, 2^64) -> the int64 values that hold them (two's complement at and above 2^63).  Anything else raises."""
    if isinstance(seeds, (str, bytes)) or not hasattr(seeds, "__iter__"):
        raise _l.PbeError(f"seeds: expected an int64 tensor [B] on the GPU or a sequence of ints in [0, 2^64), got {type(seeds).__name__}")
    out = []
    for s in seeds:
        if isinstance(s, bool) or not isinstance(s, int):
            raise _l.PbeError(f"seeds: {s!r} is not an int (a seed is an integer in [0, 2^64))")
        if not 0 <= s < 1 << 64:
            raise _l.PbeError(f"seeds: {s} is outside [0, 2^64)")
        out.append(s - (1 << 64) if s >= 1 << 63 else s)
    return out


def seed_tensor(seeds, B: Optional[int], device=None) -> torch.Tensor:
    """seeds (an int64 tensor [B] on the GPU, or a sequence of Python ints in [0, 2^64)) -> a contiguous int64 [B] tensor on `device`
    (None: the current GPU; a tensor stays where it is)."""
    if isinstance(seeds, torch.Tensor):
        _req(seeds, torch.int64, "seeds")
        if seeds.dim() != 1:
            raise _l.PbeError(f"seeds: expected shape [B], got {tuple(seeds.shape)}")
        t = seeds.contiguous()
    else:
        words = seed_words(seeds)                      # validated before any device is touched
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _l.PbeError("seeds: the noise is drawn on the GPU (the HIP path has no CPU fallback)")
        t = torch.tensor(words, dtype=torch.int64, device=device)
    if B is not None and t.numel() != B:
        raise _l.PbeError(f"seeds: {t.numel()} seeds for a batch of {B}")
    return t


def sub_tensor(sub, B: int, device) -> Optional[torch.Tensor]:
    """sub (None, an int32 tensor [B] on the GPU, or a sequence of ints in [0, 2^31)) -> None or a contiguous int32 [B] tensor."""
    if sub is None:
        return None
    if isinstance(sub, torch.Tensor):
        t = _req(sub, torch.int32, "sub").contiguous()
    else:
        vals = list(sub)
        if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 31 for v in vals):
            raise _l.PbeError(f"sub: expected ints in [0, 2^31), got {vals!r}")
        t = torch.tensor(vals, dtype=torch.int32, device=device)
    if t.dim() != 1 or t.numel() != B:
        raise _l.PbeError(f"sub: expected {B} values, got shape {tuple(t.shape)}")
    return t


def _stream_id(stream) -> int:
    if isinstance(stream, bool) or not isinstance(stream, int) or not 0 <= stream < 1 << 64:
        raise _l.PbeError(f"stream: expected an int in [0, 2^64), got {stream!r}")
    return stream


def philox_u32(seeds, n_words: int, stream: int = 0, sub=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw Philox4x32-10 words: int32 [B, n_words] holding the unsigned words' bits (torch has no uint32 arithmetic; view as
    numpy uint32 to compare).  Word w of sample b is x[w % 4] of counter (w // 4, sub[b], stream lo32, stream hi32) under key seeds[b]."""
    sd = seed_tensor(seeds, None, out.device if isinstance(out, torch.Tensor) else None)
    B, n_words = sd.numel(), int(n_words)
    sb = sub_tensor(sub, B, sd.device)
    if B < 1 or n_words < 1:
        raise _l.PbeError(f"philox_u32: nothing to draw ({B} samples of {n_words} words)")
    if out is None:
        out = torch.empty((B, n_words), dtype=torch.int32, device=sd.device)
    elif out.dtype != torch.int32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B, n_words) or out.device != sd.device:
        raise _l.PbeError(f"philox_u32: out must be a contiguous int32 [{B}, {n_words}] tensor on the seeds' device")
    _l.check(_l.load().pbe_philox_u32(_p(out), _p(sd), _p(sb), B, n_words, _stream_id(stream), _stream()), "pbe_philox_u32")
    return out


def randn_seeded(seeds, shape, stream: int, sub=None, out: Optional[torch.Tensor] = None, a: float = 0.0, b: float = 1.0) -> torch.Tensor:
    """out = a * out + b * z with z standard normal, fp32, of the full shape [B, ...]: sample i is a pure function of (seeds[i], sub[i],
    stream, element index) - Philox4x32-10 and Box-Muller as include/pbe_hip.h states them - whatever B, the sample's place in the batch
    or the device.  seeds: an int64 tensor [B] on the GPU or a sequence of Python ints in [0, 2^64) (at and above 2^63: their two's
    complement); sub: None (0), an int32 tensor [B] or ints in [0, 2^31).  a == 0 never reads out (a fresh tensor unless given); a != 0
    needs out.  One launch, no temporary, no generator state."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1 or any(s < 1 for s in shape):
        raise _l.PbeError(f"randn_seeded: shape must be [B, ...] with positive sizes, got {shape}")
    B = shape[0]
    n = 1
    for s in shape[1:]:
        n *= s
    if out is not None:
        _f(out, "randn_seeded out")
        if tuple(out.shape) != shape or not out.is_contiguous():
            raise _l.PbeError(f"randn_seeded: out must be a contiguous fp32 tensor of shape {shape}, got {tuple(out.shape)}")
    elif float(a) != 0.0:
        raise _l.PbeError("randn_seeded: a != 0 accumulates into out, which is missing")
    sd = seed_tensor(seeds, B, None if out is None else out.device)
    if out is not None and sd.device != out.device:
        raise _l.PbeError(f"randn_seeded: seeds on {sd.device}, out on {out.device}")
    sb = sub_tensor(sub, B, sd.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=sd.device)
    _l.check(_l.load().pbe_randn_philox_f32(_p(out), _p(sd), _p(sb), B, n, _stream_id(stream), float(a), float(b), _stream()), "pbe_randn_philox_f32")
    return out


def qsample_blend(x0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, img: torch.Tensor, sqrt_ac: float, sqrt_1m_ac: float) -> torch.Tensor:
    """img_orig = q_sample(x0, t); img_orig * mask + (1 - mask) * img (plms.py:150-153, ddim.py:178-181), fp32 NCHW."""
    for t, n in ((x0, "x0"), (noise, "noise"), (mask, "mask"), (img, "img")):
        _f(t, f"qsample_blend {n}")
    x0, noise, mask, img = x0.contiguous(), noise.contiguous(), mask.contiguous(), img.contiguous()
    B, Cc, H, W = img.shape
    if x0.shape != img.shape or noise.shape != img.shape or mask.shape[0] != B or mask.shape[1] not in (1, Cc) or tuple(mask.shape[2:]) != (H, W):
        raise _l.PbeError("qsample_blend: x0 / noise must match img, mask [B, 1 or C, H, W]")
    out = torch.empty_like(img)
    _l.check(_l.load().pbe_qsample_blend_f32(_p(x0), _p(noise), _p(mask), _p(img), float(sqrt_ac), float(sqrt_1m_ac), _p(out), B, Cc, H * W,
                                             mask.shape[1], _stream()), "pbe_qsample_blend_f32")
    return out


def posterior_sample(moments: torch.Tensor, eps: torch.Tensor, scale: float) -> torch.Tensor:
    """z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps): moments fp16 NHWC [B, H, W, ld >= 8] (mean in channels 0 .. 3, logvar in
    4 .. 7), eps fp32 NCHW [B, 4, H, W] -> fp32 NCHW [B, 4, H, W]."""
    _h(moments, "posterior moments"); _f(eps, "posterior eps")
    if moments.dim() != 4 or moments.shape[3] < 8 or not moments.is_contiguous():
        raise _l.PbeError(f"posterior_sample: moments must be contiguous fp16 NHWC [B, H, W, ld >= 8], got {tuple(moments.shape)}")
    B, H, W, ld = moments.shape
    if tuple(eps.shape) != (B, 4, H, W) or not eps.is_contiguous() or eps.device != moments.device:
        raise _l.PbeError(f"posterior_sample: eps must be contiguous fp32 NCHW [{B}, 4, {H}, {W}] on the moments' device, got {tuple(eps.shape)}")
    z = torch.empty((B, 4, H, W), dtype=torch.float32, device=moments.device)
    _l.check(_l.load().pbe_posterior_sample(_p(moments), ld, _p(eps), _p(z), B, H * W, float(scale), _stream()), "pbe_posterior_sample")
    return z


def scale_latent(z: torch.Tensor, inv_scale: float) -> torch.Tensor:
    _f(z, "scale_latent z")
    z = z.contiguous()
    B, Cc, H, W = z.shape
    y = torch.empty((B, H, W, 8), dtype=torch.float16, device=z.device)
    _l.check(_l.load().pbe_scale_latent_f16(_p(z), _p(y), B, Cc, H * W, float(inv_scale), _stream()), "pbe_scale_latent_f16")
    return y


def image_post(x: torch.Tensor) -> torch.Tensor:
    """clamp((x + 1) / 2, 0, 1) of the first 3 channels: fp16 NHWC [B, H, W, ld >= 3] -> fp32 NCHW [B, 3, H, W]."""
    _h(x, "image_post x")
    if x.dim() != 4 or x.shape[3] < 3 or not x.is_contiguous():
        raise _l.PbeError(f"image_post: x must be contiguous fp16 NHWC [B, H, W, ld >= 3], got {tuple(x.shape)}")
    B, H, W, ld = x.shape
    y = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    _l.check(_l.load().pbe_image_post_f32(_p(x), _p(y), B, H * W, ld, _stream()), "pbe_image_post_f32")
    return y


def bcast_row(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, B: int, y_bs: int) -> None:
    """out[bi * y_bs + c] = a[c] + b[c] for bi < B."""
    _h(a, "bcast_row a"); _h(b, "bcast_row b"); _h(out, "bcast_row out")
    _l.check(_l.load().pbe_bcast_row_f16(_p(a), _p(b), _p(out), B, a.numel(), y_bs, _stream()), "pbe_bcast_row_f16")


# ---- weight packing (one-off, at load time) ---------------------------------------------------
def pack_conv3x3(w: torch.Tensor, cin_pad: Optional[int] = None, split: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """OIHW fp32 -> packed fp16 [Cout, 9*Cin] in the K order the kernels gather in.
    * cin_pad is None (Cin % 64 == 0, implicit-GEMM conv): k = ((ci // cb) * 9 + ky*3+kx) * cb + ci % cb with
      cb = conv_kblock(Cin) — channel-block major, tap minor, so a pixel's 9 shifted reads stay within 9*cb/64
      k-tiles of each other (L2 reuse) while cb/64 consecutive k-tiles walk the same pixel (+64 channels).
    * cin_pad given (tiny Cin, im2col + GEMM path): k = (ky*3+kx) * cin_pad + ci, zero-padded channels."""
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3
    wp = w.permute(0, 2, 3, 1)                                   # [Co, 3, 3, Ci]
    if cin_pad is not None:
        if cin_pad != ci:
            wp = torch.nn.functional.pad(wp, (0, cin_pad - ci))
        return wp.reshape(co, -1).to(torch.float16).contiguous()
    assert ci % 64 == 0, "implicit-GEMM conv needs Cin % 64 == 0 (use cin_pad for the im2col path)"
    cb = conv_kblock(*(split if split else (ci, 0)))       # split = (C1, C2) when the conv reads a channel concat
    assert not split or sum(split) == ci
    wp = wp.reshape(co, 9, ci // cb, cb).permute(0, 2, 1, 3)      # [Co, Ci/cb, 9, cb]
    return wp.reshape(co, 9 * ci).to(torch.float16).contiguous()


def pack_conv3x3_up_phases(w: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 weight of a 3x3 conv that follows a nearest-2x upsample (openaimodel.py:109-119, model.py:44-53) -> fp16 [4, Cout, 4*Cin]:
    output pixel (2y + py, 2x + px) reads only the 2x2 source block rows {y - 1 + py, y + py} x columns {x - 1 + px, x + px}, so per phase
    (py, px) the 9 taps collapse to 4 with summed weights (py = 0: ky {0} | {1, 2}; py = 1: ky {0, 1} | {2}; same in x), summed in fp32
    before the single fp16 rounding.  K order per phase: k = ((ci // 64) * 4 + ty * 2 + tx) * 64 + ci % 64.  4 / 9 of the MACs of the fused
    upsample gather."""
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3 and ci % 64 == 0
    w32 = w.detach().float()
    sets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    out = []
    for py in (0, 1):
        for px in (0, 1):
            taps = []
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = 0
                    for ky in sets[py][ty]:
                        for kx in sets[px][tx]:
                            acc = acc + w32[:, :, ky, kx]
                    taps.append(acc)                          # [Co, Ci]
            wp = torch.stack(taps, 1)                         # [Co, 4, Ci]
            wp = wp.reshape(co, 4, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, 4 * ci)
            out.append(wp)
    return torch.stack(out, 0).to(torch.float16).contiguous()


def conv_kblock(c1: int, c2: int = 0) -> int:
    """Channel block of the conv K order (deterministic, shared by pack_conv3x3 and conv3x3): 64, the kernels' k-tile.  k = ((ci // 64)
    * 9 + tap) * 64 + ci % 64: the 9 taps of a 64-channel block are consecutive k-tiles, which is what the halo-resident tiles need
    (one halo image per block serves its 9 taps) and keeps the gather kernel's shifted re-reads within 9 k-tiles (L2 hits)."""
    if c1 % 64 or c2 % 64:
        raise _l.PbeError(f"conv: C1={c1} / C2={c2} are not multiples of 64")
    return 64


def pack_linear(w: torch.Tensor) -> torch.Tensor:
    return w.reshape(w.shape[0], -1).to(torch.float16).contiguous()


def pack_linear_ln(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """Linear(LayerNorm(x)) with the LayerNorm FOLDED into the GEMM (pbe_gemm_desc.ln_stats): returns (W * gamma as fp16 [N, K], the
    fp32 bias W beta + b, colsum[n] = sum_k of the fp16 values of row n) - LN(x) W^T + b = rstd (x (W gamma)^T - mean colsum) + W beta + b."""
    w32 = w.detach().reshape(w.shape[0], -1).float()
    wg = (w32 * gamma.detach().float()[None, :]).to(torch.float16).contiguous()
    c2 = w32.double() @ beta.detach().double()
    if bias is not None:
        c2 = c2 + bias.detach().double()
    return wg, c2.float().contiguous(), wg.double().sum(1).float().contiguous()


def interleave_geglu(w: torch.Tensor, b: torch.Tensor):
    """GEGLU projection [2F, K] (rows 0..F-1 = value, F..2F-1 = gate, attention.py:41-45) -> rows interleaved
    (x_0, g_0, x_1, g_1, ...) so the GEMM epilogue sees each (value, gate) pair in one accumulator quad.  Dtypes are kept."""
    F = w.shape[0] // 2
    return torch.stack([w[:F], w[F:]], 1).reshape(2 * F, -1), torch.stack([b[:F], b[F:]], 1).reshape(2 * F)


def pack_geglu(w: torch.Tensor, b: torch.Tensor):
    """interleave_geglu as the GEMM takes it: fp16 weights, fp32 bias."""
    wi, bi = interleave_geglu(w, b)
    return wi.to(torch.float16).contiguous(), bi.detach().float().contiguous()


def tune(key: int, value: int) -> None:
    _l.check(_l.load().pbe_tune(key, value), "pbe_tune")


# ---- profiling --------------------------------------------------------------------------------
def prof_enable(on: bool) -> None:
    _l.load().pbe_prof_enable(1 if on else 0)


def prof_reset() -> None:
    _l.load().pbe_prof_reset()


def prof_collect():
    lib = _l.load()
    buf = (C.c_double * (5 * 16))()
    n = lib.pbe_prof_collect(buf, 16)
    out = {}
    for k in range(n):
        out[lib.pbe_prof_class_name(k).decode()] = {"launches": int(buf[5 * k]), "ms": buf[5 * k + 1], "work": buf[5 * k + 2],
                                                    "bytes": buf[5 * k + 3], "roofline_ms": buf[5 * k + 4]}
    return out


# ---- pictures and masks: the wrappers of ops_picture.py under their names here (ops.window_image, ops.tone_stats, ...) ----------------
from .ops_picture import *  # noqa: E402,F401,F403
