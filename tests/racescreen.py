"""Race screens of the counted-wait main loops: helpers of test_racescreen_cpu.py and test_racescreen_gpu.py.  Not a conftest: plain
functions only.

Four hand-scheduled structures overlap LDS-DMA with MFMA work behind ONE raw s_barrier per k-tile and an `s_waitcnt vmcnt(N)` whose N is
picked by a branch ("Race screens"):

  R    the ring loop of igemm_kernel.h (MODE 0 / 1)        rem = min(tiles left in the slice, D - 1)         -> vmcnt(rem * LPT)
  H1   the halo loop (MODE 2, not ping-pong)               wleft as rem, a_young (next block's halo issued)  -> vmcnt(wleft * LW [+ LAH])
  H2   the halo ping-pong loop (9-tap period unrolled)     tap, first / last block of the slice              -> vmcnt(PWG) | vmcnt(0)
  A    the A-stationary persistent loop (igemm_astat.hip)  first tile / later tile / last k-tile of the run  -> vmcnt(PW [+ 16 | + EST]) | 0

A wrong N lets a fragment read see the ring slot's previous occupant - only when the DMA lands late, i.e. in a few fragments of a few
launches on a busy chip.  A screen launches one case N_LAUNCH times while a bandwidth-bound kernel runs on a second stream and the operands
rotate through copies (HBM on some launches, L2 on others), and compares every launch with a reference that no kernel computed:

  integer family   activations from {-1, 0, 1}, weights from {-1, 0, 1, 2}, small integer bias / row vector / residual, alpha 1 or 2, fp8
                   operands as the same integers with power-of-two scales.  |C| <= 2048 and sum |a||w| < 2^24 make every fp32 partial and
                   the fp16 store exact in any order (split-K slabs included): the reference is an int64 matmul / conv in torch, compared
                   with torch.equal.  Rows are drawn from small pools (row m = pool row m % P), so the reference is a small int64 product
                   expanded by index; the two exactness conditions are checked over the pools, i.e. over every output.
  normal family    unit-normal fp16 operands (another power draw, another clock): launch 0 - before the second stream starts - is gated per
                   element against fp64 by tilecheck's bound, every later launch must reproduce its bits; where the project already asserts
                   bit identity between tiles (halo tile | gather tile 9, tile 21 | 9) those bits are compared too.
  extended epilogues and the A-stationary tiles (LayerNorm fold, GEGLU, row statistics, MX-fp8 copy-out: not exact in integers)
                   the bits of the same problem on streaming tile 9 at split-K 1 before the second stream starts - the identity
                   test_gemm_a_stationary_* asserts.  Tile 9 itself is screened in plain form against integers.

The attention, ctx-attention and MX-fp8 attention kernels drain with __syncthreads() at every tile and hold no counted wait: out of scope.

  tiles / pingpong / structure   the tile table from pbe_tile_info (never mirrored by hand) and which loop a tile runs
  CASES / plan / branches        the case table; the host planners' answer for a case; the wait branches its slices drive
  universe                       every (structure, depth, branch) that exists, from pbe_tile_info and the loops' branch models
  operands / reference / exactness   host operands of the integer and normal families, int64 (fp64) references, the two conditions
  screen / diagnose              N launches under the hog; for the first wrong one: workgroup tiles, 16x16 fragments and - integer family -
                                 the pair of k-tiles (t, t') sharing a slot with got - want = P(t') - P(t)
  mutant_lib                     the positive control: -DPBE_RACE_MUTANT=1 | 2 | 3 builds, cached on the source hash
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import shutil
import time

import torch
import torch.nn.functional as F

import convlattice as cl
import tilecheck as tc

N_LAUNCH = 60
F_DENSE, F_CONV, F_HALO, F_EX, F_F8, F_ASTAT, F_FORCED = 1, 2, 4, 8, 16, 32, 64
HOG_BYTES = 768 << 20           # three times the 256 MiB Infinity Cache
COPIES = 4                      # operand copies a case rotates through, two launches each: the first from HBM, the second from L2
PA, PW = 251, 127               # rows of the activation / weight pools (primes: no alignment with a tile)
ROOT = tc.ROOT


# ---- the tile table ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiles():
    """[dict(bm, bn, nwm, nwn, s, forms, hpa, slots)] by tile index, from pbe_tile_info."""
    from pbe_amd import lib
    h, out, rows = lib.load(), (C.c_int32 * 8)(), []
    while h.pbe_tile_info(len(rows), out) == 0:
        rows.append(dict(zip(("bm", "bn", "nwm", "nwn", "s", "forms", "hpa", "slots"), map(int, out))))
    assert rows, "pbe_tile_info returned no tile"
    return rows


def pingpong(t) -> bool:
    """launch_cfg's own condition for the ping-pong halo loop: weight ring of 3 and (BM / NWM / 16) (BN / NWN / 16) >= 16 MFMAs per k-step."""
    return bool(t["forms"] & F_HALO) and t["s"] == 3 and (t["bm"] // t["nwm"] // 16) * (t["bn"] // t["nwn"] // 16) >= 16


def structure(tile: int) -> str:
    t = tiles()[tile]
    if t["forms"] & F_ASTAT:
        return "A"
    if t["forms"] & F_HALO:
        return "H2" if pingpong(t) else "H1"
    return "R"


def tiles_of(form: int):
    return [i for i, t in enumerate(tiles()) if t["forms"] & form]


# ---- branch models: which wait a slice of a given length takes ---------------------------------------------------------------------------
def ring_branches(depth: int, nk: int):
    """R: the values of min(nk - 1 - kt, D - 1) over a slice of nk k-tiles."""
    return {("R", depth, f"rem{min(j, depth - 1)}") for j in range(nk)}


def halo_branches(depth: int, nblk: int):
    """H1: (wleft, a_young) over a slice of nblk channel blocks (9 taps each)."""
    out, nk2 = set(), 9 * nblk
    for blk in range(nblk):
        for tap in range(9):
            wleft = min(nk2 - 1 - (9 * blk + tap), depth - 1)
            young = blk + 1 < nblk and 1 <= tap <= depth
            out.add(("H1", depth, f"wleft{wleft}{'+halo' if young else ''}"))
    return out


def pingpong_branches(nblk: int):
    """H2: per block of the slice (first: queues start empty; last: no tile issued at taps 7, 8, group 1 fetches no halo) and tap."""
    out = set()
    for blk in range(nblk):
        which = ("first" if blk == 0 else "") + ("last" if blk == nblk - 1 else "") or "middle"
        out |= {("H2", 2, f"{which}:tap{tap}") for tap in range(9)}
    return out


def astat_branches(form: int, run: int):
    """A: the waits of a run of `run` column tiles (5 k-tiles each): the first tile's two, a later tile's first two (the previous epilogue's
    stores in the queue), the plain ones and the run's last k-tile."""
    out = {("A", form, "first:kt0"), ("A", form, "first:kt1"), ("A", form, "plain"), ("A", form, "last")}
    if run > 1:
        out.add(("A", form, "later:kt0-1"))
    return out


def astat_run(M: int, N: int, bn: int) -> int:
    """igemm_astat.hip launch_regs: the longest run of column tiles that still gives every CU its two workgroups."""
    tm, tn = M // 128, N // bn
    run = tn
    while run > 1 and (tm * (tn // run) < 512 or tn % run):
        run -= 1
    return run


def universe():
    """Every (structure, depth or form, branch) the four loops hold, from pbe_tile_info and the models above."""
    out = set()
    for i, t in enumerate(tiles()):
        st, d = structure(i), t["s"] - 1
        if st == "R":
            out |= ring_branches(d, d + 1)
        elif st == "H1":
            out |= halo_branches(d, 1) | halo_branches(d, 2)
        elif st == "H2":
            out |= pingpong_branches(1) | pingpong_branches(2) | pingpong_branches(3)
        else:
            for form in ((0,) if t["bn"] == 128 else (0, 1, 2)):          # pbe_launch_astat: tile 19 runs the GEGLU form only
                out |= astat_branches(form, 1) | astat_branches(form, 2)
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
class Case:
    """kind gemm: M, N, K (fp8: in bytes), k1 (two sources), splits, f8, epi (alpha 2 + row vector + residual), family.
    kind conv: B, H, W, C1, C2, Cout, stride, ups, kblock, splits, epi, family.  kind ex: form ln_geglu | qkv | stats | mx8, M (K = 320)."""

    def __init__(self, cid, kind, tile, **p):
        self.id, self.kind, self.tile, self.n = cid, kind, tile, N_LAUNCH
        self.struct = structure(tile)
        self.splits, self.family, self.epi, self.f8, self.k1, self.kblock, self.C2, self.stride, self.ups = 1, "int", False, False, 0, 64, 0, 1, 0
        self.__dict__.update(p)
        self.t = tiles()[tile]
        self.S = self.t["s"]

    @property
    def kw(self):                   # k-values per k-tile
        return 128 if self.f8 else 64

    def __repr__(self):
        return self.id


def _grid_rows(t, col_tiles: int, rounds: int = 2, cap: int = 1 << 16) -> int:
    """Rows for at least `rounds` rounds of workgroups over 256 CUs at `col_tiles` column tiles (capped)."""
    wgs = rounds * 256 * t["slots"]
    return min(cap, -(-wgs // col_tiles) * t["bm"])


def _rows_for_ws(t, N: int, splits: int, rows: int) -> int:
    """Split-K slabs must fit the 64 MiB workspace: the largest whole-tile row count <= rows with splits * M * N * 4 bytes inside it."""
    from pbe_amd import ops
    fit = ops.SPLITK_WS_BYTES // (4 * splits * N) // t["bm"] * t["bm"]
    return max(t["bm"], min(rows, fit))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    T = tiles()
    # R, dense: every tile, nk per slice in {1, 2, S - 1, S, S + 1, 2S + 1, 40}; ragged last k-tile; A | A2 seam inside a k-tile; a split-K
    # slice shorter than D (21 k-tiles in 5 slices: 5, 5, 5, 5, 1); tile 21 with M = 8 rows past a tile: the last waves' pieces are clamped
    for i in tiles_of(F_DENSE):
        t, S = T[i], T[i]["s"]
        N = 2 * t["bn"]
        M = _grid_rows(t, 2)
        for nk in sorted({1, 2, S - 1, S, S + 1, 2 * S + 1, 40}):
            out.append(Case(f"R-dense-t{i}-nk{nk}", "gemm", i, M=M, N=N, K=64 * nk, epi=nk == S + 1))
        out.append(Case(f"R-dense-t{i}-ragged", "gemm", i, M=M, N=N, K=64 * (S + 2) - 24))
        out.append(Case(f"R-dense-t{i}-seam", "gemm", i, M=M, N=N, K=64 * (S + 2), k1=96))
        if S > 2:
            out.append(Case(f"R-dense-t{i}-split5", "gemm", i, M=_rows_for_ws(t, N, 5, M), N=N, K=64 * 21, splits=5))
        out.append(Case(f"R-dense-t{i}-normal", "gemm", i, M=M, N=N, K=64 * (2 * S + 1), family="normal"))
        if t["forms"] & F_FORCED:
            out.append(Case(f"R-dense-t{i}-clamp", "gemm", i, M=M + 8, N=N, K=64 * (2 * S + 1)))
    # R, gather conv: every gather tile on a stride-1 32x32 map with 1, 2, 3 channel blocks; kblock 128; split-K resuming inside a block
    # (27 k-tiles in 2 slices: the second starts at block 1, tap 5); stride 2 and fused upsample on one tile per ring depth
    per_depth = {}
    for i in tiles_of(F_CONV):
        t = T[i]
        per_depth.setdefault(t["s"], i)
        Cout = 2 * t["bn"]
        B = max(2, _grid_rows(t, 2) // 1024)
        for c in (64, 128, 192):                 # (the 8-wave tiles with one tile in flight cover ~1 us of latency per k-tile: at 128 channels the
            cold = 4 if c == 128 and t["slots"] == 1 and t["s"] == 2 else 1      #  four operand copies outgrow the Infinity Cache, every launch reads HBM)
            out.append(Case(f"R-conv-t{i}-c{c}", "conv", i, B=B * cold, H=32, W=32, C1=c, Cout=Cout, epi=c == 128))
        cold = 4 if t["slots"] == 1 and t["s"] == 2 else 1
        out.append(Case(f"R-conv-t{i}-cat", "conv", i, B=B * cold, H=32, W=32, C1=64, C2=64, Cout=Cout))      # (block 1 = the second source: first touched at k-tile 9)
        out.append(Case(f"R-conv-t{i}-kb128", "conv", i, B=B, H=32, W=32, C1=128, Cout=Cout, kblock=128))
        out.append(Case(f"R-conv-t{i}-split2", "conv", i, B=max(2, _rows_for_ws(t, Cout, 2, B * 1024) // 1024), H=32, W=32, C1=192, Cout=Cout, splits=2))
    for S, i in sorted(per_depth.items()):
        t = T[i]
        B = max(2, _grid_rows(t, 2) // 1024)
        out.append(Case(f"R-conv-t{i}-stride2", "conv", i, B=B, H=64, W=64, C1=128, Cout=2 * t["bn"], stride=2))
        out.append(Case(f"R-conv-t{i}-ups", "conv", i, B=B, H=16, W=16, C1=128, Cout=2 * t["bn"], ups=1))
    # R, fp8 operands: k-tiles of 128 bytes
    for i in tiles_of(F_F8):
        t = T[i]
        for nk in (1, 2, 3, 9):
            out.append(Case(f"R-f8-t{i}-nk{nk}", "gemm", i, M=_grid_rows(t, 2), N=2 * t["bn"], K=128 * nk, f8=True, epi=nk == 3))
    # R, extended epilogues on one tile per width and depth (K = 320: 5 k-tiles): reference = tile 9's bits
    for i in (3, 9, 15, 18):
        assert T[i]["forms"] & F_EX
        for form in ("ln_geglu", "qkv", "stats", "mx8"):
            out.append(Case(f"R-ex-t{i}-{form}", "ex", i, form=form, M=_grid_rows(T[i], 8, cap=16384)))
    # H1 / H2: every halo tile at 1, 2, 3 channel blocks (first = last block; a_young; both), two sources, split-K at a block boundary (3 blocks
    # in 2 slices: the second starts at block 2), several whole 8x8 images per tile, and the normal family against gather tile 9
    for i in tiles_of(F_HALO):
        t = T[i]
        Cout = 2 * t["bn"]
        B = max(2, _grid_rows(t, 2) // 1024)
        for c in (64, 128, 192):
            out.append(Case(f"{structure(i)}-halo-t{i}-c{c}", "conv", i, B=B, H=32, W=32, C1=c, Cout=Cout, epi=c == 128))
        out.append(Case(f"{structure(i)}-halo-t{i}-cat", "conv", i, B=B, H=32, W=32, C1=64, C2=128, Cout=Cout))
        out.append(Case(f"{structure(i)}-halo-t{i}-split2", "conv", i, B=max(2, _rows_for_ws(t, Cout, 2, B * 1024) // 1024), H=32, W=32, C1=192, Cout=Cout, splits=2))
        if t["hpa"] >= (t["bm"] // 64) * 91:
            out.append(Case(f"{structure(i)}-halo-t{i}-8x8", "conv", i, B=B * 16, H=8, W=8, C1=128, Cout=Cout))
        out.append(Case(f"{structure(i)}-halo-t{i}-normal", "conv", i, B=B, H=32, W=32, C1=128, Cout=Cout, family="normal"))
    # A: tiles 19 / 20 GEGLU (form 0), tile 20 q | k | V^T (form 1) and its MX-fp8 copy-out (form 2); M = 1280: runs of one tile on a ragged
    # share of the chip, M = 16384: runs of four on a full one
    for i in tiles_of(F_ASTAT):
        for M in (1280, 16384):
            out.append(Case(f"A-t{i}-geglu-M{M}", "ex", i, form="ln_geglu", M=M))
        if T[i]["bn"] == 160:                    # (6 column tiles: only from M = 32768 on does a workgroup run more than one of them)
            for M in (1280, 16384, 32768):
                out.append(Case(f"A-t{i}-qkv-M{M}", "ex", i, form="qkv", M=M))
                out.append(Case(f"A-t{i}-mx8-M{M}", "ex", i, form="mx8", M=M))
    assert len({c.id for c in out}) == len(out)
    return out


def case(cid) -> Case:
    return next(c for c in cases() if c.id == cid)


# ---- host planners ---------------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20
EX_K, EX_TOK = 320, 256


def ex_dims(cs: Case):
    """(N, heads, head dim, inner) of an extended-epilogue case: the GEGLU projection 320 -> 2560, the row-statistics GEMM 320 -> 320, the
    q | k | V^T projection with inner = 320 (8 heads of 40) - or, for the MX copy-out on 128-column tiles, 640 (4 heads of 160: every
    128-column boundary then falls on a 32-element block)."""
    if cs.form == "ln_geglu":
        return 2560, 0, 0, 0
    if cs.form == "stats":
        return EX_K, 0, 0, 0
    inner, heads, D = (640, 4, 160) if cs.form == "mx8" and cs.t["bn"] == 128 else (320, 8, 40)
    return 3 * inner, heads, D, inner


def gemm_desc(cs: Case, ptr=lambda name: FAKE):
    """pbe_gemm_desc of a gemm / ex case (mx8: with its pbe_mx8_out_desc); ptr: name -> address."""
    from pbe_amd import lib, ops
    d = lib.GemmDesc()
    d.batch, d.alpha, d.tile_cfg, d.group_rows = 1, 1.0, -1, 1
    if cs.kind == "gemm":
        K1 = cs.k1 or cs.K
        d.A, d.W, d.C, d.bias = ptr("a"), ptr("w"), ptr("out"), ptr("bias")
        d.M, d.N, d.K, d.K1, d.lda, d.ldw, d.ldc = cs.M, cs.N, cs.K, K1, K1, cs.K, cs.N
        if cs.k1:
            d.A2, d.lda2 = ptr("a2"), cs.K - cs.k1
        if cs.epi:
            d.alpha, d.rowvec, d.ldv, d.group_rows, d.resid, d.ldr = 2.0, ptr("rowvec"), cs.N, 1024, ptr("resid"), cs.N
        if cs.f8:
            d.operand_dtype, d.a_scale, d.w_scale = 1, ptr("sa"), ptr("sw")
        else:
            d.workspace, d.workspace_bytes = ptr("ws"), ops.SPLITK_WS_BYTES
        return d, None
    N, heads, D, inner = ex_dims(cs)
    d.A, d.W, d.bias = ptr("a"), ptr("w"), ptr("bias")
    d.M, d.N, d.K, d.K1, d.lda, d.ldw = cs.M, N, EX_K, EX_K, EX_K, EX_K
    mx = None
    if cs.form == "stats":
        d.C, d.ldc, d.resid, d.ldr, d.rowvec, d.ldv, d.group_rows = ptr("out"), N, ptr("resid"), N, ptr("rowvec"), N, EX_TOK
        d.row_stats_out, d.row_stats_ld = ptr("stats"), cs.M
        return d, None
    d.ln_stats, d.ln_parts, d.ln_stats_ld, d.ln_colsum, d.ln_eps = ptr("ln"), 1, cs.M, ptr("colsum"), 1e-5
    if cs.form == "ln_geglu":
        d.C, d.ldc, d.act = ptr("out"), N // 2, ops.ACT_GEGLU
    else:
        d.alpha, d.alpha_cols, d.vt_col0, d.vt_tokens = 0.25, inner, 2 * inner, EX_TOK
        if cs.form == "qkv":
            d.C, d.ldc, d.VT, d.vt_bs, d.vt_rs = ptr("out"), 2 * inner, ptr("vt"), inner * EX_TOK, EX_TOK
        else:
            B = cs.M // EX_TOK
            mx = lib.Mx8OutDesc()
            mx.nranges, mx.channel_rows = 3, 0
            for r, (layout, name) in enumerate(((0, "q"), (0, "k"), (1, "v"))):
                mx.r[r] = lib.Mx8OutRange(ptr(name + "_data"), ptr(name + "_scale"), ops.MX8_VT if layout else ops.MX8_TOKENS, r * inner, 1.0, B, heads, EX_TOK, D)
    return d, mx


def conv_desc(cs: Case, ptr=lambda name: FAKE):
    from pbe_amd import lib, ops
    d = lib.Conv3x3Desc()
    d.X, d.Wp, d.Y, d.bias = ptr("x1"), ptr("wp"), ptr("out"), ptr("bias")
    d.X2 = ptr("x2") if cs.C2 else None
    if cs.epi:
        d.rowvec, d.ldv, d.resid = ptr("rowvec"), cs.Cout, ptr("resid")
    d.B, d.H, d.W, d.C1, d.C2, d.Cout = cs.B, cs.H, cs.W, cs.C1, cs.C2, cs.Cout
    d.stride, d.pad, d.upsample, d.act, d.kblock = cs.stride, 1, cs.ups, 0, cs.kblock
    d.workspace, d.workspace_bytes, d.tile_cfg = ptr("ws"), ops.SPLITK_WS_BYTES, -1
    return d


class forced:
    """ops.tune(1, tile | splits << 8) around a block; restores the heuristic, ops._FORCE_CFG and ops._PLANS."""

    def __init__(self, tile, splits=1, plans=False):
        self.value, self.plans = tile | (splits << 8), plans

    def __enter__(self):
        from pbe_amd import ops
        ops._FORCE_CFG = None
        ops._PLANS = [] if self.plans else None
        ops.tune(1, self.value)
        return ops

    def __exit__(self, *exc):
        from pbe_amd import ops
        ops.tune(1, -1)
        ops._FORCE_CFG, ops._PLANS = None, None
        return False


def conv_out(cs: Case):
    hv, wv = (cs.H << 1, cs.W << 1) if cs.ups else (cs.H, cs.W)
    return (hv - 1) // cs.stride + 1, (wv - 1) // cs.stride + 1


@functools.lru_cache(maxsize=None)
def plan(cs: Case):
    """dict(tile, splits, mode, slices): what the host planners answer for the case under its forced (tile, split-K); slices = the k-tiles
    (halo tiles: channel blocks) of each split-K slice as (first, count)."""
    from pbe_amd import lib, ops
    h = lib.load()
    with forced(cs.tile, cs.splits):
        if cs.kind == "conv":
            out = (C.c_int32 * 32)()
            lib.check(h.pbe_conv3x3_prologue(C.byref(conv_desc(cs)), out), cs.id)
            pro = dict(zip(cl.NAMES, map(int, out)))
            units = (cs.C1 + cs.C2) // 64 if pro["mode"] == 2 else 9 * (cs.C1 + cs.C2) // 64
            tile, splits, mode, per = pro["tile"], pro["splits"], pro["mode"], pro["split_per"]
        else:
            d, mx = gemm_desc(cs)
            tile, splits = ops._plan("mx8" if mx is not None else "gemm", d, mx)[:2]
            units, mode = -(-(cs.K if cs.kind == "gemm" else EX_K) // cs.kw), 0
            per = -(-units // max(1, splits))
    splits = max(1, splits)
    slices = [(k0, min(per, units - k0)) for k0 in range(0, units, per)] if splits > 1 else [(0, units)]
    assert len(slices) == splits, (cs.id, slices, splits)
    return dict(tile=tile, splits=splits, mode=mode, slices=slices)


def branches(cs: Case):
    """The wait branches the case's slices drive, from the planners' answer and the tile's ring depth."""
    pl, d, out = plan(cs), cs.S - 1, set()
    if cs.struct == "A":
        N = ex_dims(cs)[0]
        return astat_branches({"ln_geglu": 0, "qkv": 1, "mx8": 2}[cs.form], astat_run(cs.M, N, cs.t["bn"]))
    for _, cnt in pl["slices"]:
        out |= ring_branches(d, cnt) if cs.struct == "R" else halo_branches(d, cnt) if cs.struct == "H1" else pingpong_branches(cnt)
    return out


# ---- operands and references (host) ------------------------------------------------------------------------------------------------------
def _gen(cs: Case):
    return torch.Generator().manual_seed(tc.seed_of(cs.id))


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


def gemm_pools(cs: Case):
    """Pools of a gemm case: a [PA, K], w [PW, K], bias [PW], sa [PA], sw [PW], rowvec [3, PW], resid [PA, PW]; row m of A is pool row m % PA,
    row n of W pool row n % PW, the row vector of group g pool row g % 3.  int64 (integer family) or fp16 values as fp64 (normal family)."""
    g = _gen(cs)
    if cs.family == "int":
        p = dict(a=_ints(g, -1, 1, (PA, cs.K)), w=_ints(g, -1, 2, (PW, cs.K)), bias=_ints(g, -3, 3, (PW,)),
                 rowvec=_ints(g, -2, 2, (3, PW)), resid=_ints(g, -4, 4, (PA, PW)))
        p["sa"] = 2.0 ** _ints(g, 0, 1, (PA,)).double() if cs.f8 else torch.ones(PA, dtype=torch.float64)
        p["sw"] = 2.0 ** -_ints(g, 0, 1, (PW,)).double() if cs.f8 else torch.ones(PW, dtype=torch.float64)
        return p
    rn = lambda shape, s=1.0: (torch.randn(shape, generator=g) * s).half().double()
    return dict(a=rn((PA, cs.K)), w=rn((PW, cs.K), 1 / math.sqrt(cs.K)), bias=(torch.randn(PW, generator=g) * 0.5).double(), rowvec=rn((3, PW)),
                resid=rn((PA, PW)), sa=torch.ones(PA, dtype=torch.float64), sw=torch.ones(PW, dtype=torch.float64))


def gemm_reference(cs: Case, p):
    """(pre [PA, 3, PW], final [PA, 3, PW]) over the pools: the value stored before the residual and the stored output, exact int64 as fp64
    for the integer family; (pre, final, bound) with tilecheck's per-element bound for the normal family."""
    alpha = 2.0 if cs.epi else 1.0
    if cs.family == "int":
        acc = (p["a"] @ p["w"].t()).double()
        pre = acc * p["sa"][:, None] * p["sw"][None, :] * alpha + p["bias"].double()[None, :]
        pre = pre[:, None, :] + (p["rowvec"].double()[None] if cs.epi else torch.zeros(1, 3, PW, dtype=torch.float64))
        return pre, pre + (p["resid"].double()[:, None, :] if cs.epi else 0.0)
    acc, S = p["a"] @ p["w"].t(), p["a"].abs() @ p["w"].abs().t()
    want, bound = tc.expect(acc, S, cs.K, bias=p["bias"])
    bound = tc.clamp_to_close(want, bound, tc.CLOSE["gemm"])
    return want[:, None, :].expand(PA, 3, PW), want[:, None, :].expand(PA, 3, PW), bound[:, None, :].expand(PA, 3, PW)


def conv_pools(cs: Case):
    """x [2, H, W, Cin] (sample b = pool image b % 2), w [PWc, Cin, 3, 3] (output channel n = pool row n % PWc), bias, rowvec [2, PWc], resid."""
    g = _gen(cs)
    Cin, Ho, Wo = cs.C1 + cs.C2, *conv_out(cs)
    pw = min(cs.Cout, 80)
    if cs.family == "int":
        return dict(x=_ints(g, -1, 1, (2, cs.H, cs.W, Cin)), w=_ints(g, -1, 2, (pw, Cin, 3, 3)), bias=_ints(g, -3, 3, (pw,)),
                    rowvec=_ints(g, -2, 2, (2, pw)), resid=_ints(g, -4, 4, (2, Ho, Wo, pw)))
    rn = lambda shape, s=1.0: (torch.randn(shape, generator=g) * s).half().double()
    return dict(x=rn((2, cs.H, cs.W, Cin)), w=rn((pw, Cin, 3, 3), 1 / math.sqrt(9 * Cin)), bias=(torch.randn(pw, generator=g) * 0.5).double(),
                rowvec=rn((2, pw)), resid=rn((2, Ho, Wo, pw)))


def conv_reference(cs: Case, p):
    """(pre, final [, bound]) [2, Ho, Wo, PWc] over the pools: int64 F.conv2d (integer family) or fp64 with the per-element bound."""
    x = p["x"].permute(0, 3, 1, 2)
    if cs.ups:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    nhwc = lambda v: v.permute(0, 2, 3, 1)
    if cs.family == "int":
        pre = nhwc(F.conv2d(x, p["w"], stride=cs.stride, padding=1)).double() + p["bias"].double()
        if cs.epi:
            pre = pre + p["rowvec"].double()[:, None, None, :]
        return pre, pre + (p["resid"].double() if cs.epi else 0.0)
    acc, S = nhwc(F.conv2d(x, p["w"], stride=cs.stride, padding=1)), nhwc(F.conv2d(x.abs(), p["w"].abs(), stride=cs.stride, padding=1))
    sh = acc.shape
    want, bound = tc.expect(acc.reshape(-1, sh[-1]), S.reshape(-1, sh[-1]), 9 * (cs.C1 + cs.C2), bias=p["bias"])
    bound = tc.clamp_to_close(want, bound, tc.CLOSE["conv"])
    return want.view(sh), want.view(sh), bound.view(sh)


def exactness(cs: Case):
    """(largest |value| stored as fp16, before or after the residual; upper bound of sum |a||w| along K) of an integer case - over the pools,
    i.e. over every output element.  Exact when the first is <= 2048 and the second < 2^24."""
    assert cs.family == "int" and cs.kind in ("gemm", "conv")
    p = gemm_pools(cs) if cs.kind == "gemm" else conv_pools(cs)
    pre, fin = (gemm_reference if cs.kind == "gemm" else conv_reference)(cs, p)
    if cs.kind == "gemm":
        s = int((p["a"].abs() @ p["w"].abs().t()).max())
    else:
        x = p["x"].permute(0, 3, 1, 2)
        s = int(F.conv2d((x.repeat_interleave(2, 2).repeat_interleave(2, 3) if cs.ups else x).abs(), p["w"].abs(), stride=cs.stride, padding=1).max())
    return float(max(pre.abs().max(), fin.abs().max())), s


# ---- k-tiles of the integer family, for the diagnosis --------------------------------------------------------------------------------------
class KTiles:
    """Per k-tile operands of one workgroup tile of an integer case: a(t) [rows, kw], w(t) [cols, kw] int64, in the kernel's K order."""

    def __init__(self, cs: Case, pools, rows, cols):
        self.cs, self.rows, self.cols = cs, rows, cols
        if cs.kind == "gemm":
            self.A, self.Wm = pools["a"][rows % PA], pools["w"][cols % PW]
        else:
            Cin, (Ho, Wo) = cs.C1 + cs.C2, conv_out(cs)
            pw = pools["w"].shape[0]
            self.Wm = cl.pack_k(pools["w"].reshape(pw, Cin, 9), cs.kblock)[cols % pw]
            b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
            self.b, self.oy, self.ox, self.x = b % 2, rem // Wo, rem % Wo, pools["x"]

    def a(self, t):
        cs = self.cs
        if cs.kind == "gemm":
            out = torch.zeros(len(self.rows), cs.kw, dtype=torch.int64)
            blk = self.A[:, t * cs.kw:(t + 1) * cs.kw]
            out[:, :blk.shape[1]] = blk
            return out
        KB = cs.kblock // 64
        cblk, r = divmod(t, 9 * KB)
        tap, kj = divmod(r, KB)
        c0 = cblk * cs.kblock + kj * 64
        iy, ix = self.oy * cs.stride - 1 + tap // 3, self.ox * cs.stride - 1 + tap % 3
        ok = (iy >= 0) & (iy < cs.H << cs.ups) & (ix >= 0) & (ix < cs.W << cs.ups)
        v = self.x[self.b, (iy >> cs.ups).clamp(0, cs.H - 1), (ix >> cs.ups).clamp(0, cs.W - 1), c0:c0 + 64]
        return torch.where(ok[:, None], v, torch.zeros((), dtype=torch.int64))

    def w(self, t):
        out = torch.zeros(len(self.cols), self.cs.kw, dtype=torch.int64)
        blk = self.Wm[:, t * self.cs.kw:(t + 1) * self.cs.kw]
        out[:, :blk.shape[1]] = blk
        return out


class Diagnosis:
    def __init__(self, tiles_, frags, stale, note="", tile=None):
        self.tiles, self.frags, self.stale, self.note, self.tile = tiles_, frags, stale, note, tile

    def __str__(self):
        s = f"workgroup tiles (m, n) {self.tiles[:4]}{'...' if len(self.tiles) > 4 else ''} ({len(self.tiles)}), 16x16 fragments of tile {self.tile} {self.frags[:6]}{'...' if len(self.frags) > 6 else ''} ({len(self.frags)})"
        if self.stale:
            s += f", stale slot: k-tile {self.stale[0]} read as k-tile {self.stale[1]} ({self.stale[2]})"
        return s + (f", {self.note}" if self.note else "")


def diagnose(cs: Case, got, want, pools=None):
    """got, want: [rows, columns] on the host.  The workgroup tiles and the 16x16 fragments of the first that differ; with the integer pools
    also the pair (t, t') of k-tiles of one slice sharing a ring slot (t' = t - j S) with got - want = P(t') - P(t) on every differing
    fragment, where P substitutes k-tile t' for t in both operands or one, in the whole k-tile or one k-step half, row by row."""
    bm, bn = cs.t["bm"], cs.t["bn"]
    bad = (got != want) | ~torch.isfinite(got.float())
    if not bool(bad.any()):
        return None
    r, c = bad.nonzero(as_tuple=True)
    ntn = -(-got.shape[1] // bn)
    ids, cnt = torch.unique((r // bm) * ntn + c // bn, return_counts=True)
    wg = [divmod(int(i), ntn) for i in ids]
    first = None
    for j in torch.argsort(cnt, stable=True)[:12].tolist():       # the tiles with the fewest wrong elements first: likeliest to hold ONE early read
        d = _diagnose_tile(cs, got, want, pools, bad, wg, *wg[j])
        first = first or d
        if d.stale:
            return d
    return first


def _diagnose_tile(cs: Case, got, want, pools, bad, wg, tm, tn):
    bm, bn = cs.t["bm"], cs.t["bn"]
    r, c = bad[tm * bm:(tm + 1) * bm, tn * bn:(tn + 1) * bn].nonzero(as_tuple=True)
    frags = sorted(set(zip((r // 16).tolist(), (c // 16).tolist())))
    if pools is None or cs.family != "int":
        return Diagnosis(wg, frags, None, tile=(tm, tn))
    rows = torch.arange(tm * bm, min((tm + 1) * bm, got.shape[0]))
    cols = torch.arange(tn * bn, min((tn + 1) * bn, got.shape[1]))
    g = got[rows][:, cols].double()
    if not bool(torch.isfinite(g).all()):
        return Diagnosis(wg, frags, None, "non-finite values", (tm, tn))
    scale = 2.0 if cs.epi and cs.kind == "gemm" else 1.0         # (alpha 2 of the gemm cases; a conv has none)
    if cs.kind == "gemm":
        scale = scale * pools["sa"][rows % PA][:, None] * pools["sw"][cols % PW][None, :]
    delta = (g - want[rows][:, cols].double()) / scale
    kt = KTiles(cs, pools, rows, cols)
    per = 9 if plan(cs)["mode"] == 2 else 1                      # halo tiles slice in channel blocks of 9 k-tiles
    half = cs.kw // 2
    cuts = {"k-tile": slice(0, cs.kw), "k-step 0": slice(0, half), "k-step 1": slice(half, cs.kw)}
    # A DMA lands row by row (one 128-byte line each), so a stale read may hold single rows of either operand: a differing element must
    # equal one of the substitutions AT THAT ELEMENT; a fragment is explained when all its differing elements (at least 4) do
    tbad = bad[rows][:, cols]
    fsl = {f: (slice(f[0] * 16, f[0] * 16 + 16), slice(f[1] * 16, f[1] * 16 + 16)) for f in frags}
    best = None
    for first, cnt in plan(cs)["slices"]:
        for t in range(first * per, (first + cnt) * per):
            for tp in [x for x in (t - cs.S, t - 2 * cs.S) if x >= first * per]:
                a, w, ap, wp = kt.a(t), kt.w(t), kt.a(tp), kt.w(tp)
                names, cands = [], []
                for cname, cut in cuts.items():
                    base = a[:, cut] @ w[:, cut].t()
                    names += [f"both operands, {cname}", f"weights, {cname}", f"activations, {cname}"]
                    cands += [ap[:, cut] @ wp[:, cut].t() - base, a[:, cut] @ wp[:, cut].t() - base, ap[:, cut] @ w[:, cut].t() - base]
                eq = (torch.stack(cands).double() == delta[None]) & tbad[None]
                match = eq.any(0)
                okf = [f for f, (rs_, cs_) in fsl.items() if int(tbad[rs_, cs_].sum()) >= 4 and bool((match[rs_, cs_] == tbad[rs_, cs_]).all())]
                if okf and (best is None or len(okf) > len(best[0])):
                    region = torch.zeros_like(tbad)
                    for f in okf:
                        region[fsl[f]] = True
                    best = (okf, t, tp, names[int((eq & region[None]).sum((1, 2)).argmax())])
                if len(okf) == len(frags):
                    return Diagnosis(wg, frags, best[1:], tile=(tm, tn))
    if best is not None:
        return Diagnosis(wg, frags, best[1:], f"{len(best[0])} of {len(frags)} fragments; the others hold more than one early read", (tm, tn))
    return Diagnosis(wg, frags, None, "no pair of k-tiles sharing a slot explains the difference", (tm, tn))


def emulate_stale(cs: Case, want, pools, tm, tn, t, mode, which):
    """want [rows, columns] with workgroup tile (tm, tn) as a stale-slot read leaves it: k-tile t - S in place of k-tile t, in both operands of
    k-step half `which` (mode "half") or in the activations of the 16-row fragment `which` (mode "frag")."""
    bm, bn = cs.t["bm"], cs.t["bn"]
    rows = torch.arange(tm * bm, min((tm + 1) * bm, want.shape[0]))
    cols = torch.arange(tn * bn, min((tn + 1) * bn, want.shape[1]))
    kt = KTiles(cs, pools, rows, cols)
    a, w, ap, wp = kt.a(t), kt.w(t), kt.a(t - cs.S), kt.w(t - cs.S)
    if mode == "half":
        cut = slice(which * cs.kw // 2, (which + 1) * cs.kw // 2)
        delta = ap[:, cut] @ wp[:, cut].t() - a[:, cut] @ w[:, cut].t()
    else:
        delta = torch.zeros(len(rows), len(cols), dtype=torch.int64)
        rs = slice(which * 16, which * 16 + 16)
        delta[rs] = (ap[rs] - a[rs]) @ w.t()
    scale = 2.0 if cs.epi and cs.kind == "gemm" else 1.0         # (alpha 2 of the gemm cases; a conv has none)
    if cs.kind == "gemm":
        scale = scale * pools["sa"][rows % PA][:, None] * pools["sw"][cols % PW][None, :]
    got = want.clone()
    got[rows[:, None], cols[None, :]] = (want[rows][:, cols].double() + delta.double() * scale).to(want.dtype)
    return got


def expand(cs: Case, ref, device="cpu"):
    """A pool reference ([PA, 3, PW] or [2, Ho, Wo, PWc]) as the full [rows, columns] output."""
    ref = ref.to(device)
    if cs.kind == "gemm":
        m, n = torch.arange(cs.M, device=device), torch.arange(cs.N, device=device)
        return ref[(m % PA)[:, None], ((m // 1024) % 3)[:, None], (n % PW)[None, :]]
    b, n = torch.arange(cs.B, device=device), torch.arange(cs.Cout, device=device)
    return ref[b % 2][..., n % ref.shape[-1]].reshape(-1, cs.Cout)


# ---- the GPU side: hog, launches, screen ---------------------------------------------------------------------------------------------------
class Hog:
    """A bandwidth-bound kernel on ONE side stream: an in-place multiply over a buffer larger than the Infinity Cache."""

    def __init__(self, dev, nbytes=HOG_BYTES):
        self.buf = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
        self.stream = torch.cuda.Stream(dev)

    def push(self, passes=2):
        with torch.cuda.stream(self.stream):
            for _ in range(passes):
                self.buf.mul_(1.0)

    def drain(self):
        self.stream.synchronize()


_HOGS = {}


def hog_of(dev) -> Hog:
    key = str(dev)
    if key not in _HOGS:
        _HOGS[key] = Hog(dev)
    return _HOGS[key]


def screen(launch, want, n, hog, diagnose=None):
    """n launches of launch(i) -> [device tensors], each compared on the device with want (a list of tensors of the same shapes) while the
    hog runs on its stream.  -> (wrong launches, diagnosis of the first wrong one: diagnose(i, got) or the launch index)."""
    wrong, first = 0, None
    try:
        for i in range(n):
            if hog is not None:
                hog.push()
            got = launch(i)
            if not all(torch.equal(g, w) for g, w in zip(got, want)):
                wrong += 1
                if first is None or (wrong <= 4 and diagnose is not None and not getattr(first, "stale", True)):
                    d = diagnose(i, got) if diagnose is not None else i          # (the first wrong launch - or, of the first four, the first
                    first = d if first is None or getattr(d, "stale", None) else first     #  whose stale slot can be named)
    finally:
        if hog is not None:
            hog.drain()
    return wrong, first


def _copies(t, dev):
    return [t.to(dev).clone() for _ in range(COPIES)]


def prepare(cs: Case, dev):
    """-> (launch(i) -> [outputs], want [tensors], diag(i, got) -> Diagnosis | None, gate() run once on launch 0's outputs or None).
    Everything a launch reads rotates through COPIES copies, two launches each; outputs are poisoned before every launch."""
    from pbe_amd import ops
    keep, outs = {}, []
    ws = ops._splitk_ws(dev)
    cp = (lambda i: i % COPIES) if cs.struct == "A" else (lambda i: (i // 2) % COPIES)      # (the L2-resident weights of A: cold on every launch)

    def poison():                                # a launch that stores nothing must not inherit the previous launch's correct output
        for o in outs:
            o.fill_(0xAA if o.dtype == torch.uint8 else float("nan"))

    if cs.kind in ("gemm", "conv"):
        pools = gemm_pools(cs) if cs.kind == "gemm" else conv_pools(cs)
        ref = (gemm_reference if cs.kind == "gemm" else conv_reference)(cs, pools)
        if cs.kind == "gemm":
            m, n = torch.arange(cs.M, device=dev) % PA, torch.arange(cs.N, device=dev) % PW          # (pools are expanded on the device)
            K1 = cs.k1 or cs.K
            if cs.f8:
                f8 = lambda v: v.float().to(torch.float8_e4m3fn).view(torch.uint8).to(dev)
                host = dict(a=f8(pools["a"])[m], w=f8(pools["w"])[n], sa=pools["sa"].float().to(dev)[m], sw=pools["sw"].float().to(dev)[n])
            else:
                a = pools["a"].half().to(dev)[m]
                host = dict(a=a[:, :K1].contiguous(), w=pools["w"].half().to(dev)[n])
                if cs.k1:
                    host["a2"] = a[:, K1:].contiguous()
            host["bias"] = pools["bias"].float().to(dev)[n]
            if cs.epi:
                g = torch.arange(-(-cs.M // 1024), device=dev) % 3
                host["rowvec"], host["resid"] = pools["rowvec"].half().to(dev)[g][:, n].contiguous(), pools["resid"].half().to(dev)[m][:, n].contiguous()
            shape = (cs.M, cs.N)
        else:
            b, n = torch.arange(cs.B, device=dev) % 2, torch.arange(cs.Cout) % pools["w"].shape[0]
            x, w = pools["x"].half().to(dev)[b], pools["w"][n].half()
            host = dict(x1=x[..., :cs.C1].contiguous(), wp=cl.pack_k(w.reshape(cs.Cout, cs.C1 + cs.C2, 9), cs.kblock).contiguous(), bias=pools["bias"][n].float())
            if cs.C2:
                host["x2"] = x[..., cs.C1:].contiguous()
            if cs.epi:
                host["rowvec"], host["resid"] = pools["rowvec"].half().to(dev)[b][:, n.to(dev)].contiguous(), pools["resid"].half().to(dev)[b][..., n.to(dev)].contiguous()
            shape = (cs.B * conv_out(cs)[0] * conv_out(cs)[1], cs.Cout)
        for k, v in host.items():
            keep[k] = _copies(v, dev)
        out = torch.empty(shape, dtype=torch.float16, device=dev)
        outs.append(out)

        def launch(i):
            poison()
            ptr = lambda name: (out if name == "out" else ws if name == "ws" else keep[name][cp(i)]).data_ptr()
            if cs.kind == "gemm":
                ops._launch("gemm", gemm_desc(cs, ptr)[0])
            else:
                ops._launch("conv", conv_desc(cs, ptr))
            return [out]

        if cs.family == "int":
            want_dev = expand(cs, ref[1], dev).half()
            want_host = None

            def diag(i, got):
                nonlocal want_host
                want_host = expand(cs, ref[1]).half() if want_host is None else want_host
                return diagnose(cs, got[0].cpu(), want_host, pools)
            return launch, [want_dev], diag, None

        def gate(got0):                          # launch 0 per element against fp64; the project's cross-tile identities
            want, bound = expand(cs, ref[1], dev), expand(cs, ref[2], dev)
            rep = tc.compare(got0[0], want, bound, cs.id)
            assert rep.ratio <= 1.0, str(rep)
            twin = None
            if cs.kind == "conv" and cs.struct != "R":
                twin = "conv"
            elif cs.kind == "gemm" and cs.t["forms"] & F_FORCED:
                twin = "gemm"
            if twin:
                mine = got0[0].clone()
                ops.tune(1, 9 | (1 << 8))
                launch(0)
                ops.tune(1, cs.tile | (cs.splits << 8))
                torch.cuda.synchronize(dev)
                assert torch.equal(mine, out), f"{cs.id}: launch 0 differs from tile 9's bits"
            return rep
        return launch, None, lambda i, got: diagnose(cs, got[0].cpu(), WANT0[cs.id][0].cpu()), gate

    # extended epilogues and the A-stationary tiles: unit-normal operands as test_gemm_a_stationary_* draws them
    N, heads, D, inner = ex_dims(cs)
    g = torch.Generator().manual_seed(tc.seed_of(cs.id))
    x = torch.randn(cs.M, EX_K, generator=g) * 1.3 + 0.4
    x[: cs.M // 4] += 6.0
    xd = x.half().to(dev)
    w, b = torch.randn(N, EX_K, generator=g) / EX_K ** 0.5, 0.1 * torch.randn(N, generator=g)
    if cs.form == "stats":
        host = dict(a=x.half(), w=w.half(), bias=b, resid=torch.randn(cs.M, N, generator=g).half(), rowvec=torch.randn(cs.M // EX_TOK, N, generator=g).half())
    else:
        gamma, beta = 1 + 0.1 * torch.randn(EX_K, generator=g), 0.1 * torch.randn(EX_K, generator=g)
        wg, c2, c1 = ops.pack_linear_ln(w, b, gamma, beta)
        st = ops.row_stats(xd)
        host = dict(a=x.half(), w=wg, bias=c2, colsum=c1, ln=st.buf)
    for k, v in host.items():
        keep[k] = _copies(v, dev)
    B = cs.M // EX_TOK
    if cs.form == "ln_geglu":
        named = dict(out=torch.empty(cs.M, N // 2, dtype=torch.float16, device=dev))
    elif cs.form == "stats":
        named = dict(out=torch.empty(cs.M, N, dtype=torch.float16, device=dev), stats=torch.empty(8, cs.M, 2, dtype=torch.float32, device=dev))
    elif cs.form == "qkv":
        named = dict(out=torch.empty(cs.M, 2 * inner, dtype=torch.float16, device=dev), vt=torch.empty(B, inner, EX_TOK, dtype=torch.float16, device=dev))
    else:
        named = {}
        for name, mode in (("q", ops.MX8_TOKENS), ("k", ops.MX8_TOKENS), ("v", ops.MX8_VT)):
            t = ops._mx8_target(mode, B, heads, EX_TOK, D, dev)
            named[name + "_data"], named[name + "_scale"] = t.data, t.scale
    outs.extend(named.values())

    def launch(i):
        poison()
        ptr = lambda name: (named[name] if name in named else keep[name][cp(i)]).data_ptr()
        d, mx = gemm_desc(cs, ptr)
        ops._launch("mx8" if mx is not None else "gemm", d, mx)
        return [v for k, v in named.items() if k != "stats"] + ([named["stats"][:-(-N // cs.t["bn"])]] if "stats" in named else [])

    def reference():                             # the same problem on streaming tile 9, split-K 1, before the hog starts
        with forced(9, 1, plans=True) as o:
            got = [v.clone() for v in launch(0)]
            assert o._PLANS[0][1] == 9, o._PLANS
        torch.cuda.synchronize(dev)
        return got
    return launch, reference, lambda i, got: diagnose(cs, got[0].reshape(cs.M, -1).cpu(), WANT0[cs.id][0].reshape(cs.M, -1).cpu()), None


WANT0 = {}


def run_case(cs: Case, dev, n=None, use_hog=True):
    """One case end to end -> dict(case, launches, wrong, diagnosis, seconds, plan).  The forced (tile, split-K) must be what ran."""
    from pbe_amd import ops
    t0 = time.time()
    plan(cs)                                     # (cached: diagnose must not query the planners inside the forced block below)
    launch, want, diag, gate = prepare(cs, dev)
    n = cs.n if n is None else n
    if callable(want):                           # tile 9's bits (for tile 9's own extended forms: an undisturbed launch of itself)
        ref = want()
        ex_stats = cs.form == "stats"
    with forced(cs.tile, cs.splits, plans=True) as o:
        if callable(want) or want is None:
            first = [v.clone() for v in launch(0)]
            torch.cuda.synchronize(dev)
            if want is None:
                gate(first)
                want = first
            else:                                # (the row-statistics partials depend on the column-tile width: this tile's own undisturbed launch)
                want = ref[:-1] + [first[-1]] if ex_stats else ref
            o._PLANS.clear()
        WANT0[cs.id] = want
        try:
            wrong, first_bad = screen(launch, want, n, hog_of(dev) if use_hog else None, diag)
            torch.cuda.synchronize(dev)
            ran = {(p[1], max(1, p[2])) for p in o._PLANS}
        finally:
            WANT0.pop(cs.id, None)
    assert ran == {(cs.tile, cs.splits)}, f"{cs.id}: the launches ran {ran}, not tile {cs.tile} split-K {cs.splits}"
    return dict(case=cs.id, launches=n, wrong=wrong, diagnosis=first_bad, seconds=time.time() - t0)


def report(line):
    """Append a line to racescreen_report.txt beside the parity report (committed copy: profiles/racescreen_report.txt)."""
    import test_model_gpu as parity
    path = os.path.join(os.path.dirname(parity.REPORT), "racescreen_report.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def report_line(res):
    return (f"{res['case']}: {res['wrong']} of {res['launches']} launches wrong, {res['seconds']:.2f} s"
            + (f" | first wrong launch: {res['diagnosis']}" if res["wrong"] else ""))


# ---- the positive control -------------------------------------------------------------------------------------------------------------------
MUTANTS = {1: ("R", ["igemm_dense.hip", "igemm_conv.hip", "igemm_f8.hip", "igemm_ex_ln.hip", "igemm_ex_st.hip", "igemm_ex_qkv.hip", "igemm_ex_all.hip"]),
           2: ("H", ["igemm_halo.hip"]), 3: ("A", ["igemm_astat.hip"])}


def mutant_lib(value: int) -> str:
    """libpbe_hip with -DPBE_RACE_MUTANT=value (build.build_diagnostic, at most 8 compile jobs), built once per source hash under build/."""
    from pbe_amd import build, lib
    path = os.path.join(ROOT, "build", "racescreen", f"libpbe_hip_mutant{value}_{lib.source_hash()}.so")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = path + f".{os.getpid()}.tmp"
        build.build_diagnostic([f"PBE_RACE_MUTANT={value}"], tmp, only=MUTANTS[value][1])
        os.replace(tmp, path)
        shutil.rmtree(tmp + ".obj", ignore_errors=True)
    return path


def shadowed(cs: Case):
    """Why NO contention can make a mutant show in this case, or None.  Read from the shipped kernels' ISA ("Race screens"): where
    the compiler itself puts `s_waitcnt vmcnt(0)` between a tile's DMA issue and the counted wait in front of its reads, the queue is empty
    when the counted wait runs and its immediate orders nothing - the mutant is the shipped program."""
    if cs.kind == "conv" and cs.struct == "R" and (cs.t["bm"], cs.t["bn"], cs.S) == (256, 320, 2):
        return ("gather conv 256x320: 182 spilled VGPRs; a scratch reload behind the k-tile's DMA pieces is awaited with vmcnt(0) before the "
                "MFMA block of every k-tile, so tile kt + 1 has landed an iteration before its counted wait")
    if cs.struct == "A" and cs.t["bn"] == 160:
        return ("A-stationary 160-column tile, all three forms: the compiler awaits vmcnt(0) right behind the DMA issue of k-tile 0 of every "
                "later column tile and behind the epilogue-vector loads of every k-tile 2 (form 0 also at each spilled-pointer reload of the "
                "epilogue); the two weight tiles left cross a whole epilogue before they are read")
    if cs.struct == "A" and astat_run(cs.M, ex_dims(cs)[0], cs.t["bn"]) == 1:
        return ("A-stationary run of one tile: the first use of the A fragments at k-tile 0 (behind W2's issue) and the epilogue vectors "
                "loaded at k-tile 2 (behind W4's issue) are awaited with vmcnt(0): W1 .. W4 have landed before their counted waits")
    return None


def mutant_cases(value: int):
    """The cases a mutant's child process runs: one integer case per tile of the structure whose slices hold the k-tile the mutant relaxes
    (the slice's tenth; mutant 3: the A-stationary cases, whose reference is tile 9 - which the mutant does not touch)."""
    if value == 1:
        return [c for c in cases() if c.id.startswith("R-dense") and c.id.endswith("-nk40")] + \
               [c for c in cases() if c.id.startswith("R-conv") and c.id.endswith("-cat")]
    if value == 2:
        return [c for c in cases() if c.struct in ("H1", "H2") and c.id.endswith("-c128")]
    return [c for c in cases() if c.struct == "A"]


if __name__ == "__main__":                       # the child of a mutant test: python racescreen.py <value> <out.json>, PBE_LIB_PATH set by the parent
    import json
    import sys
    value, dst = int(sys.argv[1]), sys.argv[2]
    sys.path.insert(0, ROOT)
    device = torch.device("cuda", 0)
    results = []
    for cs_ in mutant_cases(value):
        res_ = run_case(cs_, device)
        d_ = res_["diagnosis"]
        results.append(dict(case=res_["case"], shadowed=shadowed(cs_) or "", launches=res_["launches"], wrong=res_["wrong"], seconds=res_["seconds"], diagnosis=str(d_) if d_ else "",
                            stale=bool(d_ is not None and getattr(d_, "stale", None))))
        with open(dst, "w") as f_:
            json.dump(results, f_)
