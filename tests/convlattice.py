"""The gather conv lattice: helpers of test_convlattice_cpu.py and test_convlattice_gpu.py.  Not a conftest: plain functions only.

igemm_kernel<MODE 1> (pbe_amd/csrc/igemm_kernel.h) runs every 3x3 conv the halo-resident tiles refuse.  The lattice launches it per
element against fp64 on every tile that can run it (GATHER_TILES), at every geometry the entry point accepts (GEOS), at every K order
(kblock 64 / 128 / 192 / 256) and with split-K slices that resume in the middle of a channel block, on the smallest maps where each
hazard exists ("The gather conv lattice").

  Case / operands      one geometry with its channels; fp16 operands drawn on the host as tilecheck.run_conv draws them (unit-normal
                       activations, weights at 1 / sqrt(9 C)), from a generator seeded by the case id
  pack_k / packed      the weights in the header's K order k = ((ci / cb) * T + tap) * cb + ci % cb, written from that formula
                       (never ops.pack_conv3x3)
  reference            fp64 F.conv2d over every output element of every sample + the per-element bound: tilecheck.expect, then
                       clamp_to_close(CLOSE["conv"])
  emulate              an fp32 restatement of the kernel on the host: tap table, (block, tap, channel) walk in k-tiles of 64, split-K
                       resume, fp32 epilogue, fp16 store - and its mutants (MUTANTS), which the gate must reject
  prologue / slices    the host planner's answer for a forced (tile, split-K) and where each split-K slice resumes
  launch               (GPU) the descriptor filled directly, kblock included, through ops._launch under ops.tune(1, tile | splits << 8)
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os

import torch
import torch.nn.functional as F

import tilecheck as tc

GATHER_TILES = list(range(10)) + [15, 16, 17, 18]
KB_TILES = [0, 3, 6, 9, 17]
SPLIT_TILES = [0, 3, 6, 9]
FAKE = 1 << 20
NAMES = ["tile", "splits", "bm", "bn", "mode", "m_fast", "tdiv", "mg_tdiv", "split_per", "sv_ns", "sv_gdiv", "mg_sv_gdiv", "hw", "mg_hw", "mg_wo",
         "per_blk", "mg_per_blk", "mg_kb", "th", "hw2", "hps", "nsub", "rows", "tpi", "mg_tpi", "mh_hps", "mh_hw2", "lgw", "lgimg", "hpa",
         "off_tail", "off_last"]
PBE_EINVAL = -1

# id: B, H, W, C1, C2, Cout, stride, pad, upsample, rowvec, resid
GEOS = {
    "base":   (5, 9, 7, 128, 0, 328, 1, 1, 0, True, True),       # M = 315: two ragged m-tiles at BM 256, boundaries inside images at 64 / 128; hw = 63: !sv_ok
    "sv":     (8, 8, 8, 128, 0, 136, 1, 1, 0, True, True),       # hw = 64: svec with 1, 2, 4 samples per tile
    "cat":    (5, 9, 7, 64, 128, 136, 1, 1, 0, True, True),      # source switch c0 < C1, unequal pixel strides
    "scalar": (5, 9, 7, 128, 0, 100, 1, 1, 0, False, True),      # Cout % 8 != 0: scalar copy-out
    "s2p1":   (5, 10, 6, 128, 0, 136, 2, 1, 0, False, False),    # iy0 = 2 oy - 1
    "s2p0":   (5, 15, 13, 128, 0, 136, 2, 0, 0, False, False),   # the VAE's (0, 1, 0, 1) pad at odd sizes: the last window ends on the last row
    "s2p0e":  (5, 14, 12, 128, 0, 136, 2, 0, 0, False, False),   # the same at even sizes: the last row and column read zeros
    "s1p0":   (5, 9, 7, 128, 0, 136, 1, 0, 0, False, False),     # pad 0 at stride 1
    "ups":    (5, 6, 5, 128, 0, 136, 1, 1, 1, True, True),       # iy >> ups against Hv = 2 H, odd W
    "upscat": (5, 6, 5, 64, 64, 136, 1, 1, 1, False, False),     # fused upsample over two sources
    "phase":  (5, 6, 5, 128, 0, 328, 1, 1, 2, False, False),     # four phases in blockIdx.y, scatter to (2y + py, 2x + px)
}
# outside the lattice: a map the halo-resident tile 11 takes at kblock 64 (M = 512 = 4 tiles of 8 rows of 16, K = 2304)
OTHER_GEOS = {"halo11": (2, 16, 16, 256, 0, 136, 1, 1, 0, True, True),
              # and one whose copy-out can emit group statistics at 8 groups: hw = 256 is whole tiles at every BM, 16 channels per group divide every BN
              "gs": (2, 16, 16, 128, 0, 128, 1, 1, 0, True, True)}
# kblock lattice: (C1, C2, kblock) at each of KB_GEOS
KB_CHANNELS = [(256, 0, 128), (256, 0, 256), (192, 0, 192), (128, 128, 128)]
KB_GEOS = ["base", "s2p0", "ups"]


class Case:
    def __init__(self, geo, c1=None, c2=None):
        self.geo = geo
        self.B, self.H, self.W, C1, C2, self.Cout, self.stride, self.pad, self.ups, self.rowvec, self.resid = (GEOS.get(geo) or OTHER_GEOS[geo])
        self.C1, self.C2 = (C1, C2) if c1 is None else (c1, c2 or 0)
        self.Cin = self.C1 + self.C2
        self.phase = self.ups == 2
        hv, wv = (self.H << 1, self.W << 1) if self.ups else (self.H, self.W)
        extra = 2 if self.pad else 1
        self.Ho, self.Wo = (hv + extra - 3) // self.stride + 1, (wv + extra - 3) // self.stride + 1
        self.T = 4 if self.phase else 9
        self.K = self.T * self.Cin
        self.nk = self.K // 64
        self.M = self.B * self.Ho * self.Wo                       # output pixels (the phase form launches B H W rows per phase)
        self.groups = 8 if self.stride == 1 and self.Cout % 8 == 0 else 0
        self.id = f"{geo}:{self.C1}+{self.C2}"

    def label(self, m):
        b, r = divmod(m, self.Ho * self.Wo)
        return "%d:%d:%d" % (b, *divmod(r, self.Wo))


@functools.lru_cache(maxsize=None)
def case(geo, c1=None, c2=None) -> Case:
    return Case(geo, c1, c2)


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def phase_weights(w):
    """OIHW fp32 -> fp16 [4, Co, Ci, 4]: per output phase (py, px) the 3x3 taps that fall on one source pixel of the 2x2 block, summed in
    fp32 and rounded once (py = 0: ky {0} | {1, 2}; py = 1: ky {0, 1} | {2}; the same in x); tap = ty * 2 + tx."""
    sets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    out = []
    for py in (0, 1):
        for px in (0, 1):
            taps = [sum(w[:, :, ky, kx] for ky in sets[py][ty] for kx in sets[px][tx]) for ty in (0, 1) for tx in (0, 1)]
            out.append(torch.stack(taps, -1))
    return torch.stack(out, 0).half()


@functools.lru_cache(maxsize=None)
def operands(cs: Case):
    g = torch.Generator().manual_seed(tc.seed_of(cs.id))
    rn = lambda shape, scale=1.0: (torch.randn(shape, generator=g) * scale).half()
    t = {"x1": rn((cs.B, cs.H, cs.W, cs.C1)), "x2": rn((cs.B, cs.H, cs.W, cs.C2)) if cs.C2 else None}
    w = torch.randn(cs.Cout, cs.Cin, 3, 3, generator=g) / math.sqrt(9 * cs.Cin)
    t["w"] = phase_weights(w) if cs.phase else w.half()           # the fp16 weights that are sent, before the K order
    t["bias"] = torch.randn(cs.Cout, generator=g) * 0.5
    t["rowvec"] = rn((cs.B, cs.Cout), 0.5) if cs.rowvec else None
    t["resid"] = rn((cs.B, cs.Ho, cs.Wo, cs.Cout)) if cs.resid else None
    return t


def pack_k(wt, cb):
    """wt [Co, Ci, T] -> [Co, T * Ci] with column k = ((ci / cb) * T + tap) * cb + ci % cb (include/pbe_hip.h, pbe_conv3x3_desc.kblock)."""
    Co, Ci, T = wt.shape
    assert cb % 64 == 0 and Ci % cb == 0
    ci, tap = torch.meshgrid(torch.arange(Ci), torch.arange(T), indexing="ij")
    k = ((ci // cb) * T + tap) * cb + ci % cb
    out = torch.empty(Co, T * Ci, dtype=wt.dtype)
    out[:, k.reshape(-1)] = wt.reshape(Co, Ci * T)
    return out


def packed(cs: Case, cb):
    w = operands(cs)["w"]
    if cs.phase:
        return torch.stack([pack_k(w[p], cb) for p in range(4)], 0).contiguous()
    return pack_k(w.reshape(cs.Cout, cs.Cin, 9), cb).contiguous()


# ---- fp64 reference and the per-element bound ------------------------------------------------------------------------------------------
def _nchw64(cs: Case, t):
    x = t["x1"] if t["x2"] is None else torch.cat([t["x1"], t["x2"]], -1)
    return x.double().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def reference(cs: Case):
    """(want, bound) [M, Cout] fp64 over every output element: F.conv2d in fp64 on the fp16 operands that are sent."""
    t = operands(cs)
    x = _nchw64(cs, t)
    if cs.phase:
        xp = F.pad(x, (1, 1, 1, 1))
        acc = torch.empty(cs.B, cs.Cout, 2 * cs.H, 2 * cs.W, dtype=torch.float64)
        S = torch.empty_like(acc)
        for py in (0, 1):
            for px in (0, 1):
                w = t["w"][2 * py + px].double().reshape(cs.Cout, cs.Cin, 2, 2)
                acc[:, :, py::2, px::2] = F.conv2d(xp, w)[:, :, py:py + cs.H, px:px + cs.W]
                S[:, :, py::2, px::2] = F.conv2d(xp.abs(), w.abs())[:, :, py:py + cs.H, px:px + cs.W]
    else:
        if cs.ups:
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        if not cs.pad:
            x = F.pad(x, (0, 1, 0, 1))
        w = t["w"].double()
        acc = F.conv2d(x, w, stride=cs.stride, padding=1 if cs.pad else 0)
        S = F.conv2d(x.abs(), w.abs(), stride=cs.stride, padding=1 if cs.pad else 0)
    assert acc.shape == (cs.B, cs.Cout, cs.Ho, cs.Wo)
    flat = lambda v: v.permute(0, 2, 3, 1).reshape(cs.M, cs.Cout)
    kw = dict(bias=t["bias"].double())
    if cs.rowvec:
        kw["rowvec"] = t["rowvec"].double().repeat_interleave(cs.Ho * cs.Wo, 0)
    if cs.resid:
        kw["resid"] = t["resid"].double().reshape(cs.M, cs.Cout)
    want, bound = tc.expect(flat(acc), flat(S), cs.K, **kw)
    return want, tc.clamp_to_close(want, bound, tc.CLOSE["conv"])


def compare(cs: Case, got, what):
    """tilecheck.Report of got [M, Cout] (or [B, Ho, Wo, Cout]) against the reference; ratio > 1 = rejected."""
    want, bound = reference(cs)
    rep = tc.compare(got.reshape(cs.M, cs.Cout).cpu(), want, bound, what)
    row = int(rep.where.split(",")[0].split()[1])
    rep.where = f"pixel {cs.label(row)}, channel {rep.where.split()[-1]}"
    return rep


def gate(cs: Case, got, what):
    rep = compare(cs, got, what)
    assert rep.ratio <= 1.0, str(rep)
    return rep


# ---- the kernel restated in fp32 on the host ---------------------------------------------------------------------------------------------
MUTANTS = ["wrong_cb", "replicate", "no_shift", "src_stride", "resume_tap0", "drop_kt"]


def applies(mutant, cs: Case, cb, split_per):
    """Does the mutant change anything the kernel does on this case?"""
    if mutant == "wrong_cb":        # weights packed at 64, consumed at 128
        return cb == 64 and cs.C1 % 128 == 0 and cs.C2 % 128 == 0
    if mutant == "replicate":       # the zero row above the image (pad 1) / below it (pad 0) replicated from the border row
        below = (cs.Ho - 1) * cs.stride + 2 >= (cs.H << (cs.ups == 1))
        return cs.pad == 1 or below
    if mutant == "no_shift":
        return cs.ups == 1
    if mutant == "src_stride":
        return cs.C2 > 0 and cs.C1 != cs.C2
    if mutant == "resume_tap0":
        return split_per is not None and any(s[2] for s in slices(cs, cb, split_per))
    if mutant == "drop_kt":
        return cb == 192
    raise KeyError(mutant)


def slices(cs: Case, cb, split_per):
    """[(kt0, channel block, tap, kj, c0)] where each split-K slice resumes (igemm_kernel: cblk = kt0 / per_blk, tap = r / KB, kj = r % KB)."""
    KB, out = cb // 64, []
    per_blk = cs.T * KB
    for kt0 in range(0, cs.nk, split_per):
        cblk, r = divmod(kt0, per_blk)
        tap, kj = divmod(r, KB)
        out.append((kt0, cblk, tap, kj, cblk * cb + kj * 64))
    return out


def tap_table(cs: Case, py=0, px=0, mutant=None):
    """[T, rows] source pixel (b H + y) W + x of every tile row's taps, -1 = the zero block; rows = output pixels (phase: source pixels)."""
    H, W = cs.H, cs.W
    hw, wo = (H * W, W) if cs.phase else (cs.Ho * cs.Wo, cs.Wo)
    m = torch.arange(cs.B * hw)
    b, rem = m // hw, m % hw
    oy, ox = rem // wo, rem % wo
    tab = []
    for tp in range(cs.T):
        if cs.phase:
            iy, ix, hv, wv, sh = oy - 1 + py + (tp >> 1), ox - 1 + px + (tp & 1), H, W, 0
        else:
            sh = cs.ups
            iy, ix, hv, wv = oy * cs.stride - cs.pad + tp // 3, ox * cs.stride - cs.pad + tp % 3, H << sh, W << sh
        if mutant == "replicate":
            iy = torch.where(iy == -1, 0, iy) if cs.pad else torch.where(iy == hv, hv - 1, iy)
        ok = (iy >= 0) & (iy < hv) & (ix >= 0) & (ix < wv)
        sy, sx = (iy.clamp(0, H - 1), ix.clamp(0, W - 1)) if mutant == "no_shift" else (iy >> sh, ix >> sh)
        tab.append(torch.where(ok, (b * H + sy) * W + sx, -1))
    return torch.stack(tab, 0)


def emulate(cs: Case, cb, split_per=None, mutant=None):
    """The stored fp16 output [B, Ho, Wo, Cout] as the kernel computes it: fp16 operands, one fp32 accumulation per 64-wide k-tile in the
    kernel's (block, tap, channel) order, split-K slabs summed in slice order, fp32 epilogue (bias + row vector, fp16 store, residual,
    fp16 store).  Never a kernel's output."""
    t = operands(cs)
    wp = packed(cs, 64 if mutant == "wrong_cb" else cb)
    if mutant == "wrong_cb":
        cb = 128
    KB, T, C1, C2 = cb // 64, cs.T, cs.C1, cs.C2
    per_blk = T * KB
    x1 = t["x1"].reshape(-1).float()
    x2 = t["x2"].reshape(-1).float() if C2 else None
    lane = torch.arange(64)
    outs = []
    for ph in range(4 if cs.phase else 1):
        tab = tap_table(cs, ph >> 1, ph & 1, mutant)
        w = (wp[ph] if cs.phase else wp).float()
        total = None
        for kt0 in range(0, cs.nk, split_per or cs.nk):
            cblk, r = divmod(kt0, per_blk)
            tap, kj = divmod(r, KB)
            c0 = cblk * cb + kj * 64
            if mutant == "resume_tap0":
                tap = 0
            acc = torch.zeros(tab.shape[1], cs.Cout)
            for kt in range(kt0, min(cs.nk, kt0 + (split_per or cs.nk))):
                first = c0 < C1
                src, ch, stride = (x1, c0, C1) if first else (x2, c0 - C1, C1 if mutant == "src_stride" else C2)
                pix = tab[tap]
                idx = (pix.clamp(min=0)[:, None] * stride + ch + lane[None, :]) % src.numel()
                a = torch.where((pix >= 0)[:, None], src[idx], torch.zeros(()))
                if not (mutant == "drop_kt" and KB == 3 and kj == KB - 1):
                    acc += a @ w[:, kt * 64:(kt + 1) * 64].t()
                c0 += 64
                kj += 1
                if kj == KB:
                    kj, tap = 0, tap + 1
                    if tap == T:
                        tap = 0
                    else:
                        c0 -= cb
            total = acc if total is None else total + acc
        outs.append(total)
    if cs.phase:
        full = torch.empty(cs.B, 2 * cs.H, 2 * cs.W, cs.Cout)
        for ph in range(4):
            full[:, (ph >> 1)::2, (ph & 1)::2] = outs[ph].view(cs.B, cs.H, cs.W, cs.Cout)
        v = full
    else:
        v = outs[0].view(cs.B, cs.Ho, cs.Wo, cs.Cout)
    v = v + t["bias"]
    if cs.rowvec:
        v = v + t["rowvec"].float()[:, None, None, :]
    y = v.half()
    if cs.resid:
        y = (y.float() + t["resid"].float()).half()
    return y


# ---- the host planner --------------------------------------------------------------------------------------------------------------------
def descriptor(cs: Case, kblock, tile_cfg=-1, ptr=None):
    """pbe_conv3x3_desc of the case; ptr: name -> address (default: aligned fake addresses, for the plan queries)."""
    from pbe_amd import lib, ops
    p = (lambda n: FAKE) if ptr is None else ptr
    d = lib.Conv3x3Desc()
    d.X, d.Wp, d.Y, d.bias = p("x1"), p("wp"), p("y"), p("bias")
    d.X2 = p("x2") if cs.C2 else None
    d.rowvec, d.ldv = (p("rowvec"), cs.Cout + 8) if cs.rowvec else (None, 0)
    d.resid = p("resid") if cs.resid else None
    d.B, d.H, d.W, d.C1, d.C2, d.Cout = cs.B, cs.H, cs.W, cs.C1, cs.C2, cs.Cout
    d.stride, d.pad, d.upsample, d.act, d.kblock = cs.stride, cs.pad, cs.ups, 0, kblock
    d.workspace, d.workspace_bytes, d.tile_cfg = p("ws"), ops.SPLITK_WS_BYTES, tile_cfg
    if cs.groups:
        d._blocks = C.c_int32(-1)
        d.group_stats_out, d.group_stats_groups = p("gstats"), cs.groups
        d.group_stats_blocks = C.cast(C.pointer(d._blocks), C.c_void_p)
    return d


def prologue(cs: Case, kblock, tile_cfg=-1):
    """pbe_conv3x3_prologue of a request as a dict (NAMES), or the error code where the entry point refuses."""
    from pbe_amd import lib
    out = (C.c_int32 * 32)()
    rc = lib.load().pbe_conv3x3_prologue(C.byref(descriptor(cs, kblock, tile_cfg)), out)
    return rc if rc else {n: int(v) for n, v in zip(NAMES, out)}


def honoured(cs: Case, kblock, tile):
    """The split-K requests 2 <= s <= nk / 4 that the planner runs as asked on this tile."""
    out = []
    for s in range(2, cs.nk // 4 + 1):
        pro = prologue(cs, kblock, tile | (s << 8))
        if (pro["tile"], pro["splits"]) == (tile, s):
            out.append((s, pro))
    return out


def kj_split(cs: Case, kblock, tile):
    """(s, prologue) of the largest honoured request with a slice that resumes at kj != 0 (inside a (block, tap) visit)."""
    for s, pro in reversed(honoured(cs, kblock, tile)):
        assert pro["per_blk"] == cs.T * kblock // 64
        if any(sl[3] for sl in slices(cs, kblock, pro["split_per"])):
            return s, pro
    raise AssertionError(f"{cs.id} kblock {kblock} tile {tile}: no honoured split-K request resumes inside a (block, tap) visit")


def lattice():
    """Every (case, kblock, split_per or None) of the GPU lattice, for the restatement: needs the built library's host planner."""
    out = [(case(g), 64, None) for g in GEOS]
    wide = case("cat", 128, 128)
    out += [(wide, 64, sp) for sp in sorted({pro["split_per"] for tl in SPLIT_TILES for _, pro in honoured(wide, 64, tl)})]
    out.append((case("phase"), 128, None))
    out.append((case("gs"), 64, None))
    halo = case("halo11")
    out += [(halo, kb, prologue(halo, 128, 11 | (1 << 8))["split_per"]) for kb in (64, 128)]
    for geo in KB_GEOS:
        for c1, c2, kb in KB_CHANNELS:
            cs = case(geo, c1, c2)
            out.append((cs, kb, None))
            out += [(cs, kb, sp) for sp in sorted({kj_split(cs, kb, tl)[1]["split_per"] for tl in KB_TILES})]
    return out


# ---- launches (GPU) -----------------------------------------------------------------------------------------------------------------------
def report(line):
    """Append a line to convlattice_report.txt beside the parity report (committed copy: profiles/convlattice_report.txt)."""
    import test_model_gpu as parity
    path = os.path.join(os.path.dirname(parity.REPORT), "convlattice_report.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def launch(cs: Case, dev, *, tile, splits=1, kblock=64, wp=None, arena=False, want=None):
    """One pbe_conv3x3_f16 launch under ops.tune(1, tile | splits << 8) -> dict(y [B, Ho, Wo, Cout] on the host, plan (tile, split-K),
    blocks, gstats).  wp: the packed weights (default: packed(cs, kblock)).  arena: X / X2 / resid out of NaN arenas, Y and the group
    statistics in sentinel arenas - nothing outside them may be written, every element of Y must be.  want: the (tile, split-K) that
    must run (default: the request)."""
    import guard
    from pbe_amd import ops
    t = operands(cs)
    keep = {}                                                      # device tensors of this launch, by descriptor field

    def up(name, v):
        if v is not None:
            keep[name] = guard.embed(v.reshape(-1), device=dev)[0] if arena and name in ("x1", "x2", "resid") else v.contiguous().to(dev)

    for name in ("x1", "x2", "bias", "resid"):
        up(name, t[name])
    up("wp", packed(cs, kblock) if wp is None else wp)
    if cs.rowvec:                                                  # ldv = Cout + 8: NaN in the leading-dimension padding
        rv = torch.full((cs.B, cs.Cout + 8), float("nan"), dtype=torch.float16)
        rv[:, :cs.Cout] = t["rowvec"]
        keep["rowvec"] = rv.to(dev)
    n = cs.M * cs.Cout
    if arena:
        keep["y"], y_arena = guard.sentinel_out((n,), device=dev)
    else:
        keep["y"] = torch.empty(n, dtype=torch.float16, device=dev)
    ng = cs.B * max(1, (cs.Ho * cs.Wo) // 64) * cs.groups * 2
    if cs.groups:
        keep["gstats"], g_arena = guard.sentinel_out((ng,), dtype=torch.float32, device=dev)
    keep["ws"] = ops._splitk_ws(dev)
    d = descriptor(cs, kblock, -1, lambda name: keep[name].data_ptr())
    try:
        ops.tune(1, tile | (splits << 8))
        ops._PLANS = []
        ops._launch("conv", d)
        plans = ops._PLANS
    finally:
        ops.tune(1, -1)
        ops._PLANS = None
    torch.cuda.synchronize(dev)
    assert len(plans) == 1, plans
    plan = (plans[0][1], max(1, plans[0][2]))
    what = f"{cs.id} kblock {kblock} tile {tile} split {splits}"
    assert plan == ((tile, splits) if want is None else want), f"{what}: the launch ran tile {plan[0]} split-K {plan[1]}"
    res = {"y": keep["y"].view(cs.B, cs.Ho, cs.Wo, cs.Cout).cpu(), "plan": plan, "blocks": 0}
    if cs.groups:
        res["blocks"] = blocks = d._blocks.value
        used = cs.B * blocks * cs.groups * 2
        assert 0 <= blocks and used <= ng, (what, blocks)
        guard.assert_untouched(g_arena, keep["gstats"][:used], what + " [group statistics]")
        if blocks:
            guard.assert_fully_written(keep["gstats"][:used], what + " [group statistics]")
            res["gstats"] = keep["gstats"][:used].view(cs.B, blocks, cs.groups, 2).double().cpu()
    if arena:
        guard.assert_untouched(y_arena, keep["y"], what + " [Y]")
        guard.assert_fully_written(keep["y"], what + " [Y]")
    return res


def check_group_stats(cs: Case, res, what):
    """The partials the copy-out emitted against fp64 sums of the STORED output, at the limits of test_tuned_entry_against_fp64."""
    if not res["blocks"]:
        return 0
    G = cs.groups
    tot = res["gstats"].sum(1)
    yg = res["y"].double().view(cs.B, cs.Ho * cs.Wo, G, cs.Cout // G)
    ref = torch.stack([yg.sum((1, 3)), (yg ** 2).sum((1, 3))], -1)
    assert torch.allclose(tot, ref, rtol=2e-6, atol=1e-3), f"{what}: group statistics off by {(tot - ref).abs().max().item():.3e}"
    return res["blocks"]


def refused(cs: Case, dev, kblock):
    """pbe_conv3x3_f16's return code for the case at this kblock with Y inside a sentinel arena, after asserting not one byte of it changed."""
    import guard
    from pbe_amd import lib, ops
    t = operands(cs)
    keep = {n: t[n].contiguous().to(dev) for n in ("x1", "x2", "bias", "resid", "rowvec") if t[n] is not None}
    keep["wp"] = packed(cs, 64).to(dev)
    keep["y"], arena = guard.sentinel_out((cs.M * cs.Cout,), device=dev)
    keep["ws"] = ops._splitk_ws(dev)
    if cs.groups:
        keep["gstats"] = torch.zeros(cs.B * max(1, (cs.Ho * cs.Wo) // 64) * cs.groups * 2, device=dev)
    d = descriptor(cs, kblock, -1, lambda name: keep[name].data_ptr())
    if cs.rowvec:
        d.ldv = cs.Cout
    rc = lib.load().pbe_conv3x3_f16(C.byref(d), ops._stream())
    torch.cuda.synchronize(dev)
    guard.assert_untouched(arena, keep["y"][:0], f"{cs.id} kblock {kblock} [refused]")
    return rc
