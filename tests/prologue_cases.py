"""Launches whose bits must not move when igemm_kernel's prologue changes: helpers shared by tests/test_prologue_gpu.py and
tools/record_prologue_golden.py (which wrote tests/golden/prologue_parent.npz with the build BEFORE the prologue work).  Plain functions.

Every case forces its tile through tile_cfg (pbe_tune key 1) and asserts the launch ran it.  Operands come from a CPU generator seeded by
the case id, so they are the same on every machine.  Of each output the golden file keeps the SHA-256 of all its bytes (equality of the whole
tensor) and every stride-th element as raw values (which elements moved, when one did); fp16 outputs as fp16.

Halo cases: a tile is listed at a map only where the library's halo rule admits it (whole rows of one image or whole images per tile, halo
rows within the tile's halo image) - tests/test_halo_plan_cpu.py restates that rule; here the plan query decides and the case asserts it.
"""
from __future__ import annotations

import hashlib
import math
import zlib

import numpy as np
import torch

KEEP = 4096                     # elements of an output kept raw in the golden file
HALO_TILES = {10: (256, 392), 11: (128, 264), 12: (128, 264), 13: (256, 392), 14: (128, 392)}        # tile -> (BM, halo image rows)
# (B, H, W, C1, C2, Cout)
HALO_MAPS = [(2, 8, 8, 128, 0, 128), (1, 16, 16, 64, 0, 160), (1, 32, 32, 64, 64, 160), (1, 64, 64, 64, 0, 160)]
DENSE_TILES = [3, 6, 9, 17, 21]
EX_TILES = [3, 6, 9, 17]
GM, GN, GK = 200, 168, 200      # ragged in all three, K % 64 != 0
GK_SPLIT = 520                  # split-K 2 needs >= 4 k-tiles of 64 per slice (clamp_splits): K = 200 has 4 in all.  520 = 8 k-tiles + 8
GK1 = 96                        # second source from k = 96: inside k-tile 1 (a straddling k-tile).  K1 must be a multiple of 32 (pbe_gemm_f16)


def halo_fits(tile, B, H, W):
    """The halo rule of the planner (igemm_plan.h, halo_rows) for tile on a [B, H, W] map."""
    bm, hpa = HALO_TILES[tile]
    if W < 8 or W > 128 or W & (W - 1) or bm % W or (B * H * W) % bm:
        return False
    th = min(bm // W, H)
    if H % th or bm % (th * W):
        return False
    nsub = bm // (th * W)
    return not (nsub > 1 and th != H) and nsub * ((th + 2) * (W + 1) + 1) <= hpa


def specs():
    out = []
    for shape in HALO_MAPS:
        for tile in HALO_TILES:
            if halo_fits(tile, *shape[:3]):
                out.append(dict(id=f"halo-t{tile}-" + "x".join(map(str, shape)), kind="conv", shape=shape, tile=tile))
    # four whole 8x8 images per 256-pixel tile (the form the 8x8 level of the U-Net runs), both 256-pixel tiles
    for tile in (10, 13):
        out.append(dict(id=f"halo-t{tile}-4img-4x8x8x128x0x128", kind="conv", shape=(4, 8, 8, 128, 0, 128), tile=tile))
    # the plain (not ping-pong) main loop of a 256-pixel tile
    out.append(dict(id="halo-t10-plainloop-1x32x32x64x64x160", kind="conv", shape=HALO_MAPS[2], tile=10, pingpong=0))
    # split-K 3 over 5 channel blocks: slices of 2, 2, 1 blocks
    out.append(dict(id="halo-t11-split3-1x16x16x320x0x160", kind="conv", shape=(1, 16, 16, 320, 0, 160), tile=11, splits=3))
    # row vector, several samples per tile: 2 (tile 11) and 4 (tile 10: more than the staged vectors hold, the per-row form)
    for tile in (11, 10):
        out.append(dict(id=f"halo-t{tile}-rowvec-4x8x8x128x0x128", kind="conv", shape=(4, 8, 8, 128, 0, 128), tile=tile, rowvec=True))
    out.append(dict(id="gather-t9-phase-up-1x16x16x64x160", kind="up", shape=(1, 16, 16, 64, 0, 160), tile=9))
    for tile in DENSE_TILES:
        for v in ("plain", "a2", "batch", "splitk"):
            out.append(dict(id=f"dense-t{tile}-{v}", kind="gemm", tile=tile, variant=v, splits=2 if v == "splitk" else 1))
    for tile in EX_TILES:
        out.append(dict(id=f"ex-t{tile}-ln-stats", kind="gemm", tile=tile, variant="lnstats"))
    for tile in (19, 20):       # A-stationary tiles: only the K = 320 GEGLU projection with the LayerNorm fold (pbe_astat_ok)
        out.append(dict(id=f"astat-t{tile}-geglu", kind="gemm", tile=tile, variant="astat"))
    return out


def _gen(spec):
    return torch.Generator().manual_seed(zlib.crc32(spec["id"].split("-t")[0].encode() + repr(spec.get("shape", spec.get("variant"))).encode()) & 0x7FFFFFFF)


def _h(g, dev, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half().to(dev)


def _forced(request, fn, pingpong=1):
    """fn() with tile_cfg `request` forced -> (result, the one recorded plan (key, tile, split-K, BM, BN, workgroups))."""
    from pbe_amd import ops
    try:
        ops.tune(1, request)
        ops.tune(4, pingpong)
        ops._PLANS = []
        r = fn()
        plans = ops._PLANS
    finally:
        ops.tune(1, -1)
        ops.tune(4, 1)
        ops._PLANS = None
    assert len(plans) == 1, plans
    return r, plans[0]


def run(spec, dev, tile=None):
    """Launch the case on tile `tile` (default: the case's own) -> list of output tensors; asserts the forced (tile, split-K) ran.
    Operands depend on the case's shape / variant only, never on the tile."""
    from pbe_amd import ops
    g = _gen(spec)
    want_tile = spec["tile"] if tile is None else tile
    splits = spec.get("splits", 1)
    request = want_tile | (splits << 8)
    if spec["kind"] in ("conv", "up"):
        B, H, W, C1, C2, Co = spec["shape"]
        x = _h(g, dev, B, H, W, C1)
        x2 = _h(g, dev, B, H, W, C2) if C2 else None
        w = torch.randn(Co, C1 + C2, 3, 3, generator=g) / math.sqrt(9 * (C1 + C2))
        bias = (torch.randn(Co, generator=g) * 0.5).to(dev)
        if spec["kind"] == "up":
            wp = ops.pack_conv3x3_up_phases(w.to(dev))
            fn = lambda: ops.conv3x3(x, wp, bias, upsample=True)
        else:
            wp = ops.pack_conv3x3(w.to(dev), split=(C1, C2) if C2 else None)
            kw = {}
            if spec.get("rowvec"):
                kw["rowvec"] = _h(g, dev, B, Co, scale=0.5)
            fn = lambda: ops.conv3x3(x, wp, bias, x2=x2, **kw)
        y, plan = _forced(request, fn, spec.get("pingpong", 1))
        outs = [y]
    else:
        v = spec["variant"]
        if v == "astat":
            M, N, K = 256, 640, 320
        else:
            M, N, K = GM, GN, GK_SPLIT if v == "splitk" else GK
        w = _h(g, dev, N, K, scale=1.0 / math.sqrt(K))
        bias = (torch.randn(N, generator=g) * 0.5).to(dev)
        if v in ("plain", "splitk"):
            a = _h(g, dev, M, K)
            fn = lambda: [ops.gemm(a, w, bias)]
        elif v == "a2":
            a, a2 = _h(g, dev, M, GK1), _h(g, dev, M, K - GK1)
            fn = lambda: [ops.gemm(a, w, bias, a2=a2)]
        elif v == "batch":
            a = _h(g, dev, 2, M + 8, K)[:, :M]                      # batch stride (M + 8) K: not the dense M K
            wb = torch.stack([w, _h(g, dev, N, K, scale=1.0 / math.sqrt(K))])
            fn = lambda: [ops.gemm(a, wb, bias)]
        else:
            a = _h(g, dev, M, K, scale=1.3)
            a[::7] += 6.0                                           # mean >> std rows: the cancellation case of the fold
            gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(dev)
            beta = (0.1 * torch.randn(K, generator=g)).to(dev)
            wg, c2, c1 = ops.pack_linear_ln(w.float(), bias, gamma, beta)
            st = ops.row_stats(a)
            if v == "astat":
                fn = lambda: [ops.gemm(a, wg, c2, ln=(st, c1, 1e-5), act=ops.ACT_GEGLU)]
            else:
                def fn():
                    y, s = ops.gemm(a, wg, c2, ln=(st, c1, 1e-5), row_stats=True)
                    return [y, s.buf[: s.parts]]
        outs, plan = _forced(request, fn)
    assert (plan[1], max(1, plan[2])) == (want_tile, splits), f"{spec['id']}: asked for tile {want_tile} split-K {splits}, the launch ran {plan}"
    torch.cuda.synchronize()
    return outs


def digest(t):
    """(sha256 of the tensor's bytes as 32 uint8, every stride-th element) of a device tensor."""
    a = t.detach().contiguous().cpu().numpy()
    flat = a.reshape(-1)
    stride = max(1, flat.size // KEEP)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy(), flat[::stride].copy()
