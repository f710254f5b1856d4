"""The launch-invariant values the host hands igemm_kernel for its prologue (pbe_conv3x3_prologue: nothing is launched), against the
kernel's halo geometry restated here with Python's own integer division.

The kernel (pbe_amd/csrc/igemm_kernel.h, MODE 2) stages, per (sub-)image of a tile, a halo of (TH + 2) rows of W + 1 pixels + 1: halo row
hp = sub * HPS + hy * HW2 + hx holds pixel (y0 + hy - 1, hx - 1) of image b0 + sub, or zeros outside the image; tile row ml = sub * TH * W +
ty * W + tx reads halo row sub * HPS + (ty + 1) * HW2 + tx + 1 for the centre tap.  Since the prologue work the kernel no longer divides:
   udiv_h(a, mh)     = (a * mh) >> 20,                 mh = ceil(2^20 / d)         halo rows: a < 2 HPA
   udiv_mg(n, d, mg) = q + (n - q d >= d), q = (n * mg) >> 32, mg = floor(2^32 / d)   tile ids, samples, k-tiles: any 32-bit n
   shifts by log2 W and log2 (TH W)                                                tile rows: ml < BM
"""
import ctypes as C

import numpy as np
import pytest

from prologue_cases import HALO_TILES, halo_fits

FAKE = 1 << 20
# (B, H, W): 8x8 with 4 images per 256-pixel tile (2 per 128-pixel tile), 16x16, 24x16, 32x32, 64x64, 128-wide
MAPS = [(4, 8, 8), (2, 16, 16), (2, 24, 16), (2, 32, 32), (2, 64, 64), (1, 16, 128)]
NAMES = ["tile", "splits", "bm", "bn", "mode", "m_fast", "tdiv", "mg_tdiv", "split_per", "sv_ns", "sv_gdiv", "mg_sv_gdiv", "hw", "mg_hw", "mg_wo",
         "per_blk", "mg_per_blk", "mg_kb", "th", "hw2", "hps", "nsub", "rows", "tpi", "mg_tpi", "mh_hps", "mh_hw2", "lgw", "lgimg", "hpa",
         "off_tail", "off_last"]


def mg_of(d):
    return 0xFFFFFFFF if d == 1 else (1 << 32) // d


def udiv_h(a, mh):
    return (a * mh) >> 20


def udiv_mg(n, d, mg):
    n = np.asarray(n, dtype=np.uint64)
    q = (n * np.uint64(mg)) >> np.uint64(32)
    return q + ((n - q * np.uint64(d)) >= np.uint64(d)).astype(np.uint64)


def prologue(B, H, W, C1, C2, Co, tile_cfg, rowvec=False):
    from pbe_amd import lib, ops
    d = lib.Conv3x3Desc()
    d.X, d.Wp, d.Y, d.bias = FAKE, FAKE, FAKE, FAKE
    d.X2 = FAKE if C2 else None
    d.rowvec, d.ldv = (FAKE, Co) if rowvec else (None, 0)
    d.B, d.H, d.W, d.C1, d.C2, d.Cout = B, H, W, C1, C2, Co
    d.stride, d.pad, d.upsample, d.act, d.kblock = 1, 1, 0, 0, 64
    d.workspace, d.workspace_bytes, d.tile_cfg = FAKE, ops.SPLITK_WS_BYTES, tile_cfg
    out = (C.c_int32 * 32)()
    h = lib.load()
    assert h.pbe_conv3x3_prologue(C.byref(d), out) == 0, h.pbe_last_error()
    return {n: (int(v) & 0xFFFFFFFF if n.startswith(("mg_", "mh_")) else int(v)) for n, v in zip(NAMES, out)}


CASES = [(t, m) for m in MAPS for t in HALO_TILES if halo_fits(t, *m)]


def test_every_map_has_a_halo_tile():
    assert {m for _, m in CASES} == set(MAPS) and {t for t, _ in CASES} == set(HALO_TILES)


@pytest.mark.parametrize("tile,shape", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"t{v}")
def test_halo_constants_and_pixels(tile, shape):
    """Constants of the launch, then for the top, the bottom and an interior tile of the map every halo row's source pixel and every tile
    row's halo row, computed the kernel's way, against divmod."""
    B, H, W = shape
    bm, hpa = HALO_TILES[tile]
    c = prologue(B, H, W, 64, 0, 160, tile | (1 << 8))
    assert (c["tile"], c["splits"], c["mode"], c["bm"], c["hpa"]) == (tile, 1, 2, bm, hpa)
    th = min(bm // W, H)
    hw2, hps, img = W + 1, (th + 2) * (W + 1) + 1, th * W
    nsub, tpi = bm // img, H // th
    assert (c["th"], c["hw2"], c["hps"], c["nsub"], c["rows"], c["tpi"]) == (th, hw2, hps, nsub, nsub * hps, tpi)
    assert (1 << c["lgw"], 1 << c["lgimg"]) == (W, img) and nsub * hps <= hpa
    tiles_m = B * H * W // bm
    assert c["tdiv"] == (tiles_m if c["m_fast"] else -(-160 // c["bn"])) and c["split_per"] == 1      # (64 channels: one block, never split)
    # every magic divisor over its whole domain: halo rows below 2 HPA, tile rows below BM, tile ids below 65 536
    a = np.arange(2 * hpa, dtype=np.int64)
    assert np.array_equal(udiv_h(a, c["mh_hps"]), a // hps) and np.array_equal(udiv_h(a, c["mh_hw2"]), a // hw2)
    assert (a * max(c["mh_hps"], c["mh_hw2"])).max() < 1 << 32 and max(c["mh_hps"], c["mh_hw2"]) < 1 << 24      # the kernel's 24-bit multiply
    ml = np.arange(bm, dtype=np.int64)
    assert np.array_equal(ml >> c["lgimg"], ml // img) and np.array_equal((ml & (img - 1)) >> c["lgw"], (ml % img) // W)
    ids = np.arange(65536, dtype=np.uint64)
    for d, mg in ((c["tdiv"], c["mg_tdiv"]), (tpi, c["mg_tpi"])):
        assert mg == mg_of(d) and np.array_equal(udiv_mg(ids, d, mg), ids // np.uint64(d)), (d, mg)
    assert (c["mh_hps"], c["mh_hw2"]) == (-(-(1 << 20) // hps), -(-(1 << 20) // hw2))
    # top, bottom and interior tiles: the kernel's (b0, y0), its halo pixels and centre rows
    for tm in sorted({0, tiles_m - 1, tiles_m // 2, min(1, tiles_m - 1)}):
        if nsub > 1:
            b0, y0 = tm * nsub, 0
        else:
            b0 = int(udiv_mg(tm, tpi, c["mg_tpi"]))
            y0 = (tm - b0 * tpi) * th
        assert (b0, y0) == ((tm * bm) // (H * W), ((tm * bm) % (H * W)) // W)
        seen = {}
        for hp in range(hpa):
            pix = -1
            if hp < c["rows"]:
                sub = udiv_h(hp, c["mh_hps"]); r = hp - sub * hps
                hy = udiv_h(r, c["mh_hw2"]); hx = r - hy * hw2
                y, x = y0 + hy - 1, hx - 1
                if 0 <= y < H and 0 <= x < W:
                    pix = ((b0 + sub) * H + y) * W + x
            # the same by divmod
            want = -1
            if hp < nsub * hps:
                sub2, r2 = divmod(hp, hps)
                hy2, hx2 = divmod(r2, hw2)
                if hy2 < th + 2 and 0 <= y0 + hy2 - 1 < H and 0 <= hx2 - 1 < W:
                    want = ((b0 + sub2) * H + y0 + hy2 - 1) * W + hx2 - 1
            assert pix == want, (tm, hp, pix, want)
            seen[hp] = pix
        for m in range(bm):             # centre tap of every tile row lands on its own pixel; the 8 neighbours on theirs or on zeros
            sub = m >> c["lgimg"]; rr = m - (sub << c["lgimg"]); ty = rr >> c["lgw"]; tx = rr - (ty << c["lgw"])
            hc = sub * hps + (ty + 1) * hw2 + tx + 1
            assert seen[hc] == tm * bm + m, (tm, m)
            b, yy, xx = (tm * bm + m) // (H * W), ((tm * bm + m) % (H * W)) // W, m % W
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    inside = 0 <= yy + dy < H and 0 <= xx + dx < W
                    assert seen[hc + dy * hw2 + dx] == ((b * H + yy + dy) * W + xx + dx if inside else -1), (tm, m, dy, dx)


def test_split_k_slices_and_samples_per_tile():
    """Split-K 3 over 5 channel blocks: slices of 2 blocks (2, 2, 1); a row vector over 8x8 samples: 2 per 128-pixel tile, 4 per 256-pixel
    tile; 64x64 samples: 16 / 32 row tiles per sample."""
    c = prologue(1, 16, 16, 320, 0, 160, 11 | (3 << 8))
    assert (c["tile"], c["splits"], c["split_per"]) == (11, 3, 2)
    c = prologue(1, 16, 16, 320, 0, 160, 9 | (3 << 8))              # the gather tile slices k-tiles: 45 in 3 slices
    assert (c["tile"], c["mode"], c["splits"], c["split_per"], c["per_blk"], c["hw"]) == (9, 1, 3, 15, 9, 256)
    assert (prologue(4, 8, 8, 128, 0, 128, 11 | (1 << 8), rowvec=True)["sv_ns"], prologue(4, 8, 8, 128, 0, 128, 10 | (1 << 8), rowvec=True)["sv_ns"]) == (2, 4)
    c = prologue(2, 64, 64, 64, 0, 160, 10 | (1 << 8), rowvec=True)
    assert (c["sv_ns"], c["sv_gdiv"]) == (1, 16) and int(udiv_mg(37, 16, c["mg_sv_gdiv"])) == 2


# (B, H, W, C1, C2, tile | split-K << 8, row vector, upsample): gather launches (MODE 1: tap table and split-K resume) and halo launches
HOST_CASES = [(2, 24, 16, 64, 0, 9 | (1 << 8), False, 0), (1, 16, 16, 320, 0, 9 | (3 << 8), False, 0), (2, 32, 32, 128, 128, 3 | (1 << 8), False, 0),
              (1, 16, 16, 64, 0, 9 | (1 << 8), False, 2), (8, 64, 64, 64, 0, 10 | (1 << 8), True, 0), (8, 64, 64, 64, 0, 11 | (1 << 8), True, 0),
              (4, 8, 8, 128, 0, 10 | (1 << 8), True, 0), (2, 24, 16, 64, 0, 11 | (1 << 8), True, 0)]


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda v: "-".join(map(str, v)))
def test_host_reciprocals_of_every_divisor(case):
    """Every reciprocal the host passes is floor(2^32 / its divisor) (2^32 - 1 for 1) - the value test_udiv_mg_is_exact proves exact - and
    divides exactly over its domain: output pixels m < M (tap table), k-tiles < K / 64 (split-K resume), row tiles (first sample of a tile)."""
    B, H, W, C1, C2, cfg, rowvec, ups = case
    from pbe_amd import lib, ops
    d = lib.Conv3x3Desc()
    d.X, d.Wp, d.Y, d.bias = FAKE, FAKE, FAKE, FAKE
    d.X2 = FAKE if C2 else None
    d.rowvec, d.ldv = (FAKE, 160) if rowvec else (None, 0)
    d.B, d.H, d.W, d.C1, d.C2, d.Cout = B, H, W, C1, C2, 160
    d.stride, d.pad, d.upsample, d.act, d.kblock = 1, 1, ups, 0, 64
    d.workspace, d.workspace_bytes, d.tile_cfg = FAKE, ops.SPLITK_WS_BYTES, cfg
    out = (C.c_int32 * 32)()
    assert lib.load().pbe_conv3x3_prologue(C.byref(d), out) == 0, lib.load().pbe_last_error()
    c = {n: (int(v) & 0xFFFFFFFF if n.startswith(("mg_", "mh_")) else int(v)) for n, v in zip(NAMES, out)}
    assert (c["tile"], c["splits"]) == (cfg & 255, cfg >> 8)
    taps, nk = (4, 4 * C1 // 64) if ups == 2 else (9, 9 * (C1 + C2) // 64)
    M = B * H * W
    assert (c["hw"], c["per_blk"]) == (H * W, taps) and c["sv_gdiv"] == max(1, H * W // c["bm"] if rowvec else c["sv_gdiv"])
    assert c["sv_ns"] == (max(1, c["bm"] // (H * W)) if rowvec else 1)
    tiles_m = M // c["bm"]
    for name, dv, dom in (("mg_hw", H * W, M + c["bm"]), ("mg_wo", W, H * W), ("mg_per_blk", taps, nk), ("mg_kb", 1, taps),
                          ("mg_sv_gdiv", c["sv_gdiv"], tiles_m), ("mg_tdiv", c["tdiv"], tiles_m * -(-160 // c["bn"]))):
        assert c[name] == mg_of(dv), (name, dv, c[name])
        n = np.arange(dom, dtype=np.uint64)
        assert np.array_equal(udiv_mg(n, dv, c[name]), n // np.uint64(dv)), name


@pytest.mark.parametrize("d", [1, 2, 3, 5, 7, 9, 16, 17, 36, 45, 255, 256, 257, 1000, 4095, 4096, 65535, 65536, 1 << 20, (1 << 31) - 1])
def test_udiv_mg_is_exact(d):
    """The fix-up form over tile ids below 65 536 and over the far end of the 32-bit range, for divisors of every size."""
    mg = 0xFFFFFFFF if d == 1 else (1 << 32) // d
    for n in (np.arange(65536, dtype=np.uint64), np.arange((1 << 32) - 65536, 1 << 32, dtype=np.uint64), np.arange(0, 1 << 32, 65521, dtype=np.uint64)):
        assert np.array_equal(udiv_mg(n, d, mg), n // np.uint64(d))


def test_parameter_block_head_and_tail():
    """Everything read before the first fetch sits in the first 224 bytes (three and a half 64-byte lines); the epilogue's fields follow: the
    tail starts where the head ends (the output pointer) and its last field (sv_ok; a diagnostic build appends its stamp pointer) ends the
    block.  The offsets the host fills are pinned in the library by static_asserts; here they are read back through its queries."""
    from pbe_amd import lib
    h = lib.load()
    head, size = h.pbe_sizeof_igemm_head(), h.pbe_sizeof_igemm_params()
    c = prologue(1, 16, 16, 64, 0, 160, 11 | (1 << 8))
    assert head == 224 and head % 8 == 0 and size % 8 == 0 and head < size <= 1024
    assert c["off_tail"] == head and head + 128 < c["off_last"] and c["off_last"] + 4 <= size <= c["off_last"] + 16
