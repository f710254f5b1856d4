"""The contract between the conv planner (halo_rows / plan_igemm, igemm_plan.h) and the halo-resident conv tiles 10 .. 14 (the MODE 2
prologue of igemm_kernel): whenever a plan names a halo tile, the tile's BM output rows are exactly the pixels of the image rows the
kernel stages for it.  Host-only plan queries with stand-in pointers (as tests/test_launch_cpu.py); nothing is launched.

The kernel's geometry, restated from the prologue (TW = W, TH = th):
    th            = min(BM / W, H)                   image rows per tile (launch_cfg)
    img_px        = th * W,  nsub = BM / img_px      (integer division; nsub > 1: the tile holds nsub whole images)
    tiles_per_img = H / th
    b0            = tm_i * nsub        if nsub > 1 else tm_i / tiles_per_img
    y0            = 0                  if nsub > 1 else (tm_i - b0 * tiles_per_img) * th
    staged        : rows y0 - 1 .. y0 + th of images b0 .. b0 + nsub - 1 (rows outside the image are zero)
    local pixel ml: sub = ml / img_px, ty = (ml % img_px) / W, tx = ml % W -> halo row of (image b0 + sub, row y0 + ty, column tx)
    copy-out      : local pixel ml is written to output row tm_i * BM + ml
These agree only where BM == nsub * th * W: a 12x8 map under a 128-pixel tile (img_px = 96, nsub = 1) writes pixels 128 .. 255 from
tile 1 while it stages image 1, and reads halo rows it never staged for ml >= 96."""
import functools
import itertools

import numpy as np
import pytest

import tilecheck as tc
from test_launch_cpu import _conv, _ops

HALO = range(10, 15)
BS = (1, 2, 3, 4, 8, 16)
HS = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)
WS = (8, 16, 32, 64, 128)
CHANNELS = ((64, 0, 64), (128, 0, 160), (256, 0, 256), (320, 0, 320), (640, 640, 640), (1280, 0, 1280))
MODES = [-1] + [t | (1 << 8) for t in HALO]          # the heuristic, and each halo tile requested at split factor 1


def geometry(H, W, BM):
    th = min(BM // W, H)
    img_px = th * W
    nsub = BM // img_px
    return th, img_px, nsub, H // th


@functools.lru_cache(maxsize=None)
def tile_faults(B, H, W, BM):
    """What is wrong with running a B x H x W map on a halo tile of BM pixels ('' = nothing): the closed conditions, then, tile by
    tile, the output rows the copy-out writes against the global pixel each local pixel's halo row holds."""
    th, img_px, nsub, tiles_per_img = geometry(H, W, BM)
    M = B * H * W
    why = []
    if nsub * th * W != BM:
        why.append(f"nsub * th * W = {nsub * th * W} != BM = {BM}")
    if M % BM:
        why.append(f"M = {M} is no multiple of BM = {BM}")
    if nsub > 1 and th != H:
        why.append(f"nsub = {nsub} > 1 but th = {th} != H = {H}")
    tm = np.arange(-(-M // BM))[:, None]
    ml = np.arange(BM)[None, :]
    b0 = tm * nsub if nsub > 1 else tm // tiles_per_img
    y0 = np.zeros_like(tm) if nsub > 1 else (tm - b0 * tiles_per_img) * th
    sub, rr = ml // img_px, ml % img_px
    b, y, x = b0 + sub, y0 + rr // W, rr % W
    held = (sub < nsub) & (rr // W < th) & (y < H) & (b < B)                 # a staged interior row of an image that exists
    source = np.where(held, (b * H + y) * W + x, -1)                         # global pixel whose 3x3 window local pixel ml reads
    written = tm * BM + ml                                                   # output row local pixel ml is stored to
    for i in range(source.shape[0]):
        rows = set(written[i][written[i] < M].tolist())
        pixels = set(source[i][source[i] >= 0].tolist())
        if rows != pixels or (source[i] != written[i])[written[i] < M].any():
            why.append(f"tile {i} writes rows {written[i, 0]} .. {min(M, written[i, -1] + 1) - 1} but stages image {int(b0[i, 0])} rows "
                       f"{int(y0[i, 0])} .. {int(y0[i, 0]) + th - 1} ({len(rows - pixels)} written pixels not staged)")
            break
    return "; ".join(why)


def halo_plan_fault(B, H, W, C1, C2, Cout, cfg):
    """(plan, fault) of the conv under tile_cfg = cfg; fault is '' when the plan names no halo tile or one the kernel can express."""
    _, ops = _ops()
    d = _conv(B, H, W, C1, C2, Cout)
    if not C2:
        d.X2 = None
    d.tile_cfg = cfg
    pl = ops._plan("conv", d)
    if pl[0] not in HALO:
        return pl, ""
    return pl, tile_faults(B, H, W, pl[2])


@pytest.mark.parametrize("cfg", MODES, ids=["heuristic"] + [f"tile{t}" for t in HALO])
def test_planned_halo_tile_covers_the_rows_it_stages(cfg):
    bad, halo = [], 0
    for (C1, C2, Cout), B, H, W in itertools.product(CHANNELS, BS, HS, WS):
        pl, fault = halo_plan_fault(B, H, W, C1, C2, Cout, cfg)
        halo += pl[0] in HALO
        if fault:
            bad.append(f"{B}x{H}x{W} ({C1}+{C2})->{Cout}: tile {pl[0]} split-K {pl[1]} BM {pl[2]}: {fault}")
    assert halo > 0                                                  # the sweep reaches the halo tiles at all
    assert not bad, f"{len(bad)} of {halo} halo plans hand the kernel a tile it cannot express, e.g.\n" + "\n".join(bad[:12])


# the shapes of a 512x768 request at its 12x8 level (and their kin): tile pixels are no whole number of images and no whole rows of one
SPLIT_IMAGE = [(4, 12, 8, 1280, 0, 1280), (4, 12, 8, 1280, 1280, 1280), (8, 12, 8, 1280, 0, 1280), (4, 12, 8, 256, 0, 256), (4, 12, 16, 128, 0, 128),
               (4, 24, 8, 128, 0, 128), (8, 6, 8, 256, 0, 256), (16, 3, 8, 256, 0, 256)]


@pytest.mark.parametrize("shape", SPLIT_IMAGE, ids=lambda s: "x".join(map(str, s)))
def test_maps_a_tile_would_split_run_the_gather_tiles(shape):
    """Neither the heuristic nor a requested halo tile (which falls back to the heuristic) lands on tiles 10 .. 14."""
    for cfg in MODES:
        pl, _ = halo_plan_fault(*shape, cfg)
        assert pl[0] not in HALO, (shape, cfg, pl)


@pytest.mark.parametrize("shape,tile,per_image", [((4, 24, 16, 640, 0, 640), 12, 3), ((4, 48, 32, 320, 0, 320), 10, 6), ((2, 96, 64, 320, 0, 320), 11, 48)])
def test_whole_row_tiles_of_non_square_maps_stay_halo(shape, tile, per_image):
    """Maps whose images hold a number of tiles that is no power of two keep their halo plan."""
    pl, fault = halo_plan_fault(*shape, -1)
    assert pl[0] == tile and not fault, (shape, pl, fault)
    assert geometry(shape[1], shape[2], pl[2])[3] == per_image


def test_geometry_model_rejects_the_split_image_tile():
    """The predicate can fail: 4 x 12 x 8 under a 128-pixel tile, and 16 x 3 x 8 (5 images of 24 pixels and 8 pixels of a sixth)."""
    assert "!= BM" in tile_faults(4, 12, 8, 128) and "tile 0 writes rows 0 .. 127 but stages image 0 rows 0 .. 11 (32 " in tile_faults(4, 12, 8, 128)
    assert tile_faults(16, 3, 8, 128) and tile_faults(8, 12, 8, 256) and tile_faults(4, 12, 16, 256)
    for ok in ((4, 8, 8, 128), (16, 8, 8, 256), (2, 24, 32, 256), (8, 4, 8, 128), (1, 6, 128, 128), (1, 96, 64, 256), (2, 64, 64, 256)):
        assert tile_faults(*ok) == "", ok


def test_tuned_halo_entries_satisfy_the_contract():
    """Every conv entry of the tuned table that names a halo tile plans that tile and passes the predicate."""
    n = 0
    for key, value in tc.load_table().items():
        c = tc.Case(key, value)
        if c.form != "c" or c.tile not in HALO:
            continue
        p = tc.plan(c)
        assert (p[0], max(1, p[1])) == (c.tile, c.splits) or tc.case_of(key).planned == (c.tile, c.splits), (key, p)
        assert tile_faults(c.B, c.H, c.W, p[2]) == "", key
        n += 1
    assert n > 0
