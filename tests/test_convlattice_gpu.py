"""The gather conv kernel (igemm_kernel<MODE 1>) per element against fp64 on every tile that can run it, at every geometry, K order
(kblock) and split-K resume the entry point accepts (tests/convlattice.py; the host side and the proof that the gate can fail:
test_convlattice_cpu.py).

Every case fills pbe_conv3x3_desc directly, forces (tile, split-K) with ops.tune(1, ...), asserts from ops._PLANS that exactly that pair
ran, and compares EVERY output element of every sample with fp64 F.conv2d on the fp16 operands that were sent, under tilecheck's
rounding model clamped to the conv's _close limit.  One line per (geometry, kblock, tile, split) goes to convlattice_report.txt beside the
parity report (convlattice.report; committed copy: profiles/convlattice_report.txt)."""
import time

import pytest
import torch

import convlattice as cl
import guard
import tilecheck as tc
from convlattice import case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    cl.report(f"{'wall time of tests/test_convlattice_gpu.py':64s} {time.time() - t0:.1f} s")


def _line(cs, kb, tile, s, rep, extra=""):
    cl.report(f"{f'conv {cs.id} kblock {kb} tile {tile} split {s}':64s} err/bound={rep.ratio:.3f} at {rep.where} ({rep.n} elements){extra}")


def _gated(cs, dev, *, tile, splits=1, kblock=64, want=None, arena=False, note=""):
    res = cl.launch(cs, dev, tile=tile, splits=splits, kblock=kblock, want=want, arena=arena)
    what = f"conv {cs.id} kblock {kblock} tile {res['plan'][0]} split {res['plan'][1]}"
    rep = cl.compare(cs, res["y"], what)
    blocks = cl.check_group_stats(cs, res, what)
    _line(cs, kblock, *res["plan"], rep, (f" group_stats_blocks={blocks}" if blocks else "") + note)
    assert rep.ratio <= 1.0, str(rep)
    return res


def _same_bits(a, b, what):
    diff = guard.bits(a.contiguous()) != guard.bits(b.contiguous())
    assert not diff.any(), f"{what}: {int(diff.sum())} element(s) differ, first at {tuple(torch.nonzero(diff)[0].tolist())}"


# ---- every gather tile on every geometry --------------------------------------------------------------------------------------------------
def test_gather_tile_list(dev):
    """The lattice's tile list is the set of tiles the library runs in mode 1 when asked, on the base shape."""
    cs = case("base")
    got = [t for t in range(64) if (lambda p: p["tile"] == t and p["mode"] == 1)(cl.prologue(cs, 64, t | (1 << 8)))]
    assert got == cl.GATHER_TILES


@pytest.mark.parametrize("tile", cl.GATHER_TILES)
@pytest.mark.parametrize("geo", list(cl.GEOS))
def test_geometry_on_every_gather_tile(dev, geo, tile):
    """Every output element of the geometry on this tile within its bound; operands and output in arenas (guard.py), so a tap that
    reads past a border of the first or last sample meets NaN and a store outside Y is seen."""
    cs = case(geo)
    pro = cl.prologue(cs, 64, tile | (1 << 8))
    assert (pro["tile"], pro["splits"], pro["mode"]) == (tile, 1, 1), pro
    _gated(cs, dev, tile=tile, arena=True)                         # X / X2 / resid out of NaN arenas, Y in a sentinel arena


def test_group_statistics_from_the_gather_tiles(dev):
    """At 8 groups the lattice's channel counts (17 and 41 channels per group) divide no tile width, so no copy-out above emits group
    statistics.  This map's do (16 channels per group, 256 pixels per sample): every gather tile runs it, each one that reports blocks
    is compared with fp64 sums of its stored output, and some tile must report."""
    cs = case("gs")
    emitted = {}
    for tile in cl.GATHER_TILES:
        res = _gated(cs, dev, tile=tile)
        if res["blocks"]:
            emitted[tile] = res["blocks"]
            assert res["blocks"] * cl.prologue(cs, 64, tile | (1 << 8))["bm"] == cs.Ho * cs.Wo
    assert emitted, "no gather tile emitted group statistics"


# ---- split-K: resumes at a tap and inside the second source ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", cl.SPLIT_TILES)
def test_split_k_resume(dev, tile):
    """The widened concat (128 + 128) at every split-K request the planner honours (2 <= s <= nk / 4); over them a slice resumes at a tap
    other than 0 and a slice resumes inside the second source - asserted from split_per before anything is launched."""
    cs = case("cat", 128, 128)
    hon = cl.honoured(cs, 64, tile)
    sl = [x for _, pro in hon for x in cl.slices(cs, 64, pro["split_per"])]
    assert len(hon) >= 5 and any(tap for _, _, tap, _, _ in sl) and any(c0 > cs.C1 or (c0 == cs.C1 and tap) for _, _, tap, _, c0 in sl), (hon, sl)
    for s, pro in hon:
        assert pro["mode"] == 1 and pro["per_blk"] == 9
        _gated(cs, dev, tile=tile, splits=s, arena=True)


@pytest.mark.parametrize("kblock", [64, 128])
@pytest.mark.parametrize("tile", cl.SPLIT_TILES)
def test_phase_form_never_splits(dev, tile, kblock):
    """The phase form honours no split-K request (its four phases ride the grid's batch dimension; the slabs have none): the request
    runs as split 1 and passes the gate.  (So no phase slice resumes at tap != 0 of 4: there is no such plan - DESIGN.md.)"""
    cs = case("phase")
    assert cl.honoured(cs, kblock, tile) == []
    _gated(cs, dev, tile=tile, splits=2, kblock=kblock, want=(tile, 1), note=" (split 2 requested)")


# ---- kblock > 64 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
@pytest.mark.parametrize("tile", cl.KB_TILES)
@pytest.mark.parametrize("c1,c2,kb", cl.KB_CHANNELS)
@pytest.mark.parametrize("geo", cl.KB_GEOS)
def test_kblock(dev, geo, c1, c2, kb, tile, split):
    """KB = kblock / 64 > 1 k-tiles per (block, tap) visit: the kj walk, c0 -= cb, and - split - a slice that resumes at kj != 0.  Run
    plain and with X / X2 / resid out of NaN arenas and Y in a sentinel arena: the same bits, nothing outside Y written."""
    cs = case(geo, c1, c2)
    s = 1
    if split:
        s, pro = cl.kj_split(cs, kb, tile)
        KB = kb // 64
        assert pro["per_blk"] == 9 * KB and any((z * pro["split_per"]) % pro["per_blk"] % KB for z in range(s)), pro
    plain = _gated(cs, dev, tile=tile, splits=s, kblock=kb)
    padded = _gated(cs, dev, tile=tile, splits=s, kblock=kb, arena=True, note=" (arenas)")
    assert torch.isfinite(padded["y"].float()).all()
    _same_bits(padded["y"], plain["y"], f"conv {cs.id} kblock {kb} tile {tile} split {s}")


@pytest.mark.parametrize("tile", cl.KB_TILES)
def test_phase_form_at_kblock_128(dev, tile):
    """upsample = 2 at kblock = 128: the 4-tap K order k = ((ci / cb) * 4 + tap) * cb + ci % cb of include/pbe_hip.h, plain and in arenas."""
    cs = case("phase")
    plain = _gated(cs, dev, tile=tile, kblock=128)
    padded = _gated(cs, dev, tile=tile, kblock=128, arena=True, note=" (arenas)")
    _same_bits(padded["y"], plain["y"], f"conv {cs.id} kblock 128 tile {tile}")


def test_halo_request_at_kblock_128_runs_a_gather_tile(dev):
    """A map tile 11 takes at kblock 64: the same request at kblock 128 resolves to a gather tile and passes the gate, and so does the
    kblock 64 launch on that tile and split.  The two are the same conv in another order of the 64-wide k-tiles - (block of 128, tap, half)
    against (block of 64, tap) - so their fp32 sums may round differently: both are gated, the differing elements are counted in the
    report, and they differ by no more than the two bounds allow."""
    cs = case("halo11")
    at64, at128 = cl.prologue(cs, 64, 11 | (1 << 8)), cl.prologue(cs, 128, 11 | (1 << 8))
    assert (at64["tile"], at64["mode"]) == (11, 2) and at128["mode"] == 1 and at128["tile"] in cl.GATHER_TILES
    want = (at128["tile"], max(1, at128["splits"]))
    _gated(cs, dev, tile=11, kblock=64, want=(11, 1))
    wide = _gated(cs, dev, tile=11, kblock=128, want=want, note=" (tile 11 requested)")
    narrow = _gated(cs, dev, tile=want[0], splits=want[1], kblock=64)
    diff = guard.bits(wide["y"].contiguous()) != guard.bits(narrow["y"].contiguous())
    _, bound = cl.reference(cs)
    assert ((wide["y"].double() - narrow["y"].double()).abs().reshape(cs.M, cs.Cout) <= 2 * bound).all()
    cl.report(f"{f'conv {cs.id} kblock 128 vs 64 tile {want[0]} split {want[1]}':64s} {int(diff.sum())} of {diff.numel()} elements differ")


@pytest.mark.parametrize("geo,c1,c2,kb", [("base", 128, 0, 96), ("base", 192, 0, 128), ("cat", 128, 64, 128), ("phase", 128, 0, 96)])
def test_bad_kblock_is_refused(dev, geo, c1, c2, kb):
    """PBE_EINVAL, and not one byte of the output arena written."""
    assert cl.refused(case(geo, c1, c2), dev, kb) == cl.PBE_EINVAL


# ---- the gate can fail on the device -------------------------------------------------------------------------------------------------------------
def test_gate_rejects_wrong_kblock_pack(dev):
    """Weights packed at cb = 64, launched as kblock = 128."""
    cs = case("base", 256, 0)
    res = cl.launch(cs, dev, tile=3, kblock=128, wp=cl.packed(cs, 64))
    rep = cl.compare(cs, res["y"], "wrong-kblock pack")
    cl.report(f"{'conv control: cb 64 pack at kblock 128':64s} err/bound={rep.ratio:.3f} at {rep.where} (must exceed 1)")
    assert rep.ratio > 1.0, f"not detected: {rep}"


def test_gate_rejects_zeroed_last_kslice(dev):
    """tilecheck's zeroed last 64-wide k-slice, at kblock = 192 with split-K."""
    cs = case("base", 192, 0)
    s, _ = cl.kj_split(cs, 192, 9)
    res = cl.launch(cs, dev, tile=9, splits=s, kblock=192, wp=tc._zero_last_kslice(cl.packed(cs, 192)))
    rep = cl.compare(cs, res["y"], "zeroed last k-slice")
    cl.report(f"{'conv control: last k-slice zeroed':64s} err/bound={rep.ratio:.3f} at {rep.where} (must exceed 1)")
    assert rep.ratio > 1.0, f"not detected: {rep}"
