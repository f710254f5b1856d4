"""The gather conv lattice without a GPU (tests/convlattice.py): the packer, the host planner's side of the lattice, and the proof that the
gate can fail.

The fp32 restatement of igemm_kernel<MODE 1> (convlattice.emulate: never a kernel's output) must pass the per-element gate on every
lattice case - no case is impossible - and every mutant of it must be rejected on every case it applies to."""
import pytest
import torch

import convlattice as cl
from convlattice import case


def _lib():
    from pbe_amd import lib
    return lib.load()


# ---- the packer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [None, (64, 128), (128, 128)])
def test_packer_equals_ops_at_64(split):
    """k = ((ci / cb) * 9 + tap) * cb + ci % cb at cb = 64 is ops.pack_conv3x3, bit for bit, for one source and for a concat."""
    from pbe_amd import ops
    ci = sum(split) if split else 192
    w = (torch.randn(40, ci, 3, 3, generator=torch.Generator().manual_seed(ci)) / 30).half()
    mine = cl.pack_k(w.reshape(40, ci, 9), 64)
    assert torch.equal(mine.view(torch.int16), ops.pack_conv3x3(w.float(), split=split).view(torch.int16))


def test_phase_packer_equals_ops_at_64():
    from pbe_amd import ops
    w = torch.randn(24, 128, 3, 3, generator=torch.Generator().manual_seed(5)) / 30
    ph = cl.phase_weights(w)
    mine = torch.stack([cl.pack_k(ph[p], 64) for p in range(4)], 0)
    assert torch.equal(mine.view(torch.int16), ops.pack_conv3x3_up_phases(w).view(torch.int16))


@pytest.mark.parametrize("ci,cb", [(256, 128), (192, 192), (256, 256), (384, 128), (384, 192)])
@pytest.mark.parametrize("taps", [9, 4])
def test_packer_permutes_at_wider_blocks(ci, cb, taps):
    """At cb = 128 / 192 / 256 the pack is a permutation of the cb = 64 pack's columns, and not the identity."""
    wt = torch.randn(3, ci, taps, generator=torch.Generator().manual_seed(ci + cb)).half()
    idx = torch.arange(ci * taps, dtype=torch.float32).reshape(1, ci, taps)                        # the source element of each column
    a, b = cl.pack_k(idx, 64)[0], cl.pack_k(idx, cb)[0]
    assert torch.equal(a.sort().values, b.sort().values) and torch.equal(a.sort().values, torch.arange(ci * taps, dtype=torch.float32))
    assert not torch.equal(a, b)
    w64, wcb = cl.pack_k(wt, 64), cl.pack_k(wt, cb)
    perm = torch.empty(ci * taps, dtype=torch.long)
    perm[b.long()] = torch.arange(ci * taps)
    assert torch.equal(wcb[:, perm[a.long()]], w64)
    # the formula, element by element
    for c, t in ((0, 0), (63, taps - 1), (64, 0), (cb - 1, 1), (ci - 1, taps - 1), (ci - cb, 2)):
        assert b[((c // cb) * taps + t) * cb + c % cb] == c * taps + t


# ---- the host planner's side of the lattice ----------------------------------------------------------------------------------------------
def test_gather_tile_list_is_complete():
    """GATHER_TILES is exactly the set of tiles whose forced request runs as asked in mode 1 on the base shape: a new gather tile cannot
    stay outside the gate."""
    _lib()
    cs, got = case("base"), []
    for t in range(64):
        pro = cl.prologue(cs, 64, t | (1 << 8))
        if pro["tile"] == t and pro["mode"] == 1:
            got.append(t)
    assert got == cl.GATHER_TILES


@pytest.mark.parametrize("geo", list(cl.GEOS))
def test_every_gather_tile_is_honoured(geo):
    """Every geometry runs every gather tile when asked (mode 1, split 1), at kblock 64 and at each kblock of the kblock lattice."""
    _lib()
    todo = [(case(geo), 64)] + ([(case(geo, c1, c2), kb) for c1, c2, kb in cl.KB_CHANNELS] if geo in cl.KB_GEOS else [])
    for cs, kb in todo:
        for t in cl.GATHER_TILES:
            pro = cl.prologue(cs, kb, t | (1 << 8))
            assert (pro["tile"], pro["splits"], pro["mode"]) == (t, 1, 1), (cs.id, kb, t, pro)
            assert (pro["hw"], pro["per_blk"]) == (cs.Ho * cs.Wo if not cs.phase else cs.H * cs.W, cs.T * kb // 64), (cs.id, kb, pro)


def test_split_requests_reach_taps_and_the_second_source():
    """Split-K on the widened concat (128 + 128): over the honoured requests some slice resumes at a tap other than 0 and some slice
    resumes inside the second source.  The phase form honours no request: its four phases ride the grid's batch dimension, which the
    split-K workspace does not have (splitk_ok: batch 1) - so no phase slice can resume at tap != 0 of 4, and the gate holds the
    phase form to split 1."""
    _lib()
    wide = case("cat", 128, 128)
    for tile in cl.SPLIT_TILES:
        hon = cl.honoured(wide, 64, tile)
        assert [s for s, _ in hon] == [2, 3, 4, 5, 6, 8, 9], (tile, hon)         # nk = 36: 7 slices of 6 leave none for the 7th
        sl = [x for _, pro in hon for x in cl.slices(wide, 64, pro["split_per"])]
        assert any(tap for _, _, tap, _, _ in sl), sl
        assert any(c0 > wide.C1 or (c0 == wide.C1 and tap) for _, _, tap, _, c0 in sl), sl
    ph = case("phase")
    for kb in (64, 128):
        for tile in cl.SPLIT_TILES:
            assert cl.honoured(ph, kb, tile) == []
            pro = cl.prologue(ph, kb, tile | (2 << 8))
            assert (pro["tile"], pro["splits"], pro["per_blk"]) == (tile, 1, 4 * kb // 64)


@pytest.mark.parametrize("geo", cl.KB_GEOS)
@pytest.mark.parametrize("c1,c2,kb", cl.KB_CHANNELS)
def test_kblock_split_resumes_inside_a_visit(geo, c1, c2, kb):
    """The split-K request of each kblock case has a slice that starts at kj != 0: from split_per, per_blk and KB alone."""
    _lib()
    cs = case(geo, c1, c2)
    for tile in cl.KB_TILES:
        s, pro = cl.kj_split(cs, kb, tile)
        KB = kb // 64
        assert pro["per_blk"] == 9 * KB and pro["splits"] == s
        starts = [(z * pro["split_per"]) % pro["per_blk"] % KB for z in range(s)]
        assert any(starts), (cs.id, kb, tile, s, pro["split_per"])
        assert pro["mg_kb"] & 0xFFFFFFFF == (0xFFFFFFFF if KB == 1 else (1 << 32) // KB)


def test_kblock_contract_on_the_host():
    """kblock: 0 = 64; a multiple of 64 dividing C1 and C2 or PBE_EINVAL; a halo tile's request at kblock 128 resolves to a gather tile."""
    _lib()
    assert cl.prologue(case("base"), 0, 3 | (1 << 8))["per_blk"] == 9
    assert cl.prologue(case("base"), 96) == cl.PBE_EINVAL
    assert cl.prologue(case("base", 192, 0), 128) == cl.PBE_EINVAL
    assert cl.prologue(case("cat", 128, 64), 128) == cl.PBE_EINVAL
    assert cl.prologue(case("phase"), 96) == cl.PBE_EINVAL
    halo = case("halo11")
    at64, at128 = cl.prologue(halo, 64, 11 | (1 << 8)), cl.prologue(halo, 128, 11 | (1 << 8))
    assert (at64["tile"], at64["mode"]) == (11, 2)
    assert at128["mode"] == 1 and at128["tile"] in cl.GATHER_TILES


# ---- the gate can fail ---------------------------------------------------------------------------------------------------------------------
def _lattice():
    try:
        return cl.lattice()
    except Exception:                                              # library not built at collection time
        return []


LATTICE = _lattice()
_lid = lambda v: f"{v[0].id}-kb{v[1]}-sp{v[2] or 0}"


def test_lattice_was_collected():
    _lib()
    assert len(LATTICE) >= len(cl.GEOS) + 2 * 12 + 2


@pytest.mark.parametrize("item", LATTICE, ids=_lid)
def test_restatement_passes_the_gate(item):
    cs, kb, sp = item
    rep = cl.gate(cs, cl.emulate(cs, kb, sp), _lid(item))
    assert rep.ratio <= 1.0


@pytest.mark.parametrize("mutant", cl.MUTANTS)
def test_mutant_is_rejected_wherever_it_applies(mutant):
    hit = 0
    for item in LATTICE:
        cs, kb, sp = item
        if not cl.applies(mutant, cs, kb, sp):
            continue
        rep = cl.compare(cs, cl.emulate(cs, kb, sp, mutant=mutant), f"{mutant} on {_lid(item)}")
        assert rep.ratio > 1.0, f"not rejected: {rep}"
        hit += 1
    assert hit >= {"wrong_cb": 8, "replicate": 9, "no_shift": 2, "src_stride": 1, "resume_tap0": 3, "drop_kt": 3}[mutant], (mutant, hit)
