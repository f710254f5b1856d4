"""The race screens' host side (tests/racescreen.py): exactness of every integer case, branch and tile coverage of the case table against
pbe_tile_info, the stale-slot diagnosis on emulated early reads.  Nothing is launched: the planners are host code."""
import ctypes as C

import pytest
import torch

import racescreen as rs


def test_tile_info_agrees_with_the_planner():
    """pbe_tile_info's BM and BN are what pbe_gemm_plan / pbe_conv3x3_prologue report for every tile a case forces, and the table ends
    where the entry says so."""
    from pbe_amd import lib
    T = rs.tiles()
    assert lib.load().pbe_tile_info(len(T), (C.c_int32 * 8)()) != 0 and lib.load().pbe_tile_info(-1, (C.c_int32 * 8)()) != 0
    seen = set()
    for cs in rs.cases():
        if cs.tile in seen or cs.kind == "conv":
            continue
        seen.add(cs.tile)
        d, mx = rs.gemm_desc(cs)
        with rs.forced(cs.tile, cs.splits) as ops:
            pl = ops._plan("mx8" if mx is not None else "gemm", d, mx)
        assert (pl[0], pl[2], pl[3]) == (cs.tile, T[cs.tile]["bm"], T[cs.tile]["bn"]), (cs.id, pl, T[cs.tile])
    for cs in rs.cases():                         # the halo tiles plan convs only
        if cs.kind == "conv" and cs.tile not in seen:
            seen.add(cs.tile)
            out = (C.c_int32 * 32)()
            with rs.forced(cs.tile, cs.splits):
                assert lib.load().pbe_conv3x3_prologue(C.byref(rs.conv_desc(cs)), out) == 0
            assert (out[0], out[2], out[3], out[29]) == (cs.tile, T[cs.tile]["bm"], T[cs.tile]["bn"], T[cs.tile]["hpa"]), (cs.id, list(out))
    assert seen == set(range(len(T))), f"tiles no case forces: {sorted(set(range(len(T))) - seen)}"
    for t in T:
        assert 2 <= t["s"] <= 4 and t["bm"] % 16 == 0 and t["bn"] % 16 == 0 and t["slots"] >= 1


def test_every_case_runs_the_tile_and_split_it_names():
    for cs in rs.cases():
        pl = rs.plan(cs)
        assert (pl["tile"], pl["splits"]) == (cs.tile, cs.splits), (cs.id, pl)
        assert pl["mode"] == (0 if cs.kind != "conv" else 1 if cs.struct == "R" else 2), (cs.id, pl)


def test_cases_cover_every_wait_branch_and_every_tile():
    """The union of the cases' branch sets is every (structure, depth, branch) of the universe - which is enumerated from pbe_tile_info,
    not from the case table - and every tile appears in a case of each of its forms."""
    want = rs.universe()
    got = set().union(*(rs.branches(cs) for cs in rs.cases()))
    assert got == want, (sorted(want - got), sorted(got - want))
    depths = {(rs.structure(i), t["s"] - 1) for i, t in enumerate(rs.tiles()) if rs.structure(i) != "A"}
    assert {(b[0], b[1]) for b in want if b[0] != "A"} == depths
    by = lambda pred: {cs.tile for cs in rs.cases() if pred(cs)}
    assert by(lambda c: c.kind == "gemm" and not c.f8) == set(rs.tiles_of(rs.F_DENSE))
    assert by(lambda c: c.kind == "conv" and c.struct == "R") == set(rs.tiles_of(rs.F_CONV))
    assert by(lambda c: c.kind == "conv" and c.struct != "R") == set(rs.tiles_of(rs.F_HALO))
    assert by(lambda c: c.f8) == set(rs.tiles_of(rs.F_F8))
    assert by(lambda c: c.struct == "A") == set(rs.tiles_of(rs.F_ASTAT))
    # the slices the issue names: a split-K slice shorter than the ring is deep, a gather slice resuming inside a block, a halo slice from block 2
    for cs in rs.cases():
        sl = rs.plan(cs)["slices"]
        if cs.id.endswith("-split5"):
            assert min(c for _, c in sl) < cs.S - 1, (cs.id, sl)
        if cs.id.startswith("R-conv") and cs.id.endswith("-split2"):
            assert sl[1][0] % 9 != 0, (cs.id, sl)
        if "halo" in cs.id and cs.id.endswith("-split2"):
            assert sl[1][0] > 0, (cs.id, sl)


INT_CASES = [cs.id for cs in rs.cases() if cs.family == "int" and cs.kind in ("gemm", "conv")]


@pytest.mark.parametrize("cid", INT_CASES)
def test_integer_case_is_exact(cid):
    """Every output of the case is an integer multiple of a power of two no larger than 2048 in magnitude (exact in fp16, before and after
    the residual add) and sum |a||w| < 2^24 along K (every fp32 partial exact in any order): conditions on the inputs alone."""
    cs = rs.case(cid)
    top, s = rs.exactness(cs)
    assert top <= 2048.0 and s < 2 ** 24, (cid, top, s)
    if cs.f8:                                     # the same integers as e4m3 bytes: the conversion is exact
        p = rs.gemm_pools(cs)
        for k in ("a", "w"):
            assert torch.equal(p[k].float().to(torch.float8_e4m3fn).float(), p[k].float())


DIAG = [("R-dense-t9-nk5", 3, 1, 4), ("R-dense-t1-nk7", 0, 0, 5), ("R-dense-t18-nk9", 2, 1, 7), ("R-dense-t1-split5", 0, 1, 13),
        ("R-f8-t3-nk9", 1, 0, 6), ("R-conv-t9-c128", 5, 1, 11), ("R-conv-t3-kb128", 2, 0, 9), ("H2-halo-t10-c128", 3, 1, 13),
        ("H1-halo-t12-cat", 7, 0, 20), ("R-dense-t9-seam", 1, 1, 3)]


@pytest.mark.parametrize("cid,tm,tn,t", DIAG)
def test_diagnosis_names_the_stale_slot(cid, tm, tn, t):
    """One workgroup tile emulated with k-tile t - S in place of k-tile t - in one k-step half of both operands, or in the activations of
    one 16-row fragment: the diagnosis names the tile, the fragments and (t, t - S); the untouched output is reported clean."""
    cs = rs.case(cid)
    pools = rs.gemm_pools(cs) if cs.kind == "gemm" else rs.conv_pools(cs)
    ref = (rs.gemm_reference if cs.kind == "gemm" else rs.conv_reference)(cs, pools)
    want = rs.expand(cs, ref[1]).half()
    assert rs.diagnose(cs, want.clone(), want, pools) is None
    for mode, which in (("half", 0), ("half", 1), ("frag", 1)):
        got = rs.emulate_stale(cs, want, pools, tm, tn, t, mode, which)
        d = rs.diagnose(cs, got, want, pools)
        assert d is not None and d.tiles == [(tm, tn)], (cid, mode, str(d))
        assert d.stale is not None and d.stale[:2] == (t, t - cs.S), (cid, mode, str(d))
        rows = {f[0] for f in d.frags}
        assert rows == {1} if mode == "frag" else len(rows) > 1, (cid, mode, d.frags)
        assert ("k-step %d" % which in d.stale[2]) if mode == "half" else ("activations" in d.stale[2]), (cid, mode, str(d))
