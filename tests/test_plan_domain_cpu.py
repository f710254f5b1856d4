"""The accepted domain of pbe_gemm_plan, host only: a deterministic lattice of descriptors (full products of short lists, stand-in pointers
that are never dereferenced) over shapes, epilogue forms, requested tiles / split-K factors and workspaces.  For every descriptor the
plan call either refuses with PBE_EINVAL or returns a plan whose invariants hold - the ones the launch relies on without checking them
again (igemm_kernel.h: the V^T tiles of a column tile, the split-K slabs, the row-statistics partials per column tile).

Then the launches SpatialTransformer.run_paired makes under pinned_batch_scale(2) with row statistics (proj_in, to_out), driven through
ops._launch itself with the library's launch entry replaced by a recorder: the descriptor that would be launched at batch B plans the
split-K factor and the tile width (= statistics partials, their fp32 summation order) of the 2B launch, or ops._PIN_MISSES says so."""
import ctypes as C
import itertools
import warnings

import pytest

P = 1 << 20                                          # 16-byte aligned stand-in address (never read)
EINVAL = -1

# (BM, BN) per tile config index (igemm_kernel.h, kTiles) and the tiles an extended-epilogue problem may run
TILES = [(256, 256), (256, 128), (128, 256), (128, 128), (128, 64), (64, 128), (64, 64), (256, 320), (128, 320), (128, 160),
         (256, 160), (128, 160), (128, 320), (256, 128), (128, 128), (128, 128), (128, 64), (64, 64), (128, 160),
         (128, 128), (128, 160), (256, 160)]
EX_TILES = {3, 4, 5, 6, 8, 9, 15, 16, 17, 18}        # streaming extended-epilogue tiles
ASTAT_TILES = {19, 20}                               # A-stationary

MS = (1, 7, 64, 65, 200, 1000, 4096)
NS = (4, 12, 72, 96, 120, 136, 240, 328, 600, 960, 2560)
KS = (8, 40, 72, 136, 320, 1280, 5120)
TILE_CFGS = (-1,) + tuple(t | (s << 8) for t in range(len(TILES)) for s in (0, 1, 3, 32))
WORKSPACES = ((None, 0), (P, 4 << 10), (P, 64 << 20))
FORMS = ("plain", "row_stats", "ln", "qkv8", "qkv64")


def _cdiv(a, b):
    return -(-a // b)


def _ops():
    from pbe_amd import lib, ops
    lib.load()
    return lib, ops


def _gemm(M, N, K, **kw):
    """2-D fp16 GEMM x [M, K] w [N, K] -> [M, N] with bias and the split-K workspace of ops.gemm, extra fields from kw."""
    lib, ops = _ops()
    d = lib.GemmDesc(P, None, P, P, P, None, None, M, N, K, K, K, 0, K, N, 0, 0, 0, 0, 0, 0, 0, 1, 1.0, 0, 0, P, ops.SPLITK_WS_BYTES, -1)
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def _form(form, M, N, K):
    """The descriptor of one lattice point, or None where the form has no such point (q|k|V^T: N = 3 * inner)."""
    if form == "plain":
        return _gemm(M, N, K)
    if form == "row_stats":
        return _gemm(M, N, K, row_stats_out=P, row_stats_ld=M)
    ln = dict(ln_stats=P, ln_parts=1, ln_stats_ld=M, ln_colsum=P, ln_eps=1e-5)
    if form == "ln":
        return _gemm(M, N, K, **ln)
    if N % 3:
        return None
    inner, tokens = N // 3, int(form[3:])
    return _gemm(M, N, K, ldc=2 * inner, alpha_cols=inner, VT=P, vt_col0=2 * inner, vt_tokens=tokens, vt_bs=inner * tokens, vt_rs=tokens, **ln)


def _check_plan(d, out, need, ws_bytes, ex):
    """The plan invariants of an accepted descriptor; returns the first broken one as text, or None."""
    cfg, split, bm, bn, wgs, parts = out
    if not (0 <= cfg < len(TILES)) or (bm, bn) != TILES[cfg]:
        return f"tile {cfg} reported as {bm} x {bn}"
    if split < 1 or wgs != _cdiv(d.M, bm) * _cdiv(d.N, bn) * d.batch * split:
        return f"{wgs} workgroups for split-K {split}"
    if parts != _cdiv(d.N, bn):
        return f"{parts} column tiles"
    if ex and (split != 1 or cfg not in EX_TILES | ASTAT_TILES):
        return f"extended epilogue on tile {cfg}, split-K {split}"
    if d.VT and d.vt_col0 % bn:
        return f"vt_col0 % BN = {d.vt_col0 % bn}: the V^T columns start inside a tile"
    if split > 1:
        nk = _cdiv(d.K, 64)
        per = _cdiv(nk, split)
        if need != split * d.M * d.N * 4 or need > ws_bytes:
            return f"split-K {split} needs {need} bytes of a {ws_bytes}-byte workspace"
        if _cdiv(nk, per) != split:
            return f"split-K {split} over {nk} k-tiles leaves an empty slice"
        if split > nk // 4 or d.N % 4:
            return f"split-K {split} over {nk} k-tiles, N = {d.N}"
    elif need:
        return f"{need} workspace bytes without split-K"
    return None


@pytest.mark.parametrize("form", FORMS)
def test_every_accepted_descriptor_plans_consistently(form):
    lib, _ = _ops()
    plan = lib.load().pbe_gemm_plan
    out, need = (C.c_int32 * 6)(), C.c_size_t()
    ex = form != "plain"
    bad, accepted, refused = [], 0, 0
    for M, N, K in itertools.product(MS, NS, KS):
        d = _form(form, M, N, K)
        if d is None:
            continue
        ref = C.byref(d)
        for (ws, ws_bytes), cfg in itertools.product(WORKSPACES, TILE_CFGS):
            d.workspace, d.workspace_bytes, d.tile_cfg = ws, ws_bytes, cfg
            rc = plan(ref, out, C.byref(need))
            if rc == 0:
                accepted += 1
                why = _check_plan(d, list(out), need.value, ws_bytes, ex)
            else:
                refused += 1
                why = None if rc == EINVAL else f"refused with code {rc}"
            if why:
                bad.append(f"M={M} N={N} K={K} tile_cfg={cfg:#x} workspace={ws_bytes}: {why}; plan {list(out)}")
    print(f"{form}: {accepted} plans checked, {refused} descriptors refused, {len(bad)} broken")
    assert accepted > 0 and (form != "plain" or refused == 0)
    assert not bad, f"{len(bad)} of {accepted} accepted descriptors break a plan invariant, e.g.\n" + "\n".join(bad[:12])


FUSABLE = (32, 64, 80, 96, 160, 192, 320)            # inner widths (heads x dim_head) whose 2 * inner some extended-epilogue tile width divides
UNFUSABLE = (24, 40, 48, 200)


@pytest.mark.parametrize("tokens", [8, 64])
def test_fused_projection_is_refused_where_no_tile_divides_vt_col0(tokens):
    """q | k | V^T: accepted widths plan a tile that divides vt_col0; the others are refused by name, under the heuristic and under
    every requested tile alike, and ops.qkv_fusable (what the transformer block asks) says the same."""
    lib, ops = _ops()
    for inner in FUSABLE + UNFUSABLE:
        for cfg in (-1,) + tuple(range(len(TILES))):
            d = _form(f"qkv{tokens}", 1000 // tokens * tokens, 3 * inner, 40)
            d.tile_cfg = cfg
            if inner in FUSABLE:
                pl = ops._plan("gemm", d)
                assert d.vt_col0 % pl[3] == 0 and pl[0] in EX_TILES | ASTAT_TILES and pl[1] == 1, (inner, cfg, pl)
            else:
                with pytest.raises(lib.PbeError, match="vt_col0"):
                    pl = ops._plan("gemm", d)
                    pytest.fail(f"inner {inner}, tile_cfg {cfg}: planned {pl}: vt_col0 % BN = {d.vt_col0 % pl[3]}")
        assert ops.qkv_fusable(inner) == (inner in FUSABLE), inner


# ---- row-statistics launches under pinned_batch_scale --------------------------------------------------------------------------------
def _proj_in(B, N, C_):
    return _gemm(B * N, C_, C_)


def _to_out(B, N, C_):
    return _gemm(B * N, C_, C_, rowvec=P, ldv=C_, group_rows=N, resid=P, ldr=C_)


PINNED = {"proj_in": _proj_in, "to_out": _to_out}
WIDTHS = (32, 64, 96, 128, 192, 320, 640, 960, 1280)
TOKENS = (8, 64, 96, 256, 384, 1024, 2304, 4096, 9216)
BATCHES = (1, 2, 3, 4, 5, 8, 16)


class _Recorder:
    """The loaded library with pbe_gemm_f16 replaced: the descriptor is copied, nothing is launched."""

    def __init__(self, real):
        self._real, self.launched = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def pbe_gemm_f16(self, dref, stream):
        d = dref._obj
        self.launched.append(type(d).from_buffer_copy(d))
        return 0


class _Stats:
    """What ops._launch takes from the row_stats callback: where the partials go."""

    def __init__(self, M):
        self.ld = M

    def ptr(self):
        return P


def test_pinned_row_statistics_launch_takes_the_plan_of_twice_the_batch(monkeypatch):
    lib, ops = _ops()
    rec = _Recorder(lib.load())
    monkeypatch.setattr(lib, "load", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    ops._PIN_CACHE.clear()
    silent, total = [], 0
    for name, B, N, C_ in itertools.product(sorted(PINNED), BATCHES, TOKENS, WIDTHS):
        total += 1
        d, big = PINNED[name](B, N, C_), PINNED[name](2 * B, N, C_)
        big.row_stats_out, big.row_stats_ld = P, 2 * B * N
        big.tile_cfg = ops._TUNED.get(ops._key("gemm", big, True), -1)
        want = ops._plan("gemm", big)
        misses = len(ops._PIN_MISSES)
        del rec.launched[:]
        with warnings.catch_warnings(), ops.pinned_batch_scale(2):
            warnings.simplefilter("ignore")           # a recorded miss also warns; the record is what this test reads
            ops._launch("gemm", d, row_stats=lambda parts, M=B * N: _Stats(M))
        assert len(rec.launched) == 1 and rec.launched[0].row_stats_out == P
        got = ops._plan("gemm", rec.launched[0])
        if (got[1], got[3]) != (want[1], want[3]) and len(ops._PIN_MISSES) == misses:
            silent.append(f"{name} B={B} N={N} C={C_}: launches tile {got[0]} (BN {got[3]}, split-K {got[1]}), the 2B launch runs "
                          f"tile {want[0]} (BN {want[3]}, split-K {want[1]})")
    assert total == 1134
    assert not silent, f"{len(silent)} of {total} pinned launches silently differ from the 2B launch, e.g.\n" + "\n".join(silent[:8])

