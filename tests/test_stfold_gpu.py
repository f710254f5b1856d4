"""The two SpatialTransformer folds on the GPU: the GroupNorm on proj_in's A operand (pbe_gemm_gnfold_f16) bit for bit against the
normalisation pass + GEMM, on every extended-epilogue tile; proj_out composed into ff-out against fp64, beside the two-launch chain; the
guidance pair and the whole block, new path against old."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard
import stfoldref as R

pytestmark = pytest.mark.gpu
EPS = 1e-6


def _ex_tiles():
    """(cfg, BM, BN) of the streaming extended-epilogue tiles (pbe_tile_info: form bit 8, neither A-stationary nor forced-only)."""
    from pbe_amd import lib
    info, out = (C.c_int32 * 8)(), []
    for cfg in range(64):
        if lib.load().pbe_tile_info(cfg, info) != 0:
            break
        if info[5] & 8 and not info[5] & 96:
            out.append((cfg, info[0], info[1]))
    assert len(out) >= 4
    return out


def _problem(B, tokens, C_, N, dev, seed):
    """x [B, tokens, C] fp16 with one group far from zero (|mean| / sigma = 1000) and one of zero variance; GroupStats from 2 row blocks."""
    from pbe_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, tokens, C_, generator=g)
    cg = C_ // 32
    x[:, :, cg:2 * cg] = 50.0 + 0.05 * x[:, :, cg:2 * cg]
    x[:, :, 2 * cg:3 * cg] = 3.0
    x = x.half().to(dev)
    gamma, beta = (1.0 + 0.3 * torch.randn(C_, generator=g)).to(dev), (0.2 * torch.randn(C_, generator=g)).to(dev)
    w, b = (torch.randn(N, C_, generator=g) / C_ ** 0.5).half().to(dev), torch.randn(N, generator=g).to(dev)
    part = R.partials_of(x, 32, 2)
    return x, ops.GroupStats(part, B, 2, 32, x._version), gamma, beta, w, b


class _forced:
    """Every launch inside takes tile `cfg` (no split-K); the launch keys are recorded."""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        from pbe_amd import ops
        ops._FORCE_CFG, ops._TIMES = (None if self.cfg is None else self.cfg | (1 << 8)), {}
        return self

    def __exit__(self, *exc):
        from pbe_amd import ops
        self.keys, ops._FORCE_CFG, ops._TIMES = list(ops._TIMES), None, None
        return False


def _folded(keys):
    return any(k.endswith("G") and "|" in k for k in keys)


def _stats_equal(a, b, M):
    return a.parts == b.parts and torch.equal(a.buf[:a.parts, :M], b.buf[:b.parts, :M])


@pytest.mark.parametrize("B,tokens,C_", [(2, 64, 64), (2, 128, 320), (3, 256, 640)])
def test_head_bit_for_bit_on_every_tile(dev, B, tokens, C_):
    """gemm(gn=...) equals gemm(groupnorm_apply(x)): torch.equal on the output and on the RowStats partials, on every extended-epilogue
    tile whose rows divide the sample (at (3, 256, 640) the 64-row tiles put four tiles into a sample, their edges on sample edges)."""
    from pbe_amd import ops
    x, st, gamma, beta, w, b = _problem(B, tokens, C_, C_, dev, 7)
    M = B * tokens
    xn = ops._groupnorm_apply(x, st, gamma, beta, EPS, False)
    sc, sh = R.gn_table_ref(st.view(), gamma, beta, tokens, EPS)
    ref_n = (x.double() * sc[:, None, :] + sh[:, None, :])
    assert (xn.double() - ref_n).abs().max().item() <= 2.0 ** -10 * max(1.0, ref_n.abs().max().item())      # the pass itself: one fp16 rounding of an fp32 fma
    ran = []
    for cfg, bm, bn in _ex_tiles():
        if tokens % bm:
            continue
        with _forced(cfg):
            ref, rst = ops.gemm(xn.view(M, C_), w, b, row_stats=True)
        with _forced(cfg) as f:
            out, ost = ops.gemm(x.view(M, C_), w, b, row_stats=True, gn=(st, gamma, beta, EPS))
        assert _folded(f.keys) and any(k.startswith("nt:") for k in f.keys) and not any(k.startswith("n:") for k in f.keys), (cfg, f.keys)
        assert ost.parts == -(-C_ // bn)
        assert torch.equal(out, ref), (cfg, (out.float() - ref.float()).abs().max().item())
        assert _stats_equal(ost, rst, M), cfg
        ran.append(cfg)
    assert len(ran) >= 3 and any(bm == 64 for cfg, bm, bn in _ex_tiles() if cfg in ran)
    with _forced(ran[0]) as f:                        # with a residual and without statistics (the same tile, unsplit, on both sides: a plain
        out = ops.gemm(x.view(M, C_), w, b, resid=xn.view(M, C_), gn=(st, gamma, beta, EPS))      # GEMM left to its planner may split K)
        ref = ops.gemm(xn.view(M, C_), w, b, resid=xn.view(M, C_))
    assert _folded(f.keys) and torch.equal(out, ref)
    with _forced(None) as f:                          # the planner's own pick launches the fold too
        ops.gemm(x.view(M, C_), w, b, gn=(st, gamma, beta, EPS))
    assert _folded(f.keys)


def test_head_table_matches_formula(dev):
    from pbe_amd import lib, ops
    x, st, gamma, beta, _, _ = _problem(2, 128, 320, 64, dev, 9)
    table = torch.empty((2, 640), dtype=torch.float32, device=dev)
    lib.check(lib.load().pbe_groupnorm_table_f32(st.buf.data_ptr(), st.blocks, gamma.data_ptr(), beta.data_ptr(), table.data_ptr(), 2, 128, 320, 32,
                                                 EPS, ops._stream()), "pbe_groupnorm_table_f32")
    sc, sh = R.gn_table_ref(st.view(), gamma, beta, 128, EPS)
    want = R.table_layout(sc, sh).view(2, 640)
    # fp32 roundings of an fp64 finalise: rstd, rstd gamma; mean, then one fused beta - mean sc, whose error scales with |mean sc| = |beta - sh|
    bound = 4 * 2.0 ** -24 * R.table_layout(sc.abs(), (beta.double()[None, :] - sh).abs() + sh.abs()).view(2, 640) + 1e-30
    assert torch.isfinite(table).all() and ((table.double() - want).abs() <= bound).all()


def test_head_ineligible_shapes_take_the_old_path(dev):
    """tokens % BM != 0 on every tile (40 tokens): the separate pass runs, and the result is the old path's."""
    from pbe_amd import ops
    x, st, gamma, beta, w, b = _problem(2, 40, 64, 64, dev, 11)
    xn = ops._groupnorm_apply(x, st, gamma, beta, EPS, False)
    with _forced(None) as f:
        out, ost = ops.gemm(x.view(80, 64), w, b, row_stats=True, gn=(st, gamma, beta, EPS))
    assert not _folded(f.keys) and any(k.startswith("n:") for k in f.keys) and not any(k.startswith("nt:") for k in f.keys), f.keys
    ref, rst = ops.gemm(xn.view(80, 64), w, b, row_stats=True)
    assert torch.equal(out, ref) and _stats_equal(ost, rst, 80)


def test_head_without_producer_statistics_takes_the_old_path(dev):
    """SpatialTransformer.run on an input that carries no statistics: the norm's own launches, the bits of fold_groupnorm = False; with
    statistics attached the fold runs and the bits stay."""
    from ldm.modules.attention import SpatialTransformer
    from pbe_amd import ops
    from pbe_amd.weights import fill_module_
    st = SpatialTransformer(64, 8, 8, depth=1, context_dim=768)
    fill_module_(st, prefix="st.")
    st = st.to(dev)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 8, 8, 64, generator=g).half().to(dev)
    ctx = torch.randn(2, 1, 768, generator=g).half().to(dev)
    with torch.no_grad():
        vecs = st.context_vectors(ctx)
        with _forced(None) as f0:
            y0 = st.run(x, vecs)
        assert not _folded(f0.keys)
        st.fold_groupnorm = False
        y1 = st.run(x, vecs)
        del st.fold_groupnorm
        x._pbe_gstats = ops.GroupStats(R.partials_of(x.view(2, 64, 64), 32, 1), 2, 1, 32, x._version)
        with _forced(None) as f2:
            y2 = st.run(x, vecs)
        assert _folded(f2.keys)
        st.fold_groupnorm = False
        y3 = st.run(x, vecs)                          # the normalisation pass from the same statistics
        del st.fold_groupnorm
    assert torch.equal(y0, y1) and torch.equal(y2, y3)


def test_head_padding_rows_and_canaries(dev):
    """M = 200 rows of 128-token samples on the 64-row tiles: the last tile holds 8 rows of sample 1 and 56 padding rows.  Nothing outside
    `out` and the statistics planes is written, every element inside is, and the bits are the old path's."""
    from pbe_amd import ops
    x, st, gamma, beta, w, b = _problem(2, 128, 64, 64, dev, 17)
    M, N = 200, 64
    xn = ops._groupnorm_apply(x, st, gamma, beta, EPS, False).view(256, 64)[:M]
    for cfg, bm, bn in _ex_tiles():
        if bm != 64:
            continue
        with _forced(cfg):
            ref, rst = ops.gemm(xn, w, b, row_stats=True)
        out, arena = guard.sentinel_out((M, N), col_pad=8, device=dev)
        sbuf, sarena = guard.sentinel_out((rst.parts * M * 2,), dtype=torch.float32, device=dev)
        with _forced(cfg) as f:
            _, ost = ops.gemm(x.view(256, 64)[:M], w, b, out=out, row_stats=ops.RowStats(sbuf, rst.parts, M), gn=(st, gamma, beta, EPS, 128))
        assert _folded(f.keys), f.keys
        guard.assert_untouched(arena, out, f"gnfold tile {cfg} out")
        guard.assert_untouched(sarena, sbuf, f"gnfold tile {cfg} statistics")
        guard.assert_fully_written(out, f"gnfold tile {cfg} out")
        guard.assert_fully_written(sbuf, f"gnfold tile {cfg} statistics")
        assert torch.equal(out, ref) and torch.equal(sbuf.view(rst.parts, M, 2), rst.buf[:rst.parts, :M]), cfg


# ---- tail ----
def _tail_errors(M, C_, dev, seed):
    """(chain (max, rms), composed (max, rms), rms of the reference) against fp64 for one random problem, both on the kernels."""
    from ldm.modules.attention import compose_tail
    from pbe_amd import ops
    h, x2, xin, wff, bff, wpo, bpo = R.tail_problem(M, C_, seed, dev)
    ref = R.tail_fp64(h, x2, xin, wff, bff, wpo, bpo)
    x3 = ops.gemm(h, wff.half(), bff, resid=x2)
    chain = ops.gemm(x3, wpo.half(), bpo, resid=xin)
    wt, bt = compose_tail(wpo, bpo, wff, bff)
    comp = ops.gemm(h, wt, bt, a2=x2, resid=xin)
    return R.err(chain, ref), R.err(comp, ref), (ref * ref).mean().sqrt().item()


@pytest.mark.parametrize("M,C_", [(2 * 64, 64), (2 * 128, 320), (2 * 64, 1280)])
def test_tail_against_fp64_beside_the_chain(dev, M, C_):
    """Per-element error of the composed launch and of the two-launch chain against fp64 from the master weights, same operands.  The
    composed form is not worse: rms at most the chain's; the maximum - one element's final fp16 rounding, which both forms share - at
    most 1.25 x the chain's (tests/test_stfold_cpu.py measures both conditions with the roundings emulated: rms 0.85 x, max 0.71 .. 1.16 x)."""
    (cmax, crms), (nmax, nrms), _ = _tail_errors(M, C_, dev, 0)
    print(f"tail M={M} C={C_}: chain max {cmax:.3e} rms {crms:.3e} | composed max {nmax:.3e} rms {nrms:.3e}")
    assert nrms <= crms and nmax <= 1.25 * cmax, ((cmax, crms), (nmax, nrms))


# ---- the modules ----
def _narrow_st(dev, depth=1):
    from ldm.modules.attention import SpatialTransformer
    from pbe_amd.weights import fill_module_
    st = SpatialTransformer(64, 8, 8, depth=depth, context_dim=768)
    fill_module_(st, prefix="st.")
    st.fold_tail = True                               # (as the U-Net builds its transformers; a stand-alone module defaults to the two launches)
    return st.to(dev)


@pytest.mark.parametrize("grid", [8, 16])
def test_guidance_pair_equals_run_on_the_duplicated_input(dev, grid):
    """SpatialTransformer.run_paired == run on cat([x, x]), bit for bit, both folds on (the identity the shared guidance prefix of the
    U-Net relies on); the input carries producer statistics, so proj_in folds the norm in both."""
    from pbe_amd import ops
    st = _narrow_st(dev)
    g = torch.Generator().manual_seed(19)
    B, N = 2, grid * grid
    x = torch.randn(B, grid, grid, 64, generator=g).half().to(dev)
    ctx = torch.randn(2 * B, 1, 768, generator=g).half().to(dev)
    part = R.partials_of(x.view(B, N, 64), 32, 1)
    x._pbe_gstats = ops.GroupStats(part, B, 1, 32, x._version)
    xd = torch.cat([x, x])
    xd._pbe_gstats = ops.GroupStats(torch.cat([part, part]), 2 * B, 1, 32, xd._version)
    with torch.no_grad():
        vecs = st.context_vectors(ctx)
        with _forced(None) as fp:
            yp = st.run_paired(x, vecs)
        with _forced(None) as fr:
            yr = st.run(xd, vecs)
        assert _folded(fp.keys) and _folded(fr.keys)
        gemms = lambda keys: sum(1 for k in keys if k[0] == "g")      # noqa: E731  (launch KEYS: proj_in, q|k|v, to_out, GEGLU, tail)
        st.fold_tail = False
        with _forced(None) as fo:
            st.run(xd, vecs)
        st.fold_tail = True
    assert torch.equal(yp, yr)
    assert not any(k.startswith("n:") for k in fr.keys) and gemms(fo.keys) == gemms(fr.keys) + 1      # no norm pass; proj_out's launch is gone


def test_whole_block_new_path_against_old(dev, golden_dir):
    """One SpatialTransformer forward on the golden block inputs: the new path (both folds) and the old (fold_tail = fold_groupnorm =
    False) against the reference module's st_y.  The new path stays inside the block tolerance, and its distance to it is the old
    path's less at most the tail's own measured error (relative rms of the composed launch against fp64 at this width)."""
    from test_model_gpu import BLOCK_TOL, rel_l2
    g = np.load(os.path.join(golden_dir, "blocks.npz"))
    T = lambda k: torch.from_numpy(g[k]).to(dev)      # noqa: E731
    st = _narrow_st(dev)
    with torch.no_grad():
        new = st(T("st_x"), T("st_ctx"))
        st.fold_tail = st.fold_groupnorm = False
        old = st(T("st_x"), T("st_ctx"))
        del st.fold_groupnorm
    _, (_, nrms), ref_rms = _tail_errors(128, 64, dev, 1)
    tail_err = nrms / ref_rms
    r_new, r_old = rel_l2(new, g["st_y"]), rel_l2(old, g["st_y"])
    print(f"SpatialTransformer C=64: rel-L2 old {r_old:.3e} new {r_new:.3e} (tolerance {BLOCK_TOL:.1e}); tail error {tail_err:.3e}")
    assert r_new <= BLOCK_TOL and BLOCK_TOL - r_new >= (BLOCK_TOL - r_old) - tail_err
