"""The extended-epilogue GEMM (pbe_gemm_f16 with alpha_cols / LayerNorm fold / row statistics / V^T) off the tuned table: every feature
combination on every streaming extended-epilogue tile, every inner width the fused q | k | V^T projection accepts, the alpha boundary at
the granularities the API allows, and the paired (shared guidance prefix) launches at shapes the table does not name.

Each launch is small (M = 200 rows, K = 136: two full k-tiles and a ragged one) and checked element by element: the reference is fp64
from the fp16 operands that were sent, the bound is the rounding model of tests/tilecheck.py (expect / clamp_to_close; no tolerance of
its own here).  Rows m % 97 == 0 of A carry +6.0 (mean >> std, the cancellation case of the fold).  Operands lie in NaN-poisoned arenas
with padded leading dimensions, C and V^T between sentinels with padded ldc / vt_rs / vt_bs: nothing outside the outputs is written and
no output element is skipped.  PBE_EX_LATTICE_REPORT=<file> appends one JSON line per launch (worst bound ratio, location)."""
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

import guard
import tilecheck as tc
from oracle_loader import O
from test_ctx_attention_gpu import check as check_rel_l2
from test_edges_gpu import _ln_parts, _stats
from test_model_gpu import BLOCK_TOL

pytestmark = pytest.mark.gpu

M, K = 200, 136
EX_TILES = (3, 4, 5, 6, 8, 9, 15, 16, 17, 18)       # the streaming extended-epilogue tiles (igemm_kernel.h, kTiles: F_EX)
ASTAT_TILES = (19, 20)

# feature combination -> the launch; the translation unit that instantiates it: ln, ln_geglu: igemm_ex_ln; stats_resid: igemm_ex_st;
# qkv: igemm_ex_qkv; the other five: igemm_ex_all
COMBOS = {
    "ln": dict(N=328, ln=1),
    "ln_geglu": dict(N=336, ln=1, act=4),
    "stats_resid": dict(N=328, stats=True, resid=True),
    "qkv": dict(N=960, ln=2, vt_col0=640, alpha_cols=320, tokens=40),
    "alpha": dict(N=328, alpha_cols=132),
    "ln_stats": dict(N=328, ln=1, stats=True),
    "ln_stats_alpha": dict(N=328, ln=1, stats=True, alpha_cols=132),
    "vt": dict(N=960, vt_col0=640, tokens=40),
    "stats_alpha": dict(N=328, stats=True, alpha_cols=132),
}


def _case(name, N, *, M=M, K=K, ln=0, act=0, stats=False, resid=False, vt_col0=0, alpha_cols=0, tokens=0):
    """ln: 0 = no fold, else the number of partials of the row statistics the fold reads."""
    return SimpleNamespace(name=name, M=M, N=N, K=K, ln=ln, act=act, stats=stats, resid=resid, vt=vt_col0 > 0, vt_col0=vt_col0,
                           alpha_cols=alpha_cols, alpha=tc.QSCALE if alpha_cols else 1.0, tokens=tokens, rowvec=False, batch=1,
                           close=tc.CLOSE["ln"] if ln else tc.CLOSE["gemm"])


def _launch(c, dev, cfg, *, mutate=False, outs=None):
    """One ops.gemm launch of case c with tile_cfg cfg (None: the heuristic) -> (t for tilecheck.reference_gemm, [(view, arena)] of the
    outputs, the launch's plan (tile, split-K, BM, BN, workgroups)).  outs: a list that receives the outputs as they are made (a launch
    that raises); nothing is planned ahead of such a launch, so that pbe_gemm_f16 itself answers."""
    from pbe_amd import ops
    g = torch.Generator().manual_seed(tc.seed_of(f"{c.name}:{c.M}:{c.N}:{c.K}"))
    a = torch.randn(c.M, c.K, generator=g) * 1.3
    a[::97] += tc.LN_OFFSET
    a = a.half()
    w = torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K)
    bias = torch.randn(c.N, generator=g) * 0.5
    t, kw = {}, {}
    if c.ln:
        gamma, beta = 1 + 0.1 * torch.randn(c.K, generator=g), 0.1 * torch.randn(c.K, generator=g)
        w, bias, t["colsum"] = ops.pack_linear_ln(w, bias, gamma, beta)
        kw["ln"] = (_stats(dev, True, _ln_parts(a, c.ln), c.M), guard.embed(t["colsum"], device=dev)[0], 1e-5)
    else:
        w = w.half()
    t["A"], t["W"], t["bias"] = a, w, bias
    if c.resid:
        t["resid"] = (torch.randn(c.M, c.N, generator=g) * 2).half()
        kw["resid"] = guard.embed(t["resid"], row_pad=1, col_pad=16, device=dev)[0]
    if c.alpha_cols:
        kw.update(alpha=c.alpha, alpha_cols=c.alpha_cols)
    if c.stats:
        kw["row_stats"] = True
    out_cols = c.N // 2 if c.act == 4 else (c.vt_col0 if c.vt else c.N)
    out, arena = guard.sentinel_out((c.M, out_cols), row_pad=1, col_pad=16, device=dev)
    record, outs = outs is None, [] if outs is None else outs
    outs.append((out, arena))
    if c.vt:
        vt, vt_arena = guard.sentinel_out((c.M // c.tokens, c.N - c.vt_col0, c.tokens), row_pad=3, col_pad=8, device=dev)
        outs.append((vt, vt_arena))
        kw.update(vt=vt, vt_col0=c.vt_col0, vt_tokens=c.tokens)
        t["vt_buf"] = vt
    wd = tc._zero_last_kslice(w) if mutate else w
    try:
        ops._PLANS, ops._FORCE_CFG = [] if record else None, cfg
        r = ops.gemm(guard.embed(a, row_pad=2, col_pad=8, device=dev)[0], guard.embed(wd, row_pad=1, col_pad=8, device=dev)[0],
                     guard.embed(bias, device=dev)[0], act=c.act, out=out, **kw)
        plans = ops._PLANS
    finally:
        ops._PLANS, ops._FORCE_CFG = None, None
    assert not record or len(plans) == 1, plans
    t["out"] = out
    if c.stats:
        t["stats"] = r[1]
    return t, outs, plans[0][1:] if record else None


def _report(c, plan, rep):
    path = os.environ.get("PBE_EX_LATTICE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=c.name, M=c.M, N=c.N, K=c.K, alpha_cols=c.alpha_cols, tokens=c.tokens, tile=plan[0], ratio=rep.ratio,
                                    where=rep.where, n=rep.n)) + "\n")


def _verify(c, t, outs, plan):
    """Every element of C and V^T within its bound, nothing outside them written, none skipped; the row statistics are the fp64 sums of
    the stored output (the limits of test_tuned_table_gpu.py)."""
    what = f"{c.name} {c.M}x{c.N}x{c.K} tile {plan[0]}"
    for i, (view, arena) in enumerate(outs):
        guard.assert_untouched(arena, view, f"{what} [output {i}]")
        guard.assert_fully_written(view, f"{what} [output {i}]")
    got, want, bound, labels = tc.reference_gemm(c, t, [(0, list(range(c.M)))])
    assert got.shape == want.shape == (c.M, c.N // 2 if c.act == 4 else c.N)
    rep = tc.compare(got, want, bound, what, labels)
    print(rep)
    _report(c, plan, rep)
    assert rep.ratio <= 1.0, str(rep)
    if c.stats:
        st = t["stats"]
        assert st.parts == -(-c.N // plan[3]), (what, st.parts)
        s = st.buf[:st.parts].double().sum(0)
        yd = t["out"].double()
        ref = torch.stack([yd.sum(1), (yd ** 2).sum(1)], 1)
        assert torch.allclose(s, ref, rtol=2e-6, atol=1e-4), f"{what}: row statistics off by {(s - ref).abs().max().item():.3e}"
    return rep


# ---- 1. form x tile ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", EX_TILES)
@pytest.mark.parametrize("combo", list(COMBOS))
def test_every_form_on_every_tile(dev, combo, tile):
    c = _case(combo, **COMBOS[combo])
    with torch.no_grad():
        t, outs, plan = _launch(c, dev, tile | (1 << 8))
        assert (plan[0], max(1, plan[1])) == (tile, 1), f"{combo}: the launch ran tile {plan[0]} split-K {plan[1]}, not tile {tile}"
        _verify(c, t, outs, plan)


@pytest.mark.parametrize("combo", ["ln", "stats_resid", "qkv", "alpha"])
def test_lattice_gate_rejects_zeroed_last_kslice(dev, combo):
    """One launch per translation unit with the last 64-wide k-slice of W zeroed in the device copy: rejected against the reference of
    the intact operands (the gate can fail)."""
    c = _case(combo, **COMBOS[combo])
    with torch.no_grad():
        t, _, plan = _launch(c, dev, 9 | (1 << 8), mutate=True)
        assert plan[0] == 9
        got, want, bound, labels = tc.reference_gemm(c, t, [(0, list(range(c.M)))])
    rep = tc.compare(got, want, bound, combo, labels)
    assert rep.ratio > 1.0, f"zeroed k-slice not detected: {rep}"


# ---- 2. widths of the fused q | k | V^T projection ----------------------------------------------------------------------------------------
def _qkv(inner, tokens):
    return _case(f"qkv{inner}", 3 * inner, M=3 * tokens, ln=2, vt_col0=2 * inner, alpha_cols=inner, tokens=tokens)


@pytest.mark.parametrize("tokens", [8, 72])
@pytest.mark.parametrize("inner", [32, 64, 80, 96, 160, 192, 320])
def test_fused_projection_accepted_widths(dev, inner, tokens):
    """The heuristic's tile: its width divides vt_col0 (inner 80: q | k in one 160-wide tile with the alpha boundary inside it, and a
    ragged V^T tile)."""
    c = _qkv(inner, tokens)
    with torch.no_grad():
        t, outs, plan = _launch(c, dev, None)
        assert plan[0] in EX_TILES + ASTAT_TILES and max(1, plan[1]) == 1 and c.vt_col0 % plan[3] == 0, plan
        _verify(c, t, outs, plan)


@pytest.mark.parametrize("tokens", [8, 72])
@pytest.mark.parametrize("inner", [24, 40, 48, 200])
def test_fused_projection_refused_widths_write_nothing(dev, inner, tokens):
    """No extended-epilogue tile width divides vt_col0 = 2 * inner: PbeError before anything is launched, both output arenas intact."""
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    c = _qkv(inner, tokens)
    assert not ops.qkv_fusable(inner, tokens)
    seen = []
    with pytest.raises(PbeError, match="pbe_gemm_f16.*vt_col0"):
        _launch(c, dev, None, outs=seen)
    torch.cuda.synchronize()
    assert len(seen) == 2
    for view, arena in seen:
        assert bool((guard.bits(arena) == guard.SENTINEL_BITS[arena.dtype]).all()), f"inner {inner}: the refused launch wrote to an output arena"


@pytest.mark.parametrize("C,heads", [(64, 1), (320, 5)])
def test_spatial_transformer_unfusable_width_takes_the_unfused_path(dev, C, heads):
    """dim_head 40 with 1 / 5 heads (inner 40 / 200): the block runs the separate LayerNorm, q | k and V^T launches and matches the oracle."""
    from ldm.modules.attention import SpatialTransformer
    from pbe_amd import ops
    from pbe_amd.weights import fill_module_
    st = SpatialTransformer(C, heads, 40, depth=1, context_dim=768)
    fill_module_(st, prefix="st.")
    torch.nn.init.normal_(st.proj_out.weight, std=0.05)                      # (zero_module: the block would not reach the output)
    sd = {"st." + k: v.detach().float() for k, v in st.state_dict().items()}
    st = st.to(dev)
    blk = st.transformer_blocks[0]
    g = torch.Generator().manual_seed(C)
    x, ctx = torch.randn(2, C, 8, 8, generator=g), torch.randn(2, 1, 768, generator=g)
    with torch.no_grad():
        assert blk.fold_layernorm and not blk._folded(blk.pk(), 64)
        want = O.spatial_transformer(sd, "st.", x, ctx, heads)
        try:
            ops._TIMES = {}
            got = st(x.to(dev), ctx.to(dev))
            torch.cuda.synchronize()
            keys = list(ops._TIMES)
        finally:
            ops._TIMES = None
    assert not any(k.startswith("gx:") and "T" in k.split("|")[-1] for k in keys), keys
    check_rel_l2(f"SpatialTransformer C={C}, {heads} heads x 40 (unfused) vs the oracle", got, want, BLOCK_TOL)


# ---- 3. alpha_cols granularity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [6, 8])
@pytest.mark.parametrize("alpha_cols", [4, 36, 132, 328 - 4])
@pytest.mark.parametrize("fold", [False, True])
def test_alpha_boundary_at_every_granularity(dev, fold, alpha_cols, tile):
    """alpha on columns < alpha_cols only: the boundary inside a wave's first 8 columns, off every 16- / 32- / 64-column unit, and four
    columns before N; alone and with the LayerNorm fold."""
    c = _case("ln_alpha" if fold else "alpha", 328, ln=1 if fold else 0, alpha_cols=alpha_cols)
    with torch.no_grad():
        t, outs, plan = _launch(c, dev, tile | (1 << 8))
        assert (plan[0], max(1, plan[1])) == (tile, 1), plan
        _verify(c, t, outs, plan)


# ---- 4. paired launches off the tuned table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(3, 16, 24), (16, 8, 12)])
def test_paired_transformer_is_bit_identical_off_the_table(dev, B, H, W):
    """SpatialTransformer(640, 8, 80).run_paired on B samples against run on the duplicated 2B batch at N = 384 / 96 tokens (no tuned
    entry): the same bits, and no launch that could not take the 2B plan."""
    from ldm.modules.attention import SpatialTransformer
    from pbe_amd import ops
    from pbe_amd.weights import fill_module_
    st = SpatialTransformer(640, 8, 80, depth=1, context_dim=768)
    fill_module_(st, prefix="st640.")                                        # (name-seeded random weights)
    torch.nn.init.normal_(st.proj_out.weight, std=0.05, generator=torch.Generator().manual_seed(640))
    st = st.to(dev)
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, H, W, 640, generator=g).half().to(dev)
    ctx = torch.randn(2 * B, 1, 768, generator=g).to(dev)
    ops._PIN_CACHE.clear()
    misses = len(ops._PIN_MISSES)
    with torch.no_grad():
        vecs = st.context_vectors(ctx)
        paired = st.run_paired(x, vecs)
        full = st.run(torch.cat([x, x]), vecs)
    assert torch.isfinite(paired).all() and paired.shape == full.shape == (2 * B, H, W, 640)
    assert ops._PIN_MISSES[misses:] == [], ops._PIN_MISSES[misses:]
    assert torch.equal(paired, full), f"B={B} N={H * W}: run_paired differs from run in {int((paired != full).sum())} of {full.numel()} elements"
