"""The edges of the memory a kernel may touch (tests/guard.py), per kernel family, on the GPU.

Every case embeds the operands in arenas whose every element OUTSIDE the entry point's contract is poison (leading-dimension padding,
rows past M, keys past Nk, gaps between batches, the elements before the first and after the last of a contiguous tensor, scale
vectors past M / N) and puts every output into an arena of sentinel bits, then asserts
  (a) the result equals, bit for bit, the same launch on plain contiguous finite operands (same tile and split-K factor: ops._PLANS),
  (b) the op's existing _close bound against a plain fp32 / fp64 torch reference (tilecheck.CLOSE / the limits of test_ops_gpu.py),
  (c) nothing outside an output view was written, every element inside was,
  (d) every output is finite.
Once per family a POSITIVE CONTROL moves one poison value inside the logical extent (last valid key, A[m, K - 1], last channel ...)
and the affected outputs must turn non-finite (or, for the MX quantiser, whose saturating conversion launders NaN, change the
block's scale): the poison is live on that path, so (d) means something.

Poison per family: fp16 / fp32 quiet NaN everywhere except e4m3 operand bytes (0x7F, the e4m3 NaN), and the MX-fp8 quantiser sources
(6e4: fmaxf and the saturating conversion launder NaN there).  Softmax / attention maxima go through fmaxf, which drops a NaN, but
exp2(NaN - m) is NaN again - the controls of those families show it.

An arena makes a stray STORE land in owned memory where assert_untouched finds it.  A stray READ past an allocation cannot be seen
this way and is not hunted here (that would mean provoking faults): a read past the logical extent is caught only where it lands on
poison, i.e. inside the arena.  Every case is one or two ordinary launches.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f8ref
import guard
import mx8ref as R
from tilecheck import CLOSE

pytestmark = pytest.mark.gpu
NAN = float("nan")
U32 = 2.0 ** -24


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, ref, rtol=2e-3, atol=1e-3, what=""):
    """The bound of tests/test_ops_gpu.py::_close."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item()
    lim = rtol * ref.abs().max().item() + atol
    assert err <= lim, f"{what}: max|d|={err:.4e} > {lim:.4e}"


def _same_bits(got, plain, what):
    assert got.shape == plain.shape, (what, got.shape, plain.shape)
    diff = guard.bits(got.contiguous()) != guard.bits(plain.contiguous())
    assert not diff.any(), f"{what}: padding changed {int(diff.sum())} element(s), first at {tuple(torch.nonzero(diff)[0].tolist())}"


def _outputs_ok(pairs, what):
    """pairs: (view, arena) of every output."""
    for i, (view, arena) in enumerate(pairs):
        guard.assert_untouched(arena, view, f"{what} [output {i}]")
        guard.assert_fully_written(view, f"{what} [output {i}]")
        if view.dtype.is_floating_point:
            assert torch.isfinite(view).all(), f"{what} [output {i}]: non-finite"


class _plans:
    """with _plans() as p: ... -> p.got = [(tile, split-K factor, BM, BN, workgroups), ...] of the GEMM / conv launches inside."""

    def __enter__(self):
        from pbe_amd import ops
        ops._PLANS = []
        self.got = None
        return self

    def __exit__(self, *exc):
        from pbe_amd import ops
        self.got, ops._PLANS = [p[1:] for p in ops._PLANS], None
        return False


class _forced:
    """pbe_tune key -> value inside the block, the default restored after."""
    DEFAULT = {1: -1, 3: 0, 6: 1}

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items() if v is not None}

    def __enter__(self):
        from pbe_amd import ops
        for k, v in self.kv.items():
            ops.tune(k, v)

    def __exit__(self, *exc):
        from pbe_amd import ops
        for k in self.kv:
            ops.tune(k, self.DEFAULT[k])
        return False


def _emb(dev, padded):
    """The operand placement of a run: strided inside a poisoned arena (padded), or plain contiguous (poison only before the first and
    after the last element)."""
    def put(t, **kw):
        if t is None:
            return None
        if not padded:
            return guard.embed(t.reshape(-1), device=dev)[0].view(t.shape)
        return guard.embed(t, device=dev, **kw)[0]
    return put


def _out(dev, padded, shape, dtype=torch.float16, **kw):
    """(view, arena) of an output: with leading-dimension / row / batch padding, or plain contiguous (still between sentinels, so that
    the contiguous launch is checked - and safe - too)."""
    if padded:
        return guard.sentinel_out(shape, dtype=dtype, device=dev, **kw)
    flat, arena = guard.sentinel_out((math.prod(shape),), dtype=dtype, device=dev)
    return flat.view(shape), arena


# =====================================================================================================================================
# GEMM (pbe_gemm_f16)
# =====================================================================================================================================
def _gemm_operands(M, N, K, *, K1=0, batch=0, act=0, bias_per_row=False, group_rows=0, resid=False, seed=0):
    g = _g(seed)
    lead = (batch,) if batch else ()
    t = {"a": torch.randn(*lead, M, K1 or K, generator=g).half(),
         "a2": torch.randn(M, K - K1, generator=g).half() if K1 else None,
         "w": (torch.randn(*lead, N, K, generator=g) / math.sqrt(K)).half(),
         "bias": torch.randn(M if bias_per_row else N, generator=g),
         "rowvec": torch.randn((M + group_rows - 1) // group_rows, N, generator=g).half() if group_rows else None,
         "resid": torch.randn(*lead, M, N // 2 if act == 4 else N, generator=g).half() if resid else None}
    t["cfg"] = dict(act=act, bias_per_row=bias_per_row, group_rows=group_rows)
    return t


def _act(v, act):
    return {0: lambda x: x, 1: F.silu, 2: F.gelu, 3: lambda x: x * torch.sigmoid(1.702 * x)}[act](v)


def _gemm_ref(t, alpha=1.0):
    c = t["cfg"]
    a = t["a"] if t["a2"] is None else torch.cat([t["a"], t["a2"]], -1)
    pre = alpha * (a.float() @ t["w"].float().transpose(-1, -2))
    pre = pre + (t["bias"][:, None] if c["bias_per_row"] else t["bias"])
    if t["rowvec"] is not None:
        pre = pre + t["rowvec"].float().repeat_interleave(c["group_rows"], 0)[: pre.shape[-2]]
    y = pre[..., 0::2] * F.gelu(pre[..., 1::2]) if c["act"] == 4 else _act(pre, c["act"])
    y = y.half().float()
    return y if t["resid"] is None else y + t["resid"].float()


def _gemm_run(t, dev, padded, alpha=1.0, poke=None):
    """One launch -> (out view, out arena, plans).  padded: ld padding on every operand, poison rows after the last row of each."""
    from pbe_amd import ops
    c = t["cfg"]
    put = _emb(dev, padded)
    v = {"a": put(t["a"], row_pad=3, col_pad=8), "a2": put(t["a2"], row_pad=1, col_pad=24), "w": put(t["w"], row_pad=2, col_pad=16),
         "bias": put(t["bias"]), "rowvec": put(t["rowvec"], row_pad=1, col_pad=8), "resid": put(t["resid"], row_pad=1, col_pad=16)}
    if poke is not None:
        poke(v)
    M, N = t["a"].shape[-2], t["w"].shape[-2]
    out, arena = _out(dev, padded, tuple(t["a"].shape[:-2]) + (M, N // 2 if c["act"] == 4 else N), row_pad=2, col_pad=8)
    with _plans() as p:
        ops.gemm(v["a"], v["w"], v["bias"], a2=v["a2"], rowvec=v["rowvec"], group_rows=c["group_rows"], resid=v["resid"], act=c["act"],
                 alpha=alpha, bias_per_row=c["bias_per_row"], out=out)
    return out, arena, p.got


def _gemm_check(t, dev, what, *, alpha=1.0, cfg=None, close=CLOSE["gemm"], want_tile=None, want_split=None):
    with _forced(k1=cfg):
        plain, arena0, plan0 = _gemm_run(t, dev, False, alpha)
        got, arena, plan1 = _gemm_run(t, dev, True, alpha)
    assert plan0 == plan1, f"{what}: padding changed the launch plan {plan0} -> {plan1}"
    _outputs_ok([(plain, arena0)], what + " (contiguous)")
    if want_tile is not None:
        assert plan1[0][0] == want_tile, f"{what}: tile {want_tile} did not run: {plan1}"
    if want_split is not None:
        assert plan1[0][1] == want_split, f"{what}: split-K factor {want_split} did not run: {plan1}"
    _outputs_ok([(got, arena)], what)
    _same_bits(got, plain, what)
    _close(got, _gemm_ref(t, alpha), *close, what=what)
    return plan1[0]


DENSE_TILES = list(range(10)) + [15, 16, 17, 18, 21]


@pytest.mark.parametrize("cfg", [None] + DENSE_TILES)
def test_gemm_padding_rows_and_ragged_k(dev, cfg):
    """lda, lda2, ldw, ldr, ldv, ldc > the logical widths all at once, poison rows after A / A2 / W / resid / rowvec, M and N off every tile
    grid, K % 64 != 0 and K1 % 64 != 0, bias + row vector + SiLU + residual; vector store path (N % 8 == 0).  Poison: NaN."""
    t = _gemm_operands(200, 136, 200, K1=96, group_rows=64, resid=True, act=1, seed=3)
    _gemm_check(t, dev, f"gemm 200x136x(96|104) tile {cfg}", alpha=0.5, cfg=None if cfg is None else cfg | (1 << 8), want_tile=cfg)


@pytest.mark.parametrize("K1,K2", [(32, 40), (128, 72), (64, 64), (96, 96)])
@pytest.mark.parametrize("cfg", [None, 1, 3, 6, 9, 17, 21])
def test_gemm_ragged_k_and_straddling_concat_padding(dev, K1, K2, cfg):
    """The k-tiles that leave the lean loader form (K % 64 != 0, K1 % 64 != 0: test_gemm_ragged_k_and_straddling_concat) with lda / lda2 /
    ldw padding: the 16-byte chunks past K1 of A, past K - K1 of A2 and past K of W hold NaN.  Poison: NaN."""
    t = _gemm_operands(200, 136, K1 + K2, K1=K1, seed=K1 * 7 + K2)
    _gemm_check(t, dev, f"gemm K1={K1} K2={K2} tile {cfg}", cfg=None if cfg is None else cfg | (1 << 8), want_tile=cfg)


@pytest.mark.parametrize("M,N,K", [(333, 100, 136), (300, 4, 2880), (64, 4, 72)])
@pytest.mark.parametrize("cfg", [None, 0, 6, 9, 21])
def test_gemm_scalar_store_path(dev, M, N, K, cfg):
    """N % 8 != 0: the scalar copy-out (p.vec false), N = 4 and 100, with a residual and a row vector.  Poison: NaN."""
    t = _gemm_operands(M, N, K, group_rows=48, resid=True, seed=M + N)
    _gemm_check(t, dev, f"gemm {M}x{N}x{K} tile {cfg}", cfg=None if cfg is None else cfg | (1 << 8), want_tile=cfg)


@pytest.mark.parametrize("cfg", [None, 3, 7, 17])
def test_gemm_geglu_and_per_row_bias(dev, cfg):
    """GEGLU (ldc > N / 2, the output half as wide as the accumulator tile) and the per-row bias (poison after bias[M - 1]).  Poison: NaN."""
    force = None if cfg is None else cfg | (1 << 8)
    t = _gemm_operands(333, 272, 136, act=4, seed=11)
    _gemm_check(t, dev, f"gemm GEGLU tile {cfg}", cfg=force, want_tile=cfg)
    t = _gemm_operands(333, 136, 136, bias_per_row=True, seed=12)
    _gemm_check(t, dev, f"gemm per-row bias tile {cfg}", alpha=0.5, cfg=force, want_tile=cfg)


@pytest.mark.parametrize("cfg", [None, 2, 6])
def test_gemm_strided_batch_with_gaps(dev, cfg):
    """Strided batch: strideA / W / C / R leave poisoned (operands) or sentinel (output) gaps between the batches.  Poison: NaN."""
    t = _gemm_operands(130, 264, 72, batch=3, resid=True, seed=6)
    _gemm_check(t, dev, f"gemm batch 3 tile {cfg}", cfg=None if cfg is None else cfg | (1 << 8), want_tile=cfg)


@pytest.mark.parametrize("factor", [2, 3, 5])
@pytest.mark.parametrize("cfg", [3, 9])
def test_gemm_forced_split_k_output_in_arena(dev, cfg, factor):
    """Split-K: the slabs go to the workspace, the reduce kernel stores 4 columns per thread - M, N off the grid (N % 4 == 0, N % 8 != 0),
    ragged K, row vector + residual + SiLU, the output in an arena.  Poison: NaN."""
    t = _gemm_operands(200, 100, 1352, group_rows=64, resid=True, act=1, seed=factor)
    _gemm_check(t, dev, f"gemm split-K {factor} tile {cfg}", cfg=cfg | (factor << 8), want_tile=cfg, want_split=factor)


def test_gemm_positive_control(dev):
    """One NaN moved INSIDE the logical extent must reach the output: A[M - 1, K - 1] -> row M - 1; W[N - 1, K - 1] -> column N - 1; the
    last value of the row vector, the bias and the residual -> their elements (ragged last k-tile, last row / column tile)."""
    M, N, K = 200, 136, 200
    t = _gemm_operands(M, N, K, group_rows=64, resid=True, seed=3)

    def run(poke):
        out, _, _ = _gemm_run(t, dev, True, poke=poke)
        return ~torch.isfinite(out.float().cpu())
    bad = run(lambda v: v["a"].__setitem__((M - 1, K - 1), NAN))
    assert bad[M - 1].all() and not bad[: M - 1].any()
    bad = run(lambda v: v["w"].__setitem__((N - 1, K - 1), NAN))
    assert bad[:, N - 1].all() and not bad[:, : N - 1].any()
    bad = run(lambda v: v["rowvec"].__setitem__((-1, N - 1), NAN))
    assert bad[192:, N - 1].all() and int(bad.sum()) == M - 192
    bad = run(lambda v: v["bias"].__setitem__(N - 1, NAN))
    assert bad[:, N - 1].all() and int(bad.sum()) == M
    bad = run(lambda v: v["resid"].__setitem__((M - 1, N - 1), NAN))
    assert bad[M - 1, N - 1] and int(bad.sum()) == 1


# ---- extended epilogue ---------------------------------------------------------------------------------------------------------------
def _ln_parts(x, parts):
    """fp32 [parts, M, 2] partial (sum, sumsq) of the rows of x over `parts` column ranges (what a producer's row_stats_out leaves)."""
    cols = torch.chunk(x.float(), parts, 1)
    return torch.stack([torch.stack([c.sum(1), (c * c).sum(1)], 1) for c in cols], 0).contiguous()


def _stats(dev, padded, st, M):
    """RowStats over st [parts, M, 2]: contiguous, or with ln_stats_ld > M and poison past row M of every partial."""
    from pbe_amd import ops
    parts = st.shape[0]
    if not padded:
        return ops.RowStats(st.to(dev), parts, M)
    view, _ = guard.embed(st.reshape(parts, 2 * M), col_pad=2 * 24, device=dev)
    return ops.RowStats(view, parts, view.stride(0) // 2)


def _qkv_case(dev, padded, B, T, C, seed, poke=None):
    """The fused q | k | V^T projection with the LayerNorm fold (ln_parts = 2): q | k with ldc > vt_col0, V^T with vt_rs > vt_tokens and
    vt_bs > rows * vt_rs.  -> (qk, vt, arenas, plans, reference [M, 3C])."""
    from pbe_amd import ops
    g = _g(seed)
    M = B * T
    x = (torch.randn(M, C, generator=g) * 1.3 + 0.4).half()
    w, b = torch.randn(3 * C, C, generator=g) / C ** 0.5, 0.1 * torch.randn(3 * C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.linear(F.layer_norm(x.float(), (C,), gamma, torch.zeros(C), 1e-5), w)
    ref[:, :C] *= 0.2281
    ref += w @ beta + b
    wg, c2, c1 = ops.pack_linear_ln(w, b, gamma, beta)
    put = _emb(dev, padded)
    v = {"x": put(x, row_pad=2, col_pad=8), "w": put(wg, row_pad=1, col_pad=8), "bias": put(c2), "colsum": put(c1)}
    if poke is not None:
        poke(v)
    qk, qk_arena = _out(dev, padded, (M, 2 * C), row_pad=1, col_pad=16)
    vt, vt_arena = _out(dev, padded, (B, C, T), row_pad=3, col_pad=8)
    with _plans() as p:
        ops.gemm(v["x"], v["w"], v["bias"], ln=(_stats(dev, padded, _ln_parts(x, 2), M), v["colsum"], 1e-5), alpha=0.2281, alpha_cols=C, out=qk,
                 vt=vt, vt_col0=2 * C, vt_tokens=T)
    return qk, vt, [(qk, qk_arena), (vt, vt_arena)], p.got, ref


@pytest.mark.parametrize("B,T,C,cfg", [(3, 72, 64, None), (3, 72, 64, 6), (2, 40, 128, 3), (4, 64, 320, 20), (4, 64, 320, 9)])
def test_gemm_qkv_vt_epilogue(dev, B, T, C, cfg):
    """V^T columns (vt_rs > vt_tokens, vt_bs > rows * vt_rs: tokens past vt_tokens and rows past C of every sample untouched), q | k with
    ldc > vt_col0, LayerNorm statistics with ln_stats_ld > M and NaN past M in both partials; tokens per sample off the tile height;
    tile 20 is the A-stationary form.  Poison: NaN."""
    what = f"q|k|V^T B{B} T{T} C{C} tile {cfg}"
    with _forced(k1=None if cfg is None else cfg | (1 << 8)):
        qk0, vt0, _, plan0, _ = _qkv_case(dev, False, B, T, C, 5)
        qk, vt, outs, plan1, ref = _qkv_case(dev, True, B, T, C, 5)
    assert plan0 == plan1 and (cfg is None or plan1[0][0] == cfg), (what, plan0, plan1)
    _outputs_ok(outs, what)
    _same_bits(qk, qk0, what + " q|k")
    _same_bits(vt, vt0, what + " V^T")
    _close(qk, ref[:, :2 * C], *CLOSE["ln"], what=what + " q|k")
    _close(vt.transpose(1, 2).reshape(B * T, C), ref[:, 2 * C:], *CLOSE["ln"], what=what + " V^T")


def test_gemm_qkv_positive_control(dev):
    """NaN in the last valid row statistic (partial 1, row M - 1) and in x[M - 1, C - 1]: row M - 1 of q | k and token T - 1 of the last
    sample's V^T turn non-finite, nothing else."""
    B, T, C = 3, 72, 64
    qk, vt, _, _, _ = _qkv_case(dev, True, B, T, C, 5, poke=lambda v: v["x"].__setitem__((B * T - 1, C - 1), NAN))
    bad, badv = ~torch.isfinite(qk.float().cpu()), ~torch.isfinite(vt.float().cpu())
    assert bad[-1].all() and not bad[:-1].any()
    assert badv[B - 1, :, T - 1].all() and int(badv.sum()) == C


@pytest.mark.parametrize("M,N,K,cfg", [(200, 136, 200, None), (200, 320, 136, 8), (333, 136, 72, 17)])
def test_gemm_row_statistics_in_arena(dev, M, N, K, cfg):
    """row_stats_out with row_stats_ld > M and MORE partial planes than the plan's column tiles: rows past M of every written plane and
    the extra planes stay untouched; the written partials are those of the contiguous launch, bit for bit, and sum to the row sums of
    the stored output (the bound of test_gemm_row_statistics_epilogue).  Poison: NaN."""
    from pbe_amd import ops
    t = _gemm_operands(M, N, K, group_rows=64, resid=True, seed=M + K)
    put = _emb(dev, True)
    res = {}
    with _forced(k1=None if cfg is None else cfg | (1 << 8)):
        for padded in (False, True):
            put = _emb(dev, padded)
            out, arena = _out(dev, padded, (M, N), row_pad=2, col_pad=8)
            planes = 8
            sview, sarena = _out(dev, padded, (planes, 2 * M), dtype=torch.float32, col_pad=2 * 20)
            st_in = ops.RowStats(sview, planes, sview.stride(0) // 2)
            with _plans() as p:
                _, st = ops.gemm(put(t["a"], row_pad=3, col_pad=8), put(t["w"], row_pad=2, col_pad=16), put(t["bias"]),
                                 rowvec=put(t["rowvec"], row_pad=1, col_pad=8), group_rows=64, resid=put(t["resid"], row_pad=1, col_pad=16), out=out, row_stats=st_in)
            res[padded] = (out, arena, sview[: st.parts], sarena, p.got, st.parts)
    out, arena, sv, sarena, plan1, parts = res[True]
    what = f"row_stats {M}x{N}x{K} tile {cfg}"
    assert res[False][4] == plan1 and (cfg is None or plan1[0][0] == cfg), (what, res[False][4], plan1)
    assert parts == -(-N // plan1[0][3]) < 8
    _outputs_ok([(out, arena), (sv, sarena)], what)
    _same_bits(out, res[False][0], what)
    _same_bits(sv, res[False][2], what + " partials")
    _close(out, _gemm_ref(t), *CLOSE["gemm"], what=what)
    tot = sv.double().sum(0).view(M, 2).cpu()
    want = torch.stack([out.double().sum(1), (out.double() ** 2).sum(1)], 1).cpu()
    assert torch.allclose(tot, want, rtol=2e-6, atol=1e-4), (tot - want).abs().max()


@pytest.mark.parametrize("cfg", [19, 20, 9])
def test_gemm_a_stationary_geglu_padding(dev, cfg):
    """Tiles 19 / 20 (A block in registers, K = 320, LayerNorm fold + GEGLU) where pbe_astat_ok holds, against the streaming tile 9:
    lda / ldw / ldc padding, ln_stats_ld > M with NaN past M, ln_parts = 2.  Poison: NaN."""
    from pbe_amd import ops
    M, K, N = 256, 320, 640
    g = _g(19)
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.4).half()
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, 0.1 * torch.randn(N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    h = F.linear(F.layer_norm(x.float(), (K,), gamma, beta, 1e-5), w, b)
    ref = h[:, :N // 2] * F.gelu(h[:, N // 2:])
    wi, bi = torch.stack([w[:N // 2], w[N // 2:]], 1).reshape(N, K), torch.stack([b[:N // 2], b[N // 2:]], 1).reshape(N)
    wg, c2, c1 = ops.pack_linear_ln(wi, bi, gamma, beta)
    res = {}
    with _forced(k1=cfg | (1 << 8)):
        for padded in (False, True):
            put = _emb(dev, padded)
            out, arena = _out(dev, padded, (M, N // 2), row_pad=2, col_pad=8)
            with _plans() as p:
                ops.gemm(put(x, row_pad=2, col_pad=8), put(wg, row_pad=1, col_pad=8), put(c2), act=ops.ACT_GEGLU,
                         ln=(_stats(dev, padded, _ln_parts(x, 2), M), put(c1), 1e-5), out=out)
            res[padded] = (out, arena, p.got)
    what = f"A-stationary GEGLU tile {cfg}"
    assert res[False][2] == res[True][2] and res[True][2][0][0] == cfg, (what, res[True][2])
    _outputs_ok([res[True][:2]], what)
    _same_bits(res[True][0], res[False][0], what)
    _close(res[True][0], ref, *CLOSE["ln"], what=what)


# ---- fp8 operands --------------------------------------------------------------------------------------------------------------------
def _deq(w8, scale):
    return w8.view(torch.float8_e4m3fn).float() * scale[:, None]


def _f8_run(dev, padded, a8, sa, w8, sw, bias, res, poke=None):
    from pbe_amd import ops
    put = _emb(dev, padded)
    v = {"a8": put(a8, row_pad=2, col_pad=16), "sa": put(sa), "w8": put(w8, row_pad=1, col_pad=32), "sw": put(sw), "bias": put(bias),
         "res": put(res, row_pad=1, col_pad=8)}
    if poke is not None:
        poke(v)
    out, arena = _out(dev, padded, (a8.shape[0], w8.shape[0]), row_pad=2, col_pad=8)
    with _plans() as p:
        ops.gemm_f8(v["a8"], v["sa"], v["w8"], v["sw"], v["bias"], resid=v["res"], out=out)
    return out, arena, p.got


@pytest.mark.parametrize("cfg", [None, 3, 4, 6, 8, 9])
def test_gemm_f8_padding(dev, cfg):
    """fp8 operands: lda / ldw in BYTES with 0x7F (the e4m3 NaN) in the padding and in the rows after the last, a_scale / w_scale inside
    longer vectors with NaN past M / N, M and N off the tile grid, K % 64 != 0.  Poison: 0x7F bytes, NaN floats."""
    from pbe_amd import ops
    M, N, K = 200, 136, 208
    g = _g(8)
    a8, sa = ops.pack_linear_f8(torch.randn(M, K, generator=g) * torch.rand(M, 1, generator=g) * 3)
    w8, sw = ops.pack_linear_f8(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g).half()
    ref = (_deq(a8, sa) @ _deq(w8, sw).t() + bias).half().float() + res.float()
    what = f"gemm_f8 {M}x{N}x{K} tile {cfg}"
    with _forced(k1=None if cfg is None else cfg | (1 << 8)):
        plain, _, plan0 = _f8_run(dev, False, a8, sa, w8, sw, bias, res)
        got, arena, plan1 = _f8_run(dev, True, a8, sa, w8, sw, bias, res)
        if cfg is None:
            ctl = {k: ~torch.isfinite(_f8_run(dev, True, a8, sa, w8, sw, bias, res, poke=f)[0].float().cpu()) for k, f in (
                ("a", lambda v: v["a8"].__setitem__((M - 1, K - 1), 0x7F)), ("sa", lambda v: v["sa"].__setitem__(M - 1, NAN)),
                ("sw", lambda v: v["sw"].__setitem__(N - 1, NAN)))}
    assert plan0 == plan1 and (cfg is None or plan1[0][0] == cfg), (what, plan0, plan1)
    _outputs_ok([(got, arena)], what)
    _same_bits(got, plain, what)
    _close(got, ref, *CLOSE["f8"], what=what)
    if cfg is None:                                          # positive control: the last operand byte / the last scale of each vector
        assert ctl["a"][M - 1].all() and not ctl["a"][: M - 1].any()
        assert ctl["sa"][M - 1].all() and not ctl["sa"][: M - 1].any()
        assert ctl["sw"][:, N - 1].all() and not ctl["sw"][:, : N - 1].any()


def test_gemm_f8_vt_layout_padding(dev):
    """The V^T projection form (weights as the shared A operand, one W / w_scale per sample): poisoned gaps between the samples' tokens and
    between their scale vectors, V^T rows (tokens) with vt row padding in a sentinel arena.  Poison: 0x7F bytes, NaN floats."""
    from pbe_amd import ops
    B, N, Cc, inner = 3, 200, 208, 136
    g = _g(5)
    x8, sx = ops.pack_linear_f8(torch.randn(B * N, Cc, generator=g))
    w8, sw = ops.pack_linear_f8(torch.randn(inner, Cc, generator=g) / math.sqrt(Cc))
    ref = torch.einsum("ik,bnk->bin", _deq(w8, sw), _deq(x8, sx).view(B, N, Cc))
    res = {}
    for padded in (False, True):
        put = _emb(dev, padded)
        out, arena = _out(dev, padded, (B, inner, N), row_pad=2, col_pad=16)
        with _plans() as p:
            ops.gemm_f8(put(w8, row_pad=1, col_pad=16).unsqueeze(0).expand(B, -1, -1), put(sw), put(x8.view(B, N, Cc), row_pad=3, col_pad=16),
                        put(sx.view(B, N), col_pad=8), out=out)
        res[padded] = (out, arena, p.got)
    assert res[False][2] == res[True][2]
    _outputs_ok([res[True][:2]], "gemm_f8 V^T")
    _same_bits(res[True][0], res[False][0], "gemm_f8 V^T")
    _close(res[True][0], ref, *CLOSE["f8"], what="gemm_f8 V^T")


# ---- split-K workspace -----------------------------------------------------------------------------------------------------------------
class _workspace:
    """ops' split-K scratch replaced by `nbytes` bytes inside a sentinel arena (None: a null workspace)."""

    def __init__(self, dev, nbytes):
        from pbe_amd import ops
        self.ops, self.nbytes = ops, nbytes
        if nbytes is None:
            self.view = self.arena = torch.empty(0, dtype=torch.float32, device=dev)        # data_ptr() == 0
        else:
            self.view, self.arena = guard.sentinel_out((max(nbytes // 4, 1),), dtype=torch.float32, device=dev)

    def __enter__(self):
        self.saved = (self.ops._splitk_ws, self.ops.SPLITK_WS_BYTES)
        self.ops._splitk_ws = lambda device: self.view
        if self.nbytes is not None:
            self.ops.SPLITK_WS_BYTES = self.nbytes
        return self

    def __exit__(self, *exc):
        self.ops._splitk_ws, self.ops.SPLITK_WS_BYTES = self.saved
        return False

    def intact(self, what):
        if self.nbytes is not None:
            guard.assert_untouched(self.arena, self.view[: self.nbytes // 4], what + " [split-K workspace]")


def _gemm_plan_query(M, N, K, ldc, ws_bytes, tile_cfg):
    """pbe_gemm_plan of the descriptor ops.gemm builds for a plain [M, K] x [N, K] launch -> (out6, workspace_needed)."""
    from pbe_amd import lib
    d = lib.GemmDesc()
    d.A = d.W = d.C = 1 << 20
    d.M, d.N, d.K, d.K1, d.lda, d.ldw, d.ldc, d.batch, d.alpha, d.tile_cfg = M, N, K, K, K, K, ldc, 1, 1.0, tile_cfg
    d.workspace, d.workspace_bytes = (1 << 20) if ws_bytes else None, ws_bytes
    out, need = (C.c_int32 * 6)(), C.c_size_t()
    lib.check(lib.load().pbe_gemm_plan(C.byref(d), out, C.byref(need)), "pbe_gemm_plan")
    return list(out), need.value


def test_gemm_split_k_workspace_contract(dev):
    """pbe_gemm_desc.workspace_bytes, 'any size: the split is clamped to what fits': (i) exactly workspace_needed bytes - the bits of the
    64 MiB launch, nothing past the end written; (ii) one byte less, and half - a smaller factor, never an error, workspace_needed <=
    workspace_bytes, result within _close, arena intact; (iii) a null workspace - factor 1."""
    from pbe_amd import ops
    M, N, K, cfg, factor = 200, 100, 1352, 9, 5
    t = _gemm_operands(M, N, K, seed=77)
    force = cfg | (factor << 8)
    with _forced(k1=force):
        big, _, plan = _gemm_run(t, dev, False)
    assert plan[0][:2] == (cfg, factor)
    out6, need = _gemm_plan_query(M, N, K, N, ops.SPLITK_WS_BYTES, force)
    assert out6[1] == factor and need == factor * M * N * 4
    for nbytes, exact in ((need, True), (need - 1, False), (need // 2, False), (None, False)):
        what = f"split-K workspace of {nbytes} bytes"
        with _forced(k1=force), _workspace(dev, nbytes) as ws:
            got, arena, plan = _gemm_run(t, dev, True)
        ws.intact(what)
        _outputs_ok([(got, arena)], what)
        _close(got, _gemm_ref(t), *CLOSE["gemm"], what=what)
        o6, n2 = _gemm_plan_query(M, N, K, got.stride(0), nbytes or 0, force)
        assert plan[0][:2] == (cfg, o6[1]) and n2 <= (nbytes or 0), (what, plan, o6, n2)
        if exact:
            assert plan[0][1] == factor
            _same_bits(got, big, what)
        elif nbytes is None:
            assert plan[0][1] == 1
        else:
            assert 1 <= plan[0][1] < factor


# =====================================================================================================================================
# Conv (pbe_conv3x3_f16, pbe_im2col3x3_f16)
# =====================================================================================================================================
def _ptr(t):
    return None if t is None else t.data_ptr()


def _conv_launch(dev, x, wp, bias, y, *, x2=None, rowvec=None, resid=None, stride=1, pad=1, ups=0, act=0, gstats=None, groups=0):
    """pbe_conv3x3_f16 through the descriptor ops.conv3x3 fills (the caller owns Y) -> blocks per sample of the group statistics."""
    from pbe_amd import lib, ops
    B, H, W, C1 = x.shape
    Cout = wp.shape[1] if ups == 2 else wp.shape[0]
    d = lib.Conv3x3Desc(_ptr(x), _ptr(x2), _ptr(wp), _ptr(y), _ptr(bias), _ptr(rowvec), _ptr(resid), B, H, W, C1, 0 if x2 is None else x2.shape[3], Cout,
                        stride, pad, ups, 0 if rowvec is None else rowvec.stride(0), act, ops._splitk_ws(dev).data_ptr(), ops.SPLITK_WS_BYTES, -1, 64)
    blocks = C.c_int32(-1)
    if gstats is not None:
        d.group_stats_out, d.group_stats_groups, d.group_stats_blocks = gstats.data_ptr(), groups, C.cast(C.pointer(blocks), C.c_void_p)
    ops._launch("conv", d)
    return blocks.value


def _conv_ref(x, w, b, stride, pad, ups, x2=None):
    xx = x if x2 is None else torch.cat([x, x2], -1)
    xx = xx.float().permute(0, 3, 1, 2)
    if ups:
        xx = F.interpolate(xx, scale_factor=2, mode="nearest")
    if pad == 0:
        xx = F.pad(xx, (0, 1, 0, 1))
    return F.conv2d(xx, w.float(), b, stride=stride, padding=1 if pad else 0).permute(0, 2, 3, 1)


def _conv_operands(B, H, W, C1, C2, Co, stride, pad, ups, fused, seed):
    from pbe_amd import ops
    g = _g(seed)
    t = {"x": torch.randn(B, H, W, C1, generator=g).half(), "x2": torch.randn(B, H, W, C2, generator=g).half() if C2 else None}
    w = (torch.randn(Co, C1 + C2, 3, 3, generator=g) / math.sqrt(9 * (C1 + C2))).half()
    t["bias"] = torch.randn(Co, generator=g)
    Ho, Wo = ops.conv_out_hw(H, W, stride, pad, bool(ups))
    t["rowvec"] = torch.randn(B, Co, generator=g).half() if fused else None
    t["resid"] = torch.randn(B, Ho, Wo, Co, generator=g).half() if fused else None
    t["wp"] = ops.pack_conv3x3_up_phases(w.float()) if ups == 2 else ops.pack_conv3x3(w.float(), split=(C1, C2) if C2 else None)
    ref = _conv_ref(t["x"], w, t["bias"], stride, pad, ups, t["x2"])
    if fused:
        ref = (ref + t["rowvec"].float()[:, None, None, :]).half().float() + t["resid"].float()
    t["ref"], t["geom"], t["shape"] = ref, dict(stride=stride, pad=pad, ups=ups), (B, Ho, Wo, Co)
    return t


def _conv_run(t, dev, padded, groups=0, poke=None):
    """-> (y [B, Ho, Wo, Co], y arena, (stats view, stats arena, blocks) or None, plans).  X / X2 / resid are contiguous by contract:
    poison before their first and after their last element; rowvec with ldv > Cout; Y (contiguous) and the statistics in arenas."""
    put = _emb(dev, padded)
    v = {"x": put(t["x"]), "x2": put(t["x2"]), "wp": put(t["wp"]), "bias": put(t["bias"]), "rowvec": put(t["rowvec"], row_pad=1, col_pad=8),
         "resid": put(t["resid"])}
    if poke is not None:
        poke(v)
    B, Ho, Wo, Co = t["shape"]
    yflat, arena = _out(dev, padded, (B * Ho * Wo * Co,))
    y = yflat.view(B, Ho, Wo, Co)
    gbuf = garena = None
    if groups:
        gbuf, garena = _out(dev, padded, (B * ((Ho * Wo) // 64) * groups * 2,), dtype=torch.float32)
    with _plans() as p:
        blocks = _conv_launch(dev, v["x"], v["wp"], v["bias"], y, x2=v["x2"], rowvec=v["rowvec"], resid=v["resid"], gstats=gbuf, groups=groups,
                              **t["geom"])
    return y, arena, (gbuf, garena, blocks), p.got


def _conv_check(t, dev, what, cfg=None, groups=0, close=CLOSE["conv"]):
    with _forced(k1=cfg):
        plain, arena0, gs0, plan0 = _conv_run(t, dev, False, groups)
        got, arena, gs1, plan1 = _conv_run(t, dev, True, groups)
    assert plan0 == plan1, f"{what}: padding changed the launch plan {plan0} -> {plan1}"
    _outputs_ok([(plain.view(-1), arena0)], what + " (contiguous)")
    if cfg is not None:
        assert plan1[0][0] == cfg & 255, f"{what}: tile {cfg & 255} did not run: {plan1}"
    _outputs_ok([(got.view(-1), arena)], what)
    _same_bits(got, plain, what)
    _close(got, t["ref"], *close, what=what)
    return got, gs0, gs1, plan1[0]


CONV_CASES = [  # B, H, W, C1, C2, Cout, stride, pad, upsample, fused row vector + residual
    (3, 9, 7, 192, 0, 200, 1, 1, 0, True),       # B*Ho*Wo = 189 off the tile height, Cout off the tile width
    (2, 10, 6, 64, 64, 136, 1, 1, 0, True),      # two sources
    (1, 12, 20, 64, 0, 100, 1, 1, 0, True),      # Cout % 8 != 0: scalar copy-out
    (2, 16, 16, 64, 0, 72, 2, 1, 0, False),      # stride 2
    (2, 15, 13, 64, 0, 64, 2, 0, 0, False),      # stride 2, pad 0 (the VAE's (0, 1, 0, 1) pad)
    (2, 9, 7, 64, 0, 64, 1, 0, 0, False),        # stride 1, pad 0
    (2, 8, 6, 128, 0, 136, 1, 1, 1, True),       # nearest-2x upsample fused in the gather
    (2, 8, 6, 128, 0, 200, 1, 1, 2, False),      # the phase form
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("cfg", [None, 0, 6, 9])
def test_conv3x3_borders_and_arenas(dev, case, cfg):
    """The gather tiles: taps iy = -1 of sample 0 and iy = H of the last sample must read zeros, not the poison before / after X (and X2,
    and the residual); ldv > Cout; Y in an arena.  Poison: NaN."""
    t = _conv_operands(*case, seed=sum(case))
    _conv_check(t, dev, f"conv {case} tile {cfg}", cfg=None if cfg is None else cfg | (1 << 8))


@pytest.mark.parametrize("B,H,W,C1,C2,Co,cfg", [(16, 8, 8, 128, 0, 320, 10), (16, 8, 8, 192, 64, 160, 11), (16, 8, 8, 128, 0, 320, 12), (2, 16, 16, 64, 0, 160, 11),
                                                (8, 32, 32, 128, 0, 256, 13), (1, 128, 128, 128, 0, 128, 14), (2, 64, 64, 64, 0, 200, 10)])
def test_conv3x3_halo_tiles_borders_and_arenas(dev, B, H, W, C1, C2, Co, cfg):
    """The halo-resident tiles 10 .. 14 (the halo image is staged with rows -1 and H of each image zeroed): the same borders, several images
    per tile (8x8), Cout off the tile width (200).  Poison: NaN."""
    t = _conv_operands(B, H, W, C1, C2, Co, 1, 1, 0, True, seed=H + Co + cfg)
    _conv_check(t, dev, f"halo conv {B}x{H}x{W}x({C1}+{C2})->{Co} tile {cfg}", cfg=cfg | (1 << 8))


def test_conv3x3_positive_control(dev):
    """NaN in the last element of X reaches the outputs of the last sample's last pixels (the taps that cover it) and only those; NaN in the
    first element of X2 reaches the first pixels of sample 0."""
    case = (2, 10, 6, 64, 64, 136, 1, 1, 0, True)
    t = _conv_operands(*case, seed=sum(case))
    y, _, _, _ = _conv_run(t, dev, True, poke=lambda v: v["x"].__setitem__((1, 9, 5, 63), NAN))
    bad = ~torch.isfinite(y.float().cpu())
    assert bad[1, 8:, 4:].all() and int(bad.sum()) == 4 * 136
    y, _, _, _ = _conv_run(t, dev, True, poke=lambda v: v["x2"].__setitem__((0, 0, 0, 0), NAN))
    bad = ~torch.isfinite(y.float().cpu())
    assert bad[0, :2, :2].all() and int(bad.sum()) == 4 * 136


@pytest.mark.parametrize("B,H,C1,Co,cfg", [(2, 16, 64, 128, None), (2, 16, 64, 160, 11), (2, 32, 64, 128, 4), (8, 8, 64, 128, 6)])
def test_conv3x3_group_statistics_in_arena(dev, B, H, C1, Co, cfg):
    """group_stats_out inside an arena sized for the smallest row block: the floats past B * blocks * groups * 2 stay untouched,
    *group_stats_blocks is consistent with what was written (0: nothing written), the partials are those of the contiguous launch bit
    for bit and sum to the group sums of the stored output.  Bound: a sum of n fp32 terms in any order is within n 2^-24 sum|term|.
    Poison: NaN."""
    G = 32
    t = _conv_operands(B, H, H, C1, 0, Co, 1, 1, 0, True, seed=H + Co)
    what = f"conv group statistics {B}x{H}x{H}x{C1}->{Co} tile {cfg}"
    y, gs0, gs1, plan = _conv_check(t, dev, what, cfg=None if cfg is None else cfg | (1 << 8), groups=G)
    (buf, arena, blocks), blocks0 = gs1, gs0[2]
    assert blocks == blocks0 and blocks >= 0
    used = B * blocks * G * 2
    guard.assert_untouched(arena, buf[:used], what + " [statistics]")
    if blocks == 0:
        return
    assert (H * H) % blocks == 0 and blocks <= (H * H) // 64
    guard.assert_fully_written(buf[:used], what + " [statistics]")
    _same_bits(buf[:used], gs0[0][:used], what + " [statistics]")
    st = buf[:used].view(B, blocks, G, 2).double().cpu()
    yg = y.double().cpu().view(B, blocks, (H * H) // blocks, G, Co // G)
    n = (H * H) // blocks * (Co // G)
    for i, pw in ((0, 1), (1, 2)):
        want, mag = (yg ** pw).sum((2, 4)), (yg.abs() ** pw).sum((2, 4))
        assert ((st[..., i] - want).abs() <= n * U32 * mag + 1e-30).all(), (what, i, (st[..., i] - want).abs().max())


@pytest.mark.parametrize("cfg", [9, 10, 11])
def test_conv3x3_split_k_workspace_contract(dev, cfg):
    """The split-K workspace contract of pbe_conv3x3_desc (gather tile and halo tiles, the 8x8x1280 shape): exactly workspace_needed bytes,
    one byte less, half, null - as test_gemm_split_k_workspace_contract."""
    from pbe_amd import lib, ops
    case, factor = (8, 8, 8, 1280, 0, 320, 1, 1, 0, False), 3
    t = _conv_operands(*case, seed=4242)
    force = cfg | (factor << 8)
    M, N = 8 * 8 * 8, 320

    def planned(nbytes):
        d = lib.Conv3x3Desc(1 << 20, None, 1 << 20, 1 << 20, 1 << 20, None, None, 8, 8, 8, 1280, 0, 320, 1, 1, 0, 0, 0, (1 << 20) if nbytes else None, nbytes or 0, force, 64)
        out, need = (C.c_int32 * 6)(), C.c_size_t()
        lib.check(lib.load().pbe_conv3x3_plan(C.byref(d), out, C.byref(need)), "pbe_conv3x3_plan")
        return list(out), need.value
    with _forced(k1=force):
        big, _, _, plan = _conv_run(t, dev, False)
    o6, need = planned(ops.SPLITK_WS_BYTES)
    assert plan[0][:2] == (cfg, o6[1]) and o6[1] >= 2 and need == o6[1] * M * N * 4, (plan, o6, need)
    for nbytes, exact in ((need, True), (need - 1, False), (need // 2, False), (None, False)):
        what = f"conv tile {cfg} split-K workspace of {nbytes} bytes"
        with _forced(k1=force), _workspace(dev, nbytes) as ws:
            got, arena, _, plan = _conv_run(t, dev, True)
        ws.intact(what)
        _outputs_ok([(got.view(-1), arena)], what)
        _close(got, t["ref"], *CLOSE["conv"], what=what)
        p6, n2 = planned(nbytes)
        assert plan[0][:2] == (cfg, p6[1]) and n2 <= (nbytes or 0), (what, plan, p6, n2)
        if exact:
            assert plan[0][1] == o6[1]
            _same_bits(got, big, what)
        elif nbytes is None:
            assert plan[0][1] == 1
        else:
            assert 1 <= plan[0][1] < o6[1]


@pytest.mark.parametrize("B,H,W,Cp,stride,pad", [(2, 9, 7, 8, 1, 1), (2, 9, 7, 16, 2, 1), (2, 10, 8, 8, 2, 0), (1, 5, 5, 8, 1, 0), (3, 1, 1, 16, 1, 1)])
def test_im2col_borders_and_arena(dev, B, H, W, Cp, stride, pad):
    """pbe_im2col3x3_f16: X between poison, the output in an arena; a pure copy, so the result is EXACTLY the unfolded input with zeros
    outside the image (pad 1) / in the (0, 1, 0, 1) pad (pad 0).  Poison: NaN."""
    from pbe_amd import lib, ops
    x = torch.randn(B, H, W, Cp, generator=_g(H * W + Cp)).half()
    Ho, Wo = ops.conv_out_hw(H, W, stride, pad, False)
    xp = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1) if pad else (0, 1, 0, 1))
    cols = F.unfold(xp, 3, stride=stride).view(B, Cp, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * Cp)       # k = tap * Cp + ci
    xv, _ = guard.embed(x, device=dev)
    out, arena = guard.sentinel_out((B * Ho * Wo, 9 * Cp), device=dev)
    lib.check(lib.load().pbe_im2col3x3_f16(xv.data_ptr(), out.data_ptr(), B, H, W, Cp, stride, pad, torch.cuda.current_stream().cuda_stream), "im2col")
    _outputs_ok([(out, arena)], "im2col")
    assert torch.equal(out.float().cpu(), cols)
    xv[0, 0, 0, 0] = NAN                                     # positive control: the first element (tap (pad, pad) of output pixel 0 reads it)
    lib.check(lib.load().pbe_im2col3x3_f16(xv.data_ptr(), out.data_ptr(), B, H, W, Cp, stride, pad, torch.cuda.current_stream().cuda_stream), "im2col")
    bad = ~torch.isfinite(out.float().cpu())
    assert bad[0, (pad * 3 + pad) * Cp] and 1 <= int(bad.sum()) <= 9


# =====================================================================================================================================
# Attention (pbe_attention_f16)
# =====================================================================================================================================
def _attn_operands(B, H, Nq, Nk, D, seed):
    g = _g(seed)
    t = {"q": torch.randn(B, Nq, H * D, generator=g).half(), "k": torch.randn(B, Nk, H * D, generator=g).half(),
         "v": torch.randn(B, Nk, H * D, generator=g).half()}
    q4, k4, v4 = (t[n].float().view(B, -1, H, D).transpose(1, 2) for n in ("q", "k", "v"))
    t["ref"] = (torch.softmax(q4 @ k4.transpose(-1, -2) * D ** -0.5, -1) @ v4).transpose(1, 2).reshape(B, Nq, H * D)
    t["dims"] = (B, H, Nq, Nk, D)
    return t


def _attn_run(t, dev, padded, poke=None):
    """padded: q_rs, k_rs > H * D with poison in the gap (d = 40 .. 47 of the last head lies there), poison rows past Nq / Nk, V^T rows
    of vt_rs > roundup8(Nk) elements with poison from column Nk on, O with o_rs > H * D and sentinel rows between the samples."""
    from pbe_amd import ops
    B, H, Nq, Nk, D = t["dims"]
    vt = t["v"].transpose(1, 2).contiguous()                                     # [B, H * D, Nk]
    if padded:
        q, k = (guard.embed(t[n], row_pad=2, col_pad=8, device=dev)[0] for n in ("q", "k"))
        vtv = guard.embed(vt, row_pad=1, col_pad=16, device=dev)[0]
    else:                                                                        # as the existing tests lay them out: V^T zero-padded to 8
        q, k = (guard.embed(t[n].reshape(-1), device=dev)[0].view(t[n].shape) for n in ("q", "k"))
        vz = torch.zeros(B, H * D, (Nk + 7) // 8 * 8, dtype=torch.float16)
        vz[:, :, :Nk] = vt
        vtv = guard.embed(vz.reshape(-1), device=dev)[0].view(vz.shape)
    if poke is not None:
        poke(q, k, vtv)
    out, arena = _out(dev, padded, (B, Nq, H * D), row_pad=1, col_pad=8)
    assert not padded or vtv.stride(1) > (Nk + 7) // 8 * 8
    ops.attention(q, k, vtv, B, H, Nq, Nk, D, D ** -0.5, q_strides=(q.stride(0), q.stride(1)), k_strides=(k.stride(0), k.stride(1)),
                  vt_strides=(vtv.stride(0), vtv.stride(1)), out=out)
    return out, arena


def _attn_check(dev, B, H, Nq, Nk, D, what, **force):
    t = _attn_operands(B, H, Nq, Nk, D, Nq * 3 + Nk + D)
    with _forced(**force):
        plain, arena0 = _attn_run(t, dev, False)
        got, arena = _attn_run(t, dev, True)
    _outputs_ok([(plain, arena0), (got, arena)], what)
    _same_bits(got, plain, what)
    _close(got, t["ref"], rtol=4e-3, atol=2e-3, what=what)                       # the bound of test_attention


NKS = [1, 7, 63, 64, 65, 100, 129, 200, 257, 330]           # the ragged last tile in every slot of the ring, KH = 1 and 2
NQS = [1, 31, 130, 257]


@pytest.mark.parametrize("qw,mpad", [(1, 1), (2, 1), (1, 0), (2, 0), (3, 0)])
@pytest.mark.parametrize("i", range(len(NKS)))
def test_attention_d40_ragged_keys(dev, i, qw, mpad):
    """d = 40 in the 48-wide tile, both forms (pbe_tune key 6), queries-per-wave forced 1, 2 and 3 (3 with key 6 = 0: the <48, 2, 2> variant,
    two key tiles per barrier): Nk over every slot of the tile ring, Nq != Nk.  fix_tail must zero what the ragged V^T chunk brought in:
    the V^T rows hold NaN from column Nk on.  Poison: NaN."""
    Nk, Nq = NKS[i], NQS[i % 4]
    _attn_check(dev, 2, 3, Nq, Nk, 40, f"attention d40 Nq{Nq} Nk{Nk} qw{qw} mpad{mpad}", k3=qw, k6=mpad)


@pytest.mark.parametrize("D,qw", [(D, qw) for D in (8, 16, 32, 48, 64, 80, 128, 160) for qw in (1, 2)] + [(48, 3)])
@pytest.mark.parametrize("i", range(len(NKS)))
def test_attention_head_dims_ragged_keys(dev, D, qw, i):
    """Every head-dim instantiation, queries-per-wave forced 1 and 2 (3 at D = 48: the <48, 2, 2> variant), the same key counts.  Poison: NaN."""
    Nk, Nq = NKS[i], NQS[(i + 1) % 4]
    _attn_check(dev, 2, 2, Nq, Nk, D, f"attention D{D} Nq{Nq} Nk{Nk} qw{qw}", k3=qw)


def test_attention_heuristic_two_tiles_per_barrier(dev):
    """The <48, 2, 2, MPAD> variant through the heuristic (ceil(Nq / 256) * B * H >= 512, d = 40) with a ragged Nk.  Poison: NaN."""
    _attn_check(dev, 8, 8, 2048, 2000, 40, "attention d40 B*H 64 Nq 2048 Nk 2000")


@pytest.mark.parametrize("D,qw,mpad", [(40, 1, 1), (40, 2, 1), (40, 3, 0), (64, 2, 1), (160, 1, 1)])
def test_attention_positive_control(dev, D, qw, mpad):
    """NaN moved to the last VALID key: V^T[b, c, Nk - 1] -> channel c of every query of sample b; K[b, Nk - 1, last channel] -> the last head
    of every query of sample b (exp2(NaN - m) is NaN although fmaxf drops it from the maximum)."""
    B, H, Nq, Nk = 2, 3, 130, 200
    t = _attn_operands(B, H, Nq, Nk, D, 9)
    with _forced(k3=qw, k6=mpad):
        out, _ = _attn_run(t, dev, True, poke=lambda q, k, vt: vt.__setitem__((1, 5, Nk - 1), NAN))
        bad = ~torch.isfinite(out.float().cpu())
        assert bad[1, :, 5].all() and int(bad.sum()) == Nq
        out, _ = _attn_run(t, dev, True, poke=lambda q, k, vt: k.__setitem__((0, Nk - 1, H * D - 1), NAN))
        bad = ~torch.isfinite(out.float().cpu())
        assert bad[0, :, (H - 1) * D:].all() and int(bad.sum()) == Nq * D


# =====================================================================================================================================
# MX-fp8 (pbe_quant_mx8_f16, pbe_attention_mx8)
# =====================================================================================================================================
def _quant_raw(dev, x, mode, B, H, N, D, alpha=1.0):
    """pbe_quant_mx8_f16 with Y and S in arenas -> ((Y, arena), (S, arena)) as flat byte tensors."""
    from pbe_amd import lib
    NP = (N + 63) // 64 * 64
    if mode == 1:
        ny, ns = B * H * D * NP, B * H * (NP // 32) * (D // 32 + 1) * 32
    else:
        DP = (D + 63) // 64 * 64
        ny, ns = B * N * H * DP, B * H * (DP // 32) * NP
    Y, S = guard.sentinel_out((ny,), dtype=torch.uint8, device=dev), guard.sentinel_out((ns,), dtype=torch.uint8, device=dev)
    lib.check(lib.load().pbe_quant_mx8_f16(x.data_ptr(), Y[0].data_ptr(), S[0].data_ptr(), mode, B, H, N, D, x.stride(-2), alpha,
                                           torch.cuda.current_stream().cuda_stream), "pbe_quant_mx8_f16")
    return Y, S


@pytest.mark.parametrize("D", [40, 80, 160])
def test_quant_mx8_padding(dev, D):
    """The quantiser's sources with row padding: tokens with rs > H * D, V^T rows with rs > roundup8(N) and N % 32 != 0 (a partial last
    block).  Bytes and scales equal tests/mx8ref.py on the unpadded data, Y / S arenas intact and fully written.  Poison: 6e4 - the block
    maximum goes through fmaxf and the conversion saturates, both launder NaN; a 6e4 that reaches a block changes its scale.
    Positive control: 6e4 moved to the last valid element changes the last block's scale byte."""
    B, H, N = 2, 2, 330
    g = _g(D)
    xt = (torch.randn(B * N, H * D, generator=g) * 3).half()
    xv = (torch.randn(B * H * D, N, generator=g) * 3).half()
    for mode, x, ref in ((0, xt, R.quant_tokens(xt.numpy(), B, H, N, D)), (1, xv, R.quant_vt(xv.numpy(), B, H, N, D))):
        what = f"quant_mx8 mode {mode} D{D}"
        src, _ = guard.embed(x, row_pad=1, col_pad=16, poison=6e4, device=dev)
        assert src.stride(0) > (x.shape[1] + 7) // 8 * 8
        Y, S = _quant_raw(dev, src, mode, B, H, N, D)
        guard.assert_untouched(Y[1], Y[0], what + " [bytes]")             # (0xA5 is a valid e4m3 byte: equality with the reference below shows
        _outputs_ok([S], what + " [scales]")                              #  that every data byte was written)
        assert np.array_equal(S[0].cpu().numpy(), ref[1].reshape(-1)), f"{what}: scale bytes differ from the reference of the unpadded data"
        assert np.array_equal(Y[0].cpu().numpy(), ref[0].reshape(-1)), f"{what}: data bytes differ from the reference of the unpadded data"
        src[-1, -1] = 6e4
        _, S2 = _quant_raw(dev, src, mode, B, H, N, D)
        assert int((S2[0] != S[0]).sum()) == 1, f"{what}: the control value did not move exactly one scale"


@pytest.mark.parametrize("D,Nq,Nk", [(40, 130, 330), (80, 257, 100), (160, 31, 200)])
def test_attention_mx8_output_arena(dev, D, Nq, Nk):
    """pbe_attention_mx8 with Nq, Nk not multiples of 64 and O (o_rs > H * D, sentinel rows between samples) in an arena: bit-equal to the
    contiguous output, within the bound of test_attention_mx8_gpu.py.  (Its operands have no padding the contract leaves undefined.)"""
    from pbe_amd import ops
    import test_attention_mx8_gpu as T
    B, H = 2, 2
    g = _g(D + Nq)
    q, k = torch.randn(B * Nq, H * D, generator=g).half().to(dev), torch.randn(B * Nk, H * D, generator=g).half().to(dev)
    npad = (Nk + 7) // 8 * 8
    vt = torch.zeros(B * H * D, npad, dtype=torch.float16)
    vt[:, :Nk] = torch.randn(B * H * D, Nk, generator=g).half()
    q8 = ops.quant_mx8(q, B, H, Nq, D, rs=H * D, alpha=D ** -0.5 * T.LOG2E)
    k8 = ops.quant_mx8(k, B, H, Nk, D, rs=H * D)
    v8 = ops.quant_mx8(vt.to(dev), B, H, Nk, D, rs=npad, vt=True)
    plain = ops.attention_mx8(q8, k8, v8, 1.0)
    out, arena = guard.sentinel_out((B, Nq, H * D), row_pad=1, col_pad=8, device=dev)
    ops.attention_mx8(q8, k8, v8, 1.0, out=out)
    what = f"attention_mx8 D{D} Nq{Nq} Nk{Nk}"
    _outputs_ok([(out, arena)], what)
    _same_bits(out, plain, what)
    ref, bound = T._reference(T._M8(q8, False), T._M8(k8, False), T._M8(v8, True), 1.0)
    T._check(out, ref, bound, what)


def _mx_targets(dev, B, H, N, D):
    """(q, k, vt) targets of pbe_gemm_mx8out_f16, each data / scale tensor a contiguous view between sentinels -> (targets, arenas)."""
    from pbe_amd import ops
    outs, pairs = [], []
    for mode in (ops.MX8_TOKENS, ops.MX8_TOKENS, ops.MX8_VT):
        ref = ops._mx8_target(mode, B, H, N, D, "meta")
        d, da = guard.sentinel_out((ref.data.numel(),), dtype=torch.uint8, device=dev)
        sc, sa = guard.sentinel_out((ref.scale.numel(),), dtype=torch.uint8, device=dev)
        outs.append(ops.Mx8(d.view(ref.data.shape), sc.view(ref.scale.shape), mode, B, H, N, D))
        pairs += [(d, da), (sc, sa)]
    return tuple(outs), pairs


@pytest.mark.parametrize("C,N,B", [(320, 64, 3), (640, 128, 1), (1280, 64, 2)])
def test_gemm_mx8out_targets_in_arenas(dev, C, N, B):
    """pbe_gemm_mx8out_f16, the LayerNorm-folded q | k | V^T form and the fp8-operand form: data and scale of all three ranges between
    sentinels, the operands with lda / ldw padding, rows after the last and statistics past M poisoned.  Every byte equals the launch on
    contiguous operands into plain targets.  Poison: NaN (fp16 / fp32), 0x7F (operand bytes)."""
    from pbe_amd import ops
    H, D = 8, C // 8
    g = _g(C + N)
    x = (torch.randn(B * N, C, generator=g) * 2 + 0.5).half()
    W = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w, c2, c1 = ops.pack_linear_ln(W, None, gamma, beta)
    qscale = D ** -0.5 * 1.4426950408889634
    res = {}
    for padded in (False, True):
        put = _emb(dev, padded)
        tg, pairs = _mx_targets(dev, B, H, N, D)
        with _plans() as p:
            ops.qkv_mx8(put(x, row_pad=2, col_pad=8), put(w, row_pad=1, col_pad=8), put(c2), ln=(_stats(dev, padded, _ln_parts(x, 2), B * N), put(c1), 1e-5),
                        B=B, H=H, N=N, D=D, alpha=qscale, alpha_cols=C, out=tg)
        for view, arena in pairs:
            guard.assert_untouched(arena, view, f"mx8out C{C} N{N} B{B}")
        res[padded] = (tg, p.got)
    assert res[False][1] == res[True][1]
    for a, b, what in zip(res[False][0], res[True][0], ("q", "k", "vt")):
        _same_bits(b.data, a.data, f"mx8out {what} data")
        _same_bits(b.scale, a.scale, f"mx8out {what} scale")
    xd = x.to(dev)
    free = ops.qkv_mx8(xd, w.to(dev), c2.to(dev), ln=(ops.RowStats(_ln_parts(x, 2).to(dev), 2, B * N), c1.to(dev), 1e-5), B=B, H=H, N=N, D=D, alpha=qscale, alpha_cols=C)
    for a, b, what in zip(free, res[True][0], ("q", "k", "vt")):
        _same_bits(b.data, a.data, f"mx8out {what} data vs plain targets")
        _same_bits(b.scale, a.scale, f"mx8out {what} scale vs plain targets")
    # the fp8-operand form: q | k from token rows, V^T from the swapped (channel-row) launch
    x8, sx = ops.pack_linear_f8(torch.randn(B * N, C, generator=g))
    wqk8, sqk = ops.pack_linear_f8(W[: 2 * C])
    wv8, sv = ops.pack_linear_f8(W[2 * C:])
    res = {}
    for padded in (False, True):
        put = _emb(dev, padded)
        tg, pairs = _mx_targets(dev, B, H, N, D)
        ops.qkv_mx8_f8(put(x8, row_pad=2, col_pad=16), put(sx), put(wqk8, row_pad=1, col_pad=32), put(sqk), put(wv8, row_pad=1, col_pad=16), put(sv),
                       B=B, H=H, N=N, D=D, q_alpha=qscale, out=tg)
        for view, arena in pairs:
            guard.assert_untouched(arena, view, f"mx8out fp8 C{C} N{N} B{B}")
        res[padded] = tg
    for a, b, what in zip(res[False], res[True], ("q", "k", "vt")):
        _same_bits(b.data, a.data, f"mx8out fp8 {what} data")
        _same_bits(b.scale, a.scale, f"mx8out fp8 {what} scale")


# =====================================================================================================================================
# Norms / softmax
# =====================================================================================================================================
def _stream():
    return torch.cuda.current_stream().cuda_stream


ROWS_C = [(r, c) for r in (1, 5, 257) for c in (8, 64, 320, 2048)]


@pytest.mark.parametrize("rows,Cc", ROWS_C)
def test_layernorm_row_stats_softmax_padding(dev, rows, Cc):
    """pbe_layernorm_f16, pbe_row_stats_f16, pbe_softmax_rows_f16: ldx > C with NaN in the gap and in the row after the last, ldy > C in an
    arena.  Bit-equal to the contiguous launch; the bounds of test_layernorm / test_gemm_row_statistics_epilogue / test_softmax_rows_and_geglu.
    Positive control: NaN at x[rows - 1, C - 1] makes the last row of each output non-finite, no other.  Poison: NaN."""
    from pbe_amd import lib, ops
    L = lib.load()
    g = _g(rows + Cc)
    x = (torch.randn(rows, Cc, generator=g) * 1.5 + 0.3).half()
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    xv, _ = guard.embed(x, row_pad=1, col_pad=8, device=dev)
    gv, bv = guard.embed(gamma, device=dev)[0], guard.embed(beta, device=dev)[0]
    for control in (False, True):
        if control:
            xv[rows - 1, Cc - 1] = NAN
        y = guard.sentinel_out((rows, Cc), row_pad=1, col_pad=8, device=dev)
        st = guard.sentinel_out((rows * 2,), dtype=torch.float32, device=dev)
        sm = guard.sentinel_out((rows, Cc), row_pad=1, col_pad=16, device=dev)
        lib.check(L.pbe_layernorm_f16(xv.data_ptr(), gv.data_ptr(), bv.data_ptr(), y[0].data_ptr(), rows, Cc, xv.stride(0), y[0].stride(0), 1e-5, _stream()), "layernorm")
        lib.check(L.pbe_row_stats_f16(xv.data_ptr(), st[0].data_ptr(), rows, Cc, xv.stride(0), _stream()), "row_stats")
        lib.check(L.pbe_softmax_rows_f16(xv.data_ptr(), sm[0].data_ptr(), rows, Cc, xv.stride(0), sm[0].stride(0), 0.37, _stream()), "softmax_rows")
        for view, arena in (y, st, sm):
            guard.assert_untouched(arena, view, f"norms {rows}x{Cc}")
            guard.assert_fully_written(view, f"norms {rows}x{Cc}")
        if control:
            for view in (y[0], st[0].view(rows, 2), sm[0]):
                bad = ~torch.isfinite(view.float().cpu())
                assert bad[rows - 1].all() and not bad[: rows - 1].any()
            continue
        xd = x.to(dev)
        _same_bits(y[0], ops.layernorm(xd, gamma.to(dev), beta.to(dev), 1e-5), "layernorm")
        _same_bits(st[0].view(1, rows, 2), ops.row_stats(xd).buf, "row_stats")
        _same_bits(sm[0], ops.softmax_rows(xd, 0.37), "softmax_rows")
        _close(y[0], F.layer_norm(x.float(), (Cc,), gamma, beta, 1e-5), rtol=3e-3, what=f"layernorm {rows}x{Cc}")
        want = torch.stack([x.double().sum(1), (x.double() ** 2).sum(1)], 1)
        assert torch.allclose(st[0].view(rows, 2).double().cpu(), want, rtol=2e-6, atol=1e-4)
        _close(sm[0], torch.softmax(x.float() * 0.37, -1), rtol=3e-3, atol=1e-6, what=f"softmax_rows {rows}x{Cc}")


@pytest.mark.parametrize("rows,Cc", [(r, c) for r in (1, 5, 257) for c in (16, 64, 320, 2048)])
def test_layernorm_f8_padding(dev, rows, Cc):
    """pbe_layernorm_f8: ldx > C, Y with ldy (bytes) > C and row_scale in arenas.  Bit-equal to the contiguous launch; the bound of
    test_layernorm_f8.  Poison: 6e4 - the row maximum goes through fmaxf and the e4m3 conversion saturates, so a NaN row leaves finite
    bytes and a finite scale (measured: the NaN control did not fire); a 6e4 that reaches a row moves its mean by >= 29 and its scale with
    it.  Positive control: 6e4 at x[rows - 1, C - 1] changes row_scale[rows - 1] and the row's bytes, no other row."""
    from pbe_amd import lib, ops
    g = _g(rows * 3 + Cc)
    x = (torch.randn(rows, Cc, generator=g) * 2 + 0.3).half()
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    xv, _ = guard.embed(x, row_pad=1, col_pad=8, poison=6e4, device=dev)
    gv, bv = guard.embed(gamma, device=dev)[0], guard.embed(beta, device=dev)[0]
    y = guard.sentinel_out((rows, Cc), row_pad=1, col_pad=16, dtype=torch.uint8, device=dev)
    sc = guard.sentinel_out((rows,), dtype=torch.float32, device=dev)

    def run():
        lib.check(lib.load().pbe_layernorm_f8(xv.data_ptr(), gv.data_ptr(), bv.data_ptr(), y[0].data_ptr(), sc[0].data_ptr(), rows, Cc, xv.stride(0),
                                              y[0].stride(0), 1e-5, _stream()), "layernorm_f8")
    run()
    guard.assert_untouched(y[1], y[0], "layernorm_f8 Y")
    _outputs_ok([sc], "layernorm_f8 row_scale")
    y8, s8 = ops.layernorm_f8(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5)
    _same_bits(y[0], y8, "layernorm_f8 Y")
    _same_bits(sc[0], s8, "layernorm_f8 row_scale")
    ref = F.layer_norm(x.float(), (Cc,), gamma, beta, 1e-5)
    scc = sc[0].cpu()
    deq = y[0].cpu().contiguous().view(torch.float8_e4m3fn).float() * scc[:, None]
    assert torch.allclose(scc, ref.abs().amax(1) / 448.0, rtol=2e-3)
    assert ((deq - ref).abs() <= ref.abs() * 2 ** -4 + scc[:, None] * 2 ** -9 + 2e-3).all()
    f8ref.ln8_gate(y[0], scc, x, gamma, beta, 1e-5, f"test_layernorm_f8_padding {rows}x{Cc}")
    xv[rows - 1, Cc - 1] = 6e4
    run()
    moved, moved_y = sc[0].cpu() != scc, (y[0].cpu() != y8.cpu()).any(1)
    assert moved[rows - 1] and moved_y[rows - 1] and not moved[: rows - 1].any() and not moved_y[: rows - 1].any()
    assert torch.isfinite(sc[0]).all()
    guard.assert_untouched(y[1], y[0], "layernorm_f8 Y (control)")


def _gn_ref(x, G, gamma, beta, eps, silu):
    ref = F.group_norm(x.float().transpose(1, 2), G, gamma, beta, eps).transpose(1, 2)
    return F.silu(ref) if silu else ref


def _gn_raw(dev, xv, x2v, gv, bv, B, HW, C1, C2, G, eps, silu):
    """pbe_groupnorm_f16 with a workspace of EXACTLY pbe_groupnorm_workspace_bytes inside an arena and Y in an arena."""
    from pbe_amd import lib
    L = lib.load()
    need = L.pbe_groupnorm_workspace_bytes(B, HW)
    ws = guard.sentinel_out((need,), dtype=torch.uint8, device=dev)
    y = guard.sentinel_out((B * HW * (C1 + C2),), device=dev)
    lib.check(L.pbe_groupnorm_f16(xv.data_ptr(), _ptr(x2v), gv.data_ptr(), bv.data_ptr(), y[0].data_ptr(), B, HW, C1, C2, G, eps, 1 if silu else 0,
                                  ws[0].data_ptr(), need, _stream()), "pbe_groupnorm_f16")
    guard.assert_untouched(ws[1], ws[0], "groupnorm workspace")
    return y


@pytest.mark.parametrize("HW", [1, 63, 64, 1000, 4097])
@pytest.mark.parametrize("C1,C2", [(64, 0), (256, 0), (1280, 0), (64, 192)])
def test_groupnorm_workspace_and_arenas(dev, HW, C1, C2):
    """pbe_groupnorm_f16: X (and X2) between NaN, the workspace exactly as large as pbe_groupnorm_workspace_bytes says inside an arena, Y in
    an arena; the two-pass kernels (8 channels per group do not fit, or the map is large) and the single-launch small-map path (C = 256:
    HW <= 3072, C = 1280: HW <= 612), one and two sources.  Bit-equal to ops.groupnorm, the bound of test_groupnorm.  Positive control: NaN
    in the last element of the last source makes exactly the last group of the last sample non-finite.  Poison: NaN."""
    from pbe_amd import ops
    B, G, Cc = 2, 32, C1 + C2
    g = _g(HW + Cc)
    x = (torch.randn(B, HW, Cc, generator=g) * 2 + 0.5).half()
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    x1, x2 = x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None)
    xv = guard.embed(x1, device=dev)[0]
    x2v = guard.embed(x2, device=dev)[0] if C2 else None
    gv, bv = guard.embed(gamma, device=dev)[0], guard.embed(beta, device=dev)[0]
    what = f"groupnorm HW{HW} C{C1}+{C2}"
    y = _gn_raw(dev, xv, x2v, gv, bv, B, HW, C1, C2, G, 1e-5, True)
    _outputs_ok([y], what)
    plain = ops.groupnorm(x1.to(dev), gamma.to(dev), beta.to(dev), 1e-5, True, x2=None if x2 is None else x2.to(dev))
    _same_bits(y[0].view(B, HW, Cc), plain, what)
    _close(y[0].view(B, HW, Cc), _gn_ref(x, G, gamma, beta, 1e-5, True), rtol=3e-3, what=what)
    (x2v if C2 else xv)[B - 1, HW - 1, -1] = NAN
    y = _gn_raw(dev, xv, x2v, gv, bv, B, HW, C1, C2, G, 1e-5, True)
    bad = ~torch.isfinite(y[0].view(B, HW, Cc).float().cpu())
    cg = Cc // G
    assert bad[B - 1, :, Cc - cg:].all() and int(bad.sum()) == HW * cg
    guard.assert_untouched(y[1], y[0], what + " (control)")


@pytest.mark.parametrize("HW,Cc,blocks", [(256, 128, 4), (1000, 64, 5), (4097, 320, 1)])
def test_groupnorm_apply_partials_in_poisoned_buffer(dev, HW, Cc, blocks):
    """pbe_groupnorm_apply_f16: `blocks` partials per (sample, group) at the head of a larger buffer whose rest is NaN (a conv's
    group_stats_out sized for the smallest row block), Y in an arena.  Positive control: NaN in the last partial.  Poison: NaN."""
    from pbe_amd import lib
    B, G = 2, 32
    g = _g(HW + Cc)
    x = (torch.randn(B, HW, Cc, generator=g) * 2 + 0.5).half()
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    parts = torch.zeros(B, blocks, G, 2)
    for i, rows in enumerate(torch.chunk(torch.arange(HW), blocks)):
        xb = x[:, rows].float().view(B, len(rows), G, Cc // G)
        parts[:, i, :, 0], parts[:, i, :, 1] = xb.sum((1, 3)), (xb * xb).sum((1, 3))
    pv = guard.embed(parts.view(-1), tail=B * 16 * G * 2, device=dev)[0]
    xv = guard.embed(x, device=dev)[0]
    gv, bv = guard.embed(gamma, device=dev)[0], guard.embed(beta, device=dev)[0]
    what = f"groupnorm_apply HW{HW} C{Cc} blocks {blocks}"
    for control in (False, True):
        if control:
            pv[-1] = NAN
        y = guard.sentinel_out((B * HW * Cc,), device=dev)
        lib.check(lib.load().pbe_groupnorm_apply_f16(xv.data_ptr(), pv.data_ptr(), blocks, gv.data_ptr(), bv.data_ptr(), y[0].data_ptr(), B, HW, Cc, G, 1e-5, 0,
                                                     _stream()), "pbe_groupnorm_apply_f16")
        guard.assert_untouched(y[1], y[0], what)
        guard.assert_fully_written(y[0], what)
        got = y[0].view(B, HW, Cc)
        if control:
            bad = ~torch.isfinite(got.float().cpu())
            assert bad[B - 1, :, Cc - Cc // G:].all() and int(bad.sum()) == HW * (Cc // G)
        else:
            _close(got, _gn_ref(x, G, gamma, beta, 1e-5, False), rtol=3e-3, what=what)


# ---- GroupNorm with mean >> std (variance as E[x^2] - mean^2 from fp32 partial sums) ------------------------------------------------------
def _gn_far(shape, g):
    return (torch.randn(*shape, generator=g) * 0.5 + 8.0).half()          # mean = 16 std; the fp16 spacing at 8 is 2^-7


@pytest.mark.parametrize("B,HW,Cc", [(2, 4096, 320), (1, 65536, 128), (2, 64, 1280)])
def test_groupnorm_mean_far_above_std(dev, B, HW, Cc):
    """Inputs randn * 0.5 + 8 (mean = 16 std): the cancellation case of E[x^2] - mean^2, on the two-pass kernels (C = 320 at 4096 rows,
    128 at 65536) and the single-launch small-map path (64 x 1280).  Bound: test_groupnorm's _close(rtol = 3e-3), unchanged - a one-pass
    scheme with sequential fp32 chunks of 256 elements combined in fp64 errs by 4.2e-3 at this ratio against the limit of 1.5e-2."""
    from pbe_amd import ops
    g = _g(HW + Cc + 8)
    x = _gn_far((B, HW, Cc), g)
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    got = ops.groupnorm(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5, True)
    _close(got, _gn_ref(x, 32, gamma, beta, 1e-5, True), rtol=3e-3, what=f"groupnorm mean >> std C={Cc} HW={HW}")


def test_groupnorm_two_sources_mean_far_above_std(dev):
    from pbe_amd import ops
    g = _g(78)
    B, HW, C1, C2 = 2, 256, 640, 320
    x = _gn_far((B, HW, C1 + C2), g)
    gamma, beta = 1 + 0.1 * torch.randn(C1 + C2, generator=g), 0.1 * torch.randn(C1 + C2, generator=g)
    got = ops.groupnorm(x[..., :C1].contiguous().to(dev), gamma.to(dev), beta.to(dev), 1e-5, True, x2=x[..., C1:].contiguous().to(dev))
    _close(got, _gn_ref(x, 32, gamma, beta, 1e-5, True), rtol=3e-3, what="groupnorm two sources, mean >> std")


def test_conv_group_statistics_mean_far_above_std(dev):
    """conv3x3(group_stats = 32) -> groupnorm with a residual of mean 8: the conv's copy-out statistics (fp32 partial sums of the stored
    values) feed the normalisation pass; same bound."""
    from pbe_amd import ops
    g = _g(79)
    B, H, Cc = 2, 64, 320
    x = (torch.randn(B, H, H, Cc, generator=g) * 0.7).half().to(dev)
    wp = ops.pack_conv3x3(torch.randn(Cc, Cc, 3, 3, generator=g) / (3 * Cc ** 0.5) * 0.5).to(dev)
    r = _gn_far((B, H, H, Cc), g).to(dev)
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    y = ops.conv3x3(x, wp, None, resid=r, group_stats=32)
    assert getattr(y, "_pbe_gstats", None) is not None, "the conv left no statistics: the case does not test what it names"
    got = ops.groupnorm(y, gamma.to(dev), beta.to(dev), 1e-5, True)
    ref = _gn_ref(y.float().cpu().view(B, H * H, Cc), 32, gamma, beta, 1e-5, True).view(B, H, H, Cc)
    _close(got, ref, rtol=3e-3, what="groupnorm from the conv's statistics, mean >> std")


# =====================================================================================================================================
# Element-wise
# =====================================================================================================================================
TOTALS = [1, 255, 257, 999983]          # off the 256-thread grid; 999983 is prime


def _ew(dev, ins, outs, call, what, finite=True):
    """ins: name -> CPU tensor, contiguous by the entry point's contract (embedded flat: poison before the first and after the last
    element), outs: name -> (shape, dtype).  Runs `call(views)` once and checks the arenas -> {name: output view}."""
    v = {k: guard.embed(t.reshape(-1), device=dev)[0].view(t.shape) for k, t in ins.items()}
    o = {k: guard.sentinel_out(s[0], dtype=s[1], device=dev) for k, s in outs.items()}
    v.update({k: p[0] for k, p in o.items()})
    call(v)
    for view, arena in o.values():
        guard.assert_untouched(arena, view, what)
        guard.assert_fully_written(view, what)
        assert not finite or not view.dtype.is_floating_point or torch.isfinite(view).all(), f"{what}: non-finite"
    return {k: p[0] for k, p in o.items()}


@pytest.mark.parametrize("n", TOTALS)
def test_axpy_qsample_mul_planes(dev, n):
    """pbe_axpy_f32, pbe_qsample_blend_f32 (mask channels 1 and C), pbe_mul_planes_f32: no direct parity test elsewhere.  Against fp64:
    axpy is ONE fused multiply-add, correctly rounded: |d| <= 2^-24 |y|; mul_planes one multiplication: equal to torch's fp32 product;
    the blend is orig = a x0 + b noise, out = orig m + (1 - m) img, S = (|a x0| + |b noise|) |m| +
    |1 - m| |img|, 7 roundings without contraction, each of a term bounded by S -> |d| <= 8 * 2^-24 S (+ the subnormal floor).  Outputs in arenas, inputs between NaN.  Poison: NaN."""
    from pbe_amd import lib
    L = lib.load()
    g = _g(n)
    x, y0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a32 = float(torch.tensor(0.37, dtype=torch.float32))
    yv, ya = guard.embed(y0, device=dev)                                 # in place: y sits in an arena of NaN bits
    xv, _ = guard.embed(x, device=dev)
    lib.check(L.pbe_axpy_f32(yv.data_ptr(), 0.37, xv.data_ptr(), n, _stream()), "axpy")
    guard.assert_untouched(ya, yv, "axpy", pattern=guard.POISON_BITS[torch.float32])
    want = y0.double() + a32 * x.double()
    assert ((yv.double().cpu() - want).abs() <= U32 * want.abs() + 1e-45).all()
    xv[n - 1] = NAN                                                      # positive control: the last element of x reaches the last of y only
    lib.check(L.pbe_axpy_f32(yv.data_ptr(), 0.37, xv.data_ptr(), n, _stream()), "axpy")
    bad = ~torch.isfinite(yv.cpu())
    assert bad[n - 1] and int(bad.sum()) == 1
    B, Cc = 1, 3
    HW = n
    if n > 1000:
        B, Cc, HW = 1, 3, n // 3 + 1
    x0, noise, img = (torch.randn(B, Cc, HW, generator=g) for _ in range(3))
    for mc in (1, Cc):
        m = torch.rand(B, mc, HW, generator=g)
        o = _ew(dev, {"x0": x0, "noise": noise, "m": m, "img": img}, {"out": ((B * Cc * HW,), torch.float32)},
                lambda v: lib.check(L.pbe_qsample_blend_f32(v["x0"].data_ptr(), v["noise"].data_ptr(), v["m"].data_ptr(), v["img"].data_ptr(), 0.8, 0.6,
                                                            v["out"].data_ptr(), B, Cc, HW, mc, _stream()), "qsample_blend"), f"qsample_blend mask {mc}")
        a, b = (float(torch.tensor(c, dtype=torch.float32)) for c in (0.8, 0.6))
        md = m.double().expand(B, Cc, HW)
        want = (a * x0.double() + b * noise.double()) * md + (1 - md) * img.double()
        S = ((a * x0.double()).abs() + (b * noise.double()).abs()) * md.abs() + (1 - md).abs() * img.double().abs()
        assert ((o["out"].view(B, Cc, HW).double().cpu() - want).abs() <= 8 * U32 * S + 1e-38).all(), f"qsample_blend mask {mc}"
    m1 = torch.rand(B, 1, HW, generator=g)
    o = _ew(dev, {"x": x0, "m": m1}, {"out": ((B * Cc * HW,), torch.float32)},
            lambda v: lib.check(L.pbe_mul_planes_f32(v["x"].data_ptr(), v["m"].data_ptr(), v["out"].data_ptr(), B, Cc, HW, _stream()), "mul_planes"), "mul_planes")
    assert torch.equal(o["out"].view(B, Cc, HW).cpu(), x0 * m1)


@pytest.mark.parametrize("B,Cc", [(1, 1), (3, 85), (1, 257), (7, 768)])
def test_bcast_row(dev, B, Cc):
    """pbe_bcast_row_f16 (no direct parity test elsewhere): Y[b * y_bs + c] = fp16(a[c] + b[c]) with a gap of y_bs - C sentinel elements
    between the rows.  The fp32 sum of two fp16 values of this range is exact, so the result EQUALS torch's (a.float() + b.float()).half()."""
    from pbe_amd import ops
    g = _g(B + Cc)
    a, b = torch.randn(Cc, generator=g).half(), torch.randn(Cc, generator=g).half()
    out, arena = guard.sentinel_out((B, 1, Cc), row_pad=3, col_pad=8, device=dev)
    ops.bcast_row(guard.embed(a, device=dev)[0], guard.embed(b, device=dev)[0], out, B, out.stride(0))
    _outputs_ok([(out, arena)], "bcast_row")
    assert torch.equal(out.cpu()[:, 0], (a.float() + b.float()).half().expand(B, Cc))


@pytest.mark.parametrize("HW", [1, 255, 257, 9973, 999983])
def test_layout_and_sampler_kernels(dev, HW):
    """nchw <-> nhwc, plms_pack_input, plms_update, scale_latent, posterior_sample, image_post, geglu, u8_to_planes: inputs between poison
    (ld padding of the NHWC sources poisoned: channels past the ones the op reads), outputs in arenas, pixel counts off the 256-thread
    grid; each result equals ops.* on plain tensors bit for bit and the references / bounds of test_ops_gpu.py.  Poison: NaN (bytes: 0x7F)."""
    from pbe_amd import lib, ops
    L = lib.load()
    g = _g(HW)
    B, s = (2 if HW < 100000 else 1), _stream()
    f32, f16 = torch.float32, torch.float16
    # fp32 NCHW [B, 9, HW] -> fp16 NHWC [B, HW, 16], channels 9 .. 15 zero
    x = torch.randn(B, 9, HW, generator=g)
    o = _ew(dev, {"x": x}, {"y": ((B * HW * 16,), f16)},
            lambda v: lib.check(L.pbe_nchw_f32_to_nhwc_f16(v["x"].data_ptr(), v["y"].data_ptr(), B, 9, HW, 16, s), "nchw_to_nhwc"), "nchw_to_nhwc")
    nhwc = o["y"].view(B, HW, 16).cpu()
    assert torch.equal(nhwc[..., :9].float(), x.transpose(1, 2).half().float()) and (nhwc[..., 9:] == 0).all()
    # ... and back, reading 9 of ld = 16 channels: the other 7 are poison
    src = nhwc.clone()
    src[..., 9:] = NAN
    o = _ew(dev, {"x": src}, {"y": ((B * 9 * HW,), f32)},
            lambda v: lib.check(L.pbe_nhwc_f16_to_nchw_f32(v["x"].data_ptr(), v["y"].data_ptr(), B, 9, HW, 16, s), "nhwc_to_nchw"), "nhwc_to_nchw")
    assert torch.equal(o["y"].view(B, 9, HW).cpu(), x.half().float())
    # positive control of the family: NaN moved to the last channel the op reads (8 of 0 .. 8), last pixel -> that output element only
    src[B - 1, HW - 1, 8] = NAN
    o = _ew(dev, {"x": src}, {"y": ((B * 9 * HW,), f32)},
            lambda v: lib.check(L.pbe_nhwc_f16_to_nchw_f32(v["x"].data_ptr(), v["y"].data_ptr(), B, 9, HW, 16, s), "nhwc_to_nchw"), "nhwc_to_nchw", finite=False)
    bad = ~torch.isfinite(o["y"].view(B, 9, HW).cpu())
    assert bad[B - 1, 8, HW - 1] and int(bad.sum()) == 1
    # plms_pack_input
    xs, z, m = torch.randn(B, 4, HW, generator=g), torch.randn(B, 4, HW, generator=g), torch.rand(B, 1, HW, generator=g)
    o = _ew(dev, {"x": xs, "z": z, "m": m}, {"y": ((2 * B * HW * 16,), f16)},
            lambda v: lib.check(L.pbe_plms_pack_input(v["x"].data_ptr(), v["z"].data_ptr(), v["m"].data_ptr(), v["y"].data_ptr(), B, HW, 2, s), "plms_pack"), "plms_pack_input")
    x9 = o["y"].view(2 * B, HW, 16).float().cpu()
    ref = torch.cat([xs, z, m], 1).transpose(1, 2).half().float()
    assert torch.equal(x9[:B, :, :9], ref) and torch.equal(x9[B:, :, :9], ref) and (x9[..., 9:] == 0).all()
    # plms_update: eps_out NHWC with ld = 8, channels 4 .. 7 poison
    eps = torch.randn(2 * B, HW, 8, generator=g).half()
    eps[..., 4:] = NAN
    h1, h2, h3 = (torch.randn(B, 4, HW, generator=g) for _ in range(3))
    coef = [55 / 24, -59 / 24, 37 / 24, -9 / 24, 0.6, 1.25, 0.9, 0.43]
    arr = (C.c_float * 8)(*coef)
    o = _ew(dev, {"eps": eps, "x": xs, "h1": h1, "h2": h2, "h3": h3}, {k: ((B * 4 * HW,), f32) for k in ("e_t", "x_prev", "pred")},
            lambda v: lib.check(L.pbe_plms_update(v["eps"].data_ptr(), 8, 2, 5.0, v["x"].data_ptr(), v["h1"].data_ptr(), v["h2"].data_ptr(), v["h3"].data_ptr(), arr,
                                                  v["e_t"].data_ptr(), v["x_prev"].data_ptr(), v["pred"].data_ptr(), B, HW, s), "plms_update"), "plms_update")
    e_u, e_c = eps[:B, :, :4].float().transpose(1, 2), eps[B:, :, :4].float().transpose(1, 2)
    e = e_u + 5.0 * (e_c - e_u)
    ep = coef[0] * e + coef[1] * h1 + coef[2] * h2 + coef[3] * h3
    px0 = (xs - coef[4] * ep) * coef[5]
    for k, want in (("e_t", e), ("pred", px0), ("x_prev", coef[6] * px0 + coef[7] * ep)):
        _close(o[k].view(B, 4, HW), want, rtol=1e-5, atol=1e-5, what=f"plms {k}")
    # scale_latent: fp32 NCHW [B, 9, HW] -> fp16 NHWC [B, HW, 8]
    o = _ew(dev, {"z": x}, {"y": ((B * HW * 8,), f16)},
            lambda v: lib.check(L.pbe_scale_latent_f16(v["z"].data_ptr(), v["y"].data_ptr(), B, 9, HW, 1 / 0.18215, s), "scale_latent"), "scale_latent")
    zl = o["y"].view(B, HW, 8).float().cpu()
    # one fp32 product stored as fp16 - in one rounding (a fused convert) or two: within half an fp16 ulp (+ the fp32 rounding) of the product
    exact = (x[:, :4].double() * float(torch.tensor(1 / 0.18215, dtype=f32))).transpose(1, 2)
    assert ((zl[..., :4].double() - exact).abs() <= (2.0 ** -11 + 2.0 ** -23) * exact.abs() + 2.0 ** -25).all() and (zl[..., 4:] == 0).all()
    _same_bits(o["y"].view(B, 1, HW, 8), ops.scale_latent(x.view(B, 9, 1, HW).to(dev), 1 / 0.18215), "scale_latent")
    # posterior_sample: moments NHWC with ld = 16, channels 8 .. 15 poison
    mom = (torch.randn(B, HW, 16, generator=g) * 3).half()
    mom[..., 8:] = NAN
    pe = torch.randn(B, 4, HW, generator=g)
    o = _ew(dev, {"mom": mom, "eps": pe}, {"z": ((B * 4 * HW,), f32)},
            lambda v: lib.check(L.pbe_posterior_sample(v["mom"].data_ptr(), 16, v["eps"].data_ptr(), v["z"].data_ptr(), B, HW, 0.18215, s), "posterior"), "posterior_sample")
    mean, logvar = mom.float()[..., :4].transpose(1, 2), mom.float()[..., 4:8].transpose(1, 2)
    _close(o["z"].view(B, 4, HW), 0.18215 * (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * pe), rtol=1e-5, atol=1e-5, what="posterior")
    # image_post: fp16 NHWC ld = 8, channels 3 .. 7 poison (fminf / fmaxf would launder a NaN into 0 or 1: 6e4 would clamp too - the output
    # arena and the exact reference are the check; a read of channel 3 instead of 2 shows as a wrong value)
    img = (torch.randn(B, HW, 8, generator=g) * 2).half()
    img[..., 3:] = NAN
    o = _ew(dev, {"img": img}, {"y": ((B * 3 * HW,), f32)},
            lambda v: lib.check(L.pbe_image_post_f32(v["img"].data_ptr(), v["y"].data_ptr(), B, HW, 8, s), "image_post"), "image_post")
    _close(o["y"].view(B, 3, HW), ((img.float()[..., :3] + 1) / 2).clamp(0, 1).transpose(1, 2), rtol=1e-6, atol=1e-6, what="image_post")
    # geglu [M, 2F] -> [M, F]
    M, Fh = HW, 24
    h = torch.randn(M, 2 * Fh, generator=g).half()
    o = _ew(dev, {"h": h}, {"y": ((M * Fh,), f16)}, lambda v: lib.check(L.pbe_geglu_f16(v["h"].data_ptr(), v["y"].data_ptr(), M, Fh, s), "geglu"), "geglu")
    a, gate = h.float().chunk(2, -1)
    _close(o["y"].view(M, Fh), a * F.gelu(gate), what="geglu")
    _same_bits(o["y"].view(M, Fh), ops.geglu(h.to(dev)), "geglu")
    # u8_to_planes: u8 HWC [B, HW, 3] -> fp32 planes, and the two mask forms
    u8 = torch.randint(0, 256, (B, HW, 3), generator=g, dtype=torch.uint8)
    mean3, std3 = (C.c_float * 3)(0.48, 0.45, 0.40), (C.c_float * 3)(0.26, 0.27, 0.28)
    o = _ew(dev, {"u8": u8}, {"y": ((B * 3 * HW,), f32)},
            lambda v: lib.check(L.pbe_u8_to_planes_f32(v["u8"].data_ptr(), v["y"].data_ptr(), B, 3, HW, mean3, std3, 0, s), "u8_to_planes"), "u8_to_planes")
    _same_bits(o["y"].view(B, 3, HW, 1), ops.u8_to_planes(u8.view(B, HW, 1, 3).to(dev), [0.48, 0.45, 0.40], [0.26, 0.27, 0.28]), "u8_to_planes")
    want = (u8.float().transpose(1, 2) / 255 - torch.tensor([0.48, 0.45, 0.40])[None, :, None]) / torch.tensor([0.26, 0.27, 0.28])[None, :, None]
    _close(o["y"].view(B, 3, HW), want, rtol=1e-6, atol=1e-6, what="u8_to_planes")
    for mode in (1, 2):
        o = _ew(dev, {"u8": u8[..., :1].contiguous()}, {"y": ((B * HW,), f32)},
                lambda v: lib.check(L.pbe_u8_to_planes_f32(v["u8"].data_ptr(), v["y"].data_ptr(), B, 1, HW, None, None, mode, s), "u8_to_planes"), f"u8 mask {mode}")
        inv = 1 - u8[..., 0].float() / 255
        _close(o["y"].view(B, HW), (inv >= 0.5).float() if mode == 1 else inv, rtol=0, atol=1e-6, what=f"u8 mask form {mode}")


def test_patchify_timestep_resize_canvas(dev):
    """clip_patchify, timestep_embedding, resize_bilinear (both filters), planes_to_u8_canvas: outputs in arenas, inputs between poison;
    equal to ops.* on plain tensors bit for bit (whose parity tests hold the references).  Canvas: the rectangle touching each canvas
    edge, every byte outside it unchanged."""
    from pbe_amd import lib, ops
    L = lib.load()
    g = _g(31)
    s, f32, f16 = _stream(), torch.float32, torch.float16
    px = torch.randn(2, 3, 28, 28, generator=g)
    o = _ew(dev, {"px": px}, {"y": ((2 * 4 * 592,), f16)},
            lambda v: lib.check(L.pbe_clip_patchify_f16(v["px"].data_ptr(), v["y"].data_ptr(), 2, 28, 14, 592, s), "patchify"), "clip_patchify")
    got = o["y"].view(8, 592).float().cpu()
    assert torch.equal(got[:, :588], F.unfold(px, 14, stride=14).transpose(1, 2).reshape(8, 588).half().float()) and (got[:, 588:] == 0).all()
    for Bt, dim in ((1, 320), (5, 322), (3, 2)):
        t = torch.randint(0, 1000, (Bt,), generator=g)
        td = t.to(dev)
        y, arena = guard.sentinel_out((Bt * dim,), device=dev)
        lib.check(L.pbe_timestep_embedding_f16(td.data_ptr(), y.data_ptr(), Bt, dim, 10000.0, s), "timestep_embedding")
        _outputs_ok([(y, arena)], "timestep_embedding")
        _same_bits(y.view(Bt, dim), ops.timestep_embedding(td, dim), "timestep_embedding")
        half = dim // 2
        ang = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half).double() / half)[None]
        _close(y.view(Bt, dim)[:, :2 * half], torch.cat([ang.cos(), ang.sin()], 1), rtol=1e-3, atol=2e-3, what="timestep_embedding")
    for (P, Hi, Wi, Ho, Wo) in ((3, 100, 77, 13, 31), (2, 9, 7, 31, 17), (1, 1, 1, 5, 3)):
        x = torch.rand(1, P, Hi, Wi, generator=g)
        for aa in (1, 0):
            o = _ew(dev, {"x": x}, {"y": ((P * Ho * Wo,), f32)},
                    lambda v: lib.check(L.pbe_resize_bilinear_f32(v["x"].data_ptr(), v["y"].data_ptr(), P, Hi, Wi, Ho, Wo, aa, s), "resize"), "resize_bilinear")
            ref = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False, antialias=bool(aa))
            assert (o["y"].view(1, P, Ho, Wo).cpu() - ref).abs().max().item() <= 2e-6
    Hc, Wc, H, W = 13, 11, 5, 4
    img = torch.rand(3, H, W, generator=g) * 1.4 - 0.2
    one = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(0.0, 0.0, 0.0)
    for (y0, x0) in ((0, 0), (0, Wc - W), (Hc - H, 0), (Hc - H, Wc - W), (4, 3)):
        flat, farena = guard.sentinel_out((Hc * Wc * 3,), dtype=torch.uint8, device=dev)
        lib.check(L.pbe_planes_to_u8_canvas(guard.embed(img.reshape(-1), device=dev)[0].data_ptr(), flat.data_ptr(), H, W, Hc, Wc, y0, x0, one[0], one[1], 0, s), "canvas")
        rect = torch.as_strided(farena, (H, W * 3), (Wc * 3, 1), flat.storage_offset() + (y0 * Wc + x0) * 3)
        guard.assert_untouched(farena, rect, f"canvas rectangle at ({y0}, {x0})")
        want = (255 * img.clamp(0, 1)).to(torch.uint8).permute(1, 2, 0).reshape(H, W * 3)
        assert (rect.cpu().int() - want.int()).abs().max().item() <= 1          # (trunc of 255 x: a contraction may move a value across an integer)
        ref_canvas = torch.full((Hc, Wc, 3), guard.SENTINEL_BITS[torch.uint8], dtype=torch.uint8, device=dev)
        ops.planes_to_canvas(img.to(dev), ref_canvas, y0, x0)
        _same_bits(flat.view(Hc, Wc, 3), ref_canvas, "planes_to_u8_canvas")
