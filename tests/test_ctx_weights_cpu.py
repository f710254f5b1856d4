"""Exemplar weights / per-sample exemplar counts of the multi-token cross-attention, without a GPU: the gate of the key-bias attention
kernel tested on itself (tests/kbiasref.py), the semantics against the unmodified ctxref.reference, and the host-side validation."""
import math

import pytest
import torch

import accgate as ag
import ctxref as cr
import kbiasref as kr

from pbe_amd.lib import PbeError

B, H, NQ, NK = 3, 2, 72, 130


def _case(D, pattern):
    q, k, v = ag.attn_operands(B, H, NQ, NK, D, 100 + D)
    bias = kr.kb_bias(pattern, B, NK, kr.PATTERNS.index(pattern) * 7 + D)
    scale = D ** -0.5
    q4, k4, v4 = ag.heads(q, B, NQ, H, D), ag.heads(k, B, NK, H, D), ag.heads(v, B, NK, H, D)
    return q4, k4, v4, bias, scale * ag.LOG2E, scale


_REF = {}


def _ref(D, pattern):
    """(operands, want, bound, emulation), computed once per case."""
    key = (D, pattern)
    if key not in _REF:
        q4, k4, v4, bias, sl, scale = _case(D, pattern)
        want, bound = kr.kb_reference(q4, k4, v4, bias, sl)
        _REF[key] = ((q4, k4, v4, bias, sl, scale), want, bound, kr.kb_emulate(q4, k4, v4, bias, sl, ones=kr.kb_ones(D)))
    return _REF[key]


@pytest.mark.parametrize("pattern", kr.PATTERNS)
@pytest.mark.parametrize("D", [40, 80, 160])
def test_kbias_gate_accepts_the_emulation_and_rejects_its_mutations(D, pattern):
    """On the operands of the GPU cases: the emulation of the key-bias kernel passes the gate and is finite; with the bias row of sample
    b + 1, with the bias multiplied by `scale` (a bias added before the scaling), and with one absent key given bias 0 it fails."""
    (q4, k4, v4, bias, sl, scale), want, bound, emu = _ref(D, pattern)
    assert torch.isfinite(emu.float()).all()
    ok, text = kr.kb_verdict(emu, want, bound, emu)
    assert ok, text
    muts = {"roll_bias": dict(roll_bias=True)}
    if pattern != "one_live_key":                          # (its only finite bias is 0: nothing to scale)
        muts["bias_times_scale"] = dict(bias_times=scale)
    if bool(torch.isinf(bias).any()):
        muts["absent_as_zero"] = dict(absent_as_zero=True)
    for name, kw in muts.items():
        bad = kr.kb_emulate(q4, k4, v4, bias, sl, ones=kr.kb_ones(D), **kw)
        ok, text = kr.kb_verdict(bad, want, bound, emu)
        assert not ok, f"D {D} {pattern}: the gate accepted mutation {name}: {text}"


def test_kbias_one_live_key_is_that_value_row():
    """Exactly one live key: the fp64 result IS that key's V row, for every query."""
    (q4, k4, v4, bias, sl, _), want, _, emu = _ref(40, "one_live_key")
    for b in range(B):
        j = int(torch.nonzero(torch.isfinite(bias[b]))[0])
        row = v4[b, :, j].reshape(-1).double()
        assert torch.equal(want[b], row[None, :].expand(NQ, -1))
        assert torch.equal(emu[b].double(), want[b])       # P = 1 on one key, 0 elsewhere: exact through the fp16 store


@pytest.mark.parametrize("D", [40, 80])
def test_kbias_step_across_the_threshold_is_seen_by_the_emulation(D):
    """The step operands raise the reference exactly where their docstring says (one deferred, one raised), and the emulation passes."""
    q, k, v, bias = kr.step_operands(3, H, NQ, NK, D, 5 + D)
    q4, k4, v4 = ag.heads(q, 3, NQ, H, D), ag.heads(k, 3, NK, H, D), ag.heads(v, 3, NK, H, D)
    sl = D ** -0.5 * ag.LOG2E
    want, bound = kr.kb_reference(q4, k4, v4, bias, sl)
    per_sample = []
    for b in range(3):
        st = {}
        kr.kb_emulate(q4[b:b + 1], k4[b:b + 1], v4[b:b + 1], bias[b:b + 1], sl, ones=kr.kb_ones(D), stats=st)
        per_sample.append(st["raises"])
    assert per_sample == [1, 1, 0]
    emu = kr.kb_emulate(q4, k4, v4, bias, sl, ones=kr.kb_ones(D))
    ok, text = kr.kb_verdict(emu, want, bound, emu)
    assert ok, text


def test_kbias_zero_bias_is_the_unbiased_reference():
    q4, k4, v4, _, sl, _ = _case(80, "random")
    zero = torch.zeros(B, NK)
    want, _ = kr.kb_reference(q4, k4, v4, zero, sl)
    plain, _ = ag.attn_reference(q4, k4, v4, sl, mpad=False, q_prescaled=False)
    assert torch.equal(want, plain)
    assert torch.equal(kr.kb_emulate(q4, k4, v4, zero, sl, ones=True), ag.attn_emulate(q4, k4, v4, sl, mpad=False, q_prescaled=False, ones=True))


# ---- semantics of the weights, against the unmodified ctxref.reference ---------------------------------------------------------------
def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("shape", kr.CTX_SHAPES, ids=lambda s: "B%d-N%d-C%d-H%d-K%d-p%d" % s)
def test_weight_zero_removes_the_token(shape):
    """log2 w folded into kbias: a token of weight 0 (-inf) gives, per sample, the result of the context without it - exact to 3e-15 in
    fp64 and to 6e-8 through the fp32 kbias (relative to the largest element)."""
    Bc, N, C, Hh, Nk, parts = shape
    o = cr.random_operands(Bc, N, C, Hh, Nk, parts)
    w = kr.ctx_weights(Bc, Nk, 11 + C)
    full, _ = cr.reference(kr.fold_log2w(o, w))
    full32, _ = cr.reference(kr.fold_log2w(o, w, through_fp32=True))
    for b in range(Bc):
        live = [j for j in range(Nk) if w[b, j] > 0]
        assert 1 <= len(live) <= min(kr.COUNTS[b], Nk)
        ob = kr.sample_tokens(o, b, live)
        alone, _ = cr.reference(kr.fold_log2w(ob, w[b:b + 1, live]))
        assert _rel(full[b * N:(b + 1) * N], alone) <= 3e-15
        assert _rel(full32[b * N:(b + 1) * N], alone) <= 6e-8


@pytest.mark.parametrize("shape", kr.CTX_SHAPES, ids=lambda s: "B%d-N%d-C%d-H%d-K%d-p%d" % s)
def test_integer_weights_repeat_the_token(shape):
    """Weights (2, 1, 0, 3) on four tokens give the context [t0, t0, t1, t3, t3, t3] (the pattern continues over longer contexts)."""
    Bc, N, C, Hh, Nk, parts = shape
    o = cr.random_operands(Bc, N, C, Hh, Nk, parts)
    counts = [(2, 1, 0, 3)[j % 4] for j in range(Nk)]
    w = torch.tensor([counts] * Bc, dtype=torch.float64)
    got, _ = cr.reference(kr.fold_log2w(o, w))
    got32, _ = cr.reference(kr.fold_log2w(o, w, through_fp32=True))
    rep = [j for j in range(Nk) for _ in range(counts[j])]
    for b in range(Bc):
        want, _ = cr.reference(kr.sample_tokens(o, b, rep))
        assert _rel(got[b * N:(b + 1) * N], want) <= 3e-15
        assert _rel(got32[b * N:(b + 1) * N], want) <= 6e-8


def test_uniform_weights_change_nothing():
    o = cr.random_operands(2, 72, 320, 8, 5)
    plain, _ = cr.reference(o)
    for c in (1.0, 0.25, 7.0):
        got, _ = cr.reference(kr.fold_log2w(o, torch.full((2, 5), c, dtype=torch.float64)))
        assert _rel(got, plain) <= 3e-15
    assert torch.equal(cr.reference(kr.fold_log2w(o, torch.ones(2, 5, dtype=torch.float64), through_fp32=True))[0], cr.reference(o)[0])


@pytest.mark.parametrize("shape", kr.CTX_SHAPES, ids=lambda s: "B%d-N%d-C%d-H%d-K%d-p%d" % s)
def test_ctx_emulation_stays_finite_with_absent_tokens(shape):
    """ctxref.emulate (the fused kernel's arithmetic) takes -inf entries of kbias: finite, and as accurate as unweighted."""
    Bc, N, C, Hh, Nk, parts = shape
    o = cr.random_operands(Bc, N, C, Hh, Nk, parts)
    ow = kr.fold_log2w(o, kr.ctx_weights(Bc, Nk, 11 + C), through_fp32=True)
    assert bool(torch.isinf(ow.kbias).any())
    emu, want = cr.emulate(ow), cr.reference(ow)[0]
    ok, text = cr.verdict(emu, want, emu)
    print(text)
    assert ok, text
    assert ag.rel_l2(emu, want) <= ag.REL_L2_FACTOR * ag.rel_l2(cr.emulate(o), cr.reference(o)[0])


# ---- host validation ---------------------------------------------------------------------------------------------------------------------
def test_prepare_context_weights_validates():
    from ldm.modules.attention import ContextWeights, prepare_context_weights
    ctx = torch.zeros(2, 3, 8)
    assert prepare_context_weights(ctx, None) is None
    cw = prepare_context_weights(ctx, [[2.0, 1.0, 0.0], [0.0, 0.0, 0.5]])
    assert isinstance(cw, ContextWeights) and cw.log2w.dtype == torch.float32 and tuple(cw.log2w.shape) == (2, 3)
    assert cw.log2w.tolist() == [[1.0, 0.0, -math.inf], [-math.inf, -math.inf, -1.0]]
    assert prepare_context_weights(ctx, cw) is cw
    for bad in ([[1.0, -1.0, 1.0], [1.0, 1.0, 1.0]], [[1.0, math.nan, 1.0], [1.0, 1.0, 1.0]], [[1.0, math.inf, 1.0], [1.0, 1.0, 1.0]],
                [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], [[1.0, 1.0], [1.0, 1.0]], [1.0, 1.0, 1.0], [[1.0, 1.0, 1.0]]):
        with pytest.raises(PbeError):
            prepare_context_weights(ctx, bad)


def test_pad_conditionings():
    from pbe_amd.pipeline import pad_conditionings
    g = torch.Generator().manual_seed(3)
    conds = [torch.randn(k, 8, generator=g) for k in (3, 1, 2)]
    ctx, w = pad_conditionings(conds)
    assert tuple(ctx.shape) == (3, 3, 8) and tuple(w.shape) == (3, 3) and w.dtype == torch.float64
    assert w.tolist() == [[1.0, 1.0, 1.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0]]
    for i, c in enumerate(conds):
        assert torch.equal(ctx[i, :c.shape[0]], c)
        assert torch.equal(ctx[i, c.shape[0]:], c[:1].expand(3 - c.shape[0], -1))      # padding = a copy of a real token
    _, w2 = pad_conditionings(conds, [[2.0, 1.0, 0.0], [0.5], [0.0, 3.0]])
    assert w2.tolist() == [[2.0, 1.0, 0.0], [0.5, 0.0, 0.0], [0.0, 3.0, 0.0]]
    for bad in ([[1.0, 1.0, 1.0], [0.0], [1.0, 1.0]], [[1.0, 1.0, 1.0], [1.0], [1.0, -1.0]], [[1.0, 1.0], [1.0], [1.0, 1.0]], [[1.0, 1.0, 1.0], [1.0]]):
        with pytest.raises(PbeError):
            pad_conditionings(conds, bad)
    with pytest.raises(PbeError):
        pad_conditionings([])


def test_guidance_weights_of_the_samplers():
    from ldm.models.diffusion.plms import guidance_context, guidance_weights
    cond, uc = torch.randn(2, 3, 8), torch.randn(1, 1, 8)
    assert guidance_weights(None, cond, 2, True) is None
    w = guidance_weights([[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], cond, 2, True)
    assert w.tolist() == [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    assert tuple(guidance_context(cond, uc, 2, "cpu").shape[:2]) == tuple(w.shape)
    assert guidance_weights([[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], cond, 2, False).tolist() == [[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    with pytest.raises(PbeError):
        guidance_weights([[1.0, 1.0]], cond, 2, True)
    with pytest.raises(PbeError):                          # an unconditional context of another length still raises
        guidance_context(cond, torch.randn(1, 2, 8), 2, "cpu")


def test_cli_reference_weight_arguments():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_pbe_inference_cli", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parse(["--reference_path", "a.jpg", "b.jpg"]).reference_weight is None
    assert cli.parse(["--reference_path", "a.jpg", "b.jpg", "--reference_weight", "2", "1"]).reference_weight == [2.0, 1.0]
    for bad in (["--reference_weight", "1"], ["--reference_weight", "0", "0"], ["--reference_weight", "1", "-1"], ["--reference_weight", "nan", "1"]):
        with pytest.raises(SystemExit):
            cli.parse(["--reference_path", "a.jpg", "b.jpg"] + bad)


def test_symbols_and_launch_keys_exist():
    """The additive entry points are declared on both sides of the binding (the header comparison itself is test_host_cpu.py's)."""
    from pbe_amd import lib
    assert "pbe_attention_kbias_f16" in lib.SYMBOLS and "pbe_ctx_attention_w_f16" in lib.SYMBOLS
    assert lib.ABI_VERSION == 8
