"""Multi-token cross-attention, the parts that need no GPU: the folded algebra against the oracle's transformer block, the fp16 emulation of
the kernel against the fp64 reference, the gate tested on itself (three mutations it must reject), and the host-side validation."""
import pytest
import torch

import ctxref
from accgate import rel_l2
from oracle_loader import O

BLOCK_TOL = 2e-3          # tests/test_model_gpu.py: one block against its reference module


def _block_sd(C, H, prefix="blk."):
    from ldm.modules.attention import BasicTransformerBlock
    from pbe_amd.weights import fill_module_
    blk = BasicTransformerBlock(C, H, C // H, context_dim=768)
    fill_module_(blk, prefix=prefix)
    return {prefix + k: v.detach().float() for k, v in blk.state_dict().items()}


def _inputs(B, N, C, Nk, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, C, generator=g), torch.randn(B, Nk, 768, generator=g)


@pytest.mark.parametrize("B,N,C,H,Nk,parts", ctxref.KERNEL_SHAPES, ids=lambda v: str(v))
def test_folded_form_matches_oracle_attn2_step(B, N, C, H, Nk, parts):
    """x1 + attn2(norm2(x1), ctx) of oracle/pbe_oracle.py against ctxref.reference fed the operands folded in fp64 (algebra only), then
    against the fp16 operands and the fp32 emulation of the kernel (rel-L2 in the message, below BLOCK_TOL)."""
    sd = _block_sd(C, H)
    x1, ctx = _inputs(B, N, C, Nk, 11 + C + Nk)
    x1 = x1.half().float()
    with torch.no_grad():
        want = O.cross_attention(sd, "blk.attn2.", O.layer_norm(x1, sd, "blk.norm2"), ctx, H) + x1
    kq, colsum, kbias, vo, bias = ctxref.fold(sd, "blk.", ctx, H, torch.float64)
    x2d = x1.view(B * N, C).half()
    exact = ctxref.Operands(x2d, kq, colsum, kbias, vo, bias, ctxref.row_partials(x2d, parts), B, N, C, H, Nk)
    x2, term = ctxref.reference(exact)
    r = rel_l2(x2.view(B, N, C), want.double())
    assert r <= 2e-6, f"folded algebra vs oracle attn2 step: rel-L2 {r:.3e}"
    rt = rel_l2(term.view(B, N, C), (want - x1).double())
    assert rt <= 2e-5, f"attn2 term vs oracle: rel-L2 {rt:.3e}"
    kq, colsum, kbias, vo, bias = ctxref.fold(sd, "blk.", ctx.half().float(), H, torch.float16)
    sent = ctxref.Operands(x2d, kq, colsum, kbias, vo, bias, exact.stats, B, N, C, H, Nk)
    emu = ctxref.emulate(sent)
    re_, rterm = rel_l2(emu.view(B, N, C), want.double()), rel_l2(emu.double().view(B, N, C) - x1.double(), (want - x1).double())
    assert re_ <= BLOCK_TOL and rterm <= BLOCK_TOL, f"fp16 emulation vs oracle: x2 rel-L2 {re_:.3e}, attn2 term rel-L2 {rterm:.3e} (BLOCK_TOL {BLOCK_TOL})"
    ok, text = ctxref.verdict(emu, ctxref.reference(sent)[0], emu)
    assert ok, text


def test_repeated_token_equals_single_token():
    """K copies of one context token give the one-token result (softmax weights 1/K of K equal values): why a one-token uc may be repeated."""
    C, H = 320, 8
    sd = _block_sd(C, H)
    x1, ctx = _inputs(2, 24, C, 1, 5)
    with torch.no_grad():
        one = O.cross_attention(sd, "blk.attn2.", O.layer_norm(x1, sd, "blk.norm2"), ctx, H)
        for K in (4, 5, 16):
            rep = O.cross_attention(sd, "blk.attn2.", O.layer_norm(x1, sd, "blk.norm2"), ctx.expand(-1, K, -1), H)
            assert rel_l2(rep, one.double()) <= 2e-6, K


def test_gate_rejects_mutations():
    """The gate on itself: the honest emulation passes; no max subtraction at large logits, a padding column given weight, and the
    mean * colsum term dropped from the LayerNorm fold are each refused."""
    B, N, C, H, Nk, parts = ctxref.LARGE_LOGITS_SHAPE
    big = ctxref.random_operands(B, N, C, H, Nk, parts, seed=3, logit_scale=60.0)
    want = ctxref.reference(big)[0]
    emu = ctxref.emulate(big)
    ok, text = ctxref.verdict(emu, want, emu)
    assert ok, text
    ok, text = ctxref.verdict(ctxref.emulate(big, no_max=True), want, emu)
    assert not ok, "no max subtraction passed the gate: " + text
    o = ctxref.random_operands(2, 130, 320, 8, 5, 1, seed=4)
    want, emu = ctxref.reference(o)[0], ctxref.emulate(o)
    assert ctxref.verdict(emu, want, emu)[0]
    for kw in (dict(pad_weight=True), dict(drop_colsum=True)):
        ok, text = ctxref.verdict(ctxref.emulate(o, **kw), want, emu)
        assert not ok, f"mutation {kw} passed the gate: {text}"


@pytest.mark.parametrize("C,H,Nk,tokens,M,word", [
    (96, 8, 4, 8, 16, "multiple of 64"), (1344, 8, 4, 8, 16, "multiple of 64"), (32, 8, 4, 8, 16, "64.."),
    (320, 8, 17, 8, 16, "context tokens"), (320, 8, 0, 8, 16, "context tokens"), (320, 16, 9, 8, 16, "takes <= 128"),
    (320, 8, 4, 7, 16, "whole samples"), (320, 8, 4, 0, 16, "whole samples")])
def test_host_validation_names_the_limit(C, H, Nk, tokens, M, word):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError, match=word):
        ops.ctx_attention_check(C, H, Nk, tokens, M)
    if Nk >= 1 and tokens >= 1:                      # the launch wrapper refuses before it looks for a GPU
        HJ = H * Nk
        o = ops.CtxOperands(torch.zeros(M // max(tokens, 1) or 1, HJ, C, dtype=torch.float16), torch.zeros(1, HJ), torch.zeros(1, HJ),
                            torch.zeros(1, C, HJ, dtype=torch.float16), torch.zeros(C), H, Nk)
        st = ops.RowStats(torch.zeros(1, M, 2), 1, M)
        with pytest.raises(PbeError, match=word):
            ops.ctx_attention(torch.zeros(M, C, dtype=torch.float16), o, st, 1e-5, tokens=tokens)


def test_host_validation_operand_mismatch_and_cpu_tensors():
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    C, H, Nk, N, B = 64, 8, 2, 8, 2
    HJ = H * Nk
    o = ops.CtxOperands(torch.zeros(B, HJ, C, dtype=torch.float16), torch.zeros(B, HJ), torch.zeros(B, HJ), torch.zeros(B, C, HJ, dtype=torch.float16),
                        torch.zeros(C), H, Nk)
    st = ops.RowStats(torch.zeros(1, B * N, 2), 1, B * N)
    x = torch.zeros(B * N, C, dtype=torch.float16)
    with pytest.raises(PbeError, match="samples of width"):
        ops.ctx_attention(torch.zeros(3 * N, C, dtype=torch.float16), o, ops.RowStats(torch.zeros(1, 3 * N, 2), 1, 3 * N), 1e-5, tokens=N)
    with pytest.raises(PbeError, match="CtxOperands"):
        ops.ctx_attention(x, None, st, 1e-5, tokens=N)
    with pytest.raises(PbeError, match="on the GPU"):          # valid shapes, CPU tensors: no CPU fallback
        ops.ctx_attention(x, o, st, 1e-5, tokens=N)


def test_sampler_context_lengths():
    """A one-token uc is repeated to the conditioning's K tokens; any other mismatch is refused."""
    from ldm.models.diffusion.plms import guidance_context
    from pbe_amd.lib import PbeError
    c, uc = torch.randn(2, 3, 16), torch.randn(1, 1, 16)
    ctx = guidance_context(c, uc, 2, "cpu")
    assert ctx.shape == (4, 3, 16) and ctx.dtype == torch.float16
    assert torch.equal(ctx[:2], uc.half().expand(2, 3, 16)) and torch.equal(ctx[2:], c.half())
    assert guidance_context(c[:, :1], uc, 2, "cpu").shape == (4, 1, 16)
    with pytest.raises(PbeError, match="one-token"):
        guidance_context(c, torch.randn(2, 2, 16), 2, "cpu")
