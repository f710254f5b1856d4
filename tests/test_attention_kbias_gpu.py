"""pbe_attention_kbias_f16 (the key-bias form of attn_kernel) on the GPU: every case against the fp64 gate of tests/kbiasref.py -
every output element finite and within the rounding model's bound, rel-L2 at most 1.5 x the fp32 emulation's - at the hazards the
form has: tiles whose 64 keys are all absent (first, middle, ragged last), one live key, a bias step across ATTN_THR, the bias
belonging to the sample (XCD-remapped grids), the 64-queries-per-wave / two-tiles-per-barrier instantiation, and the memory edges."""
import pytest
import torch

import accgate as ag
import guard
import kbiasref as kr

pytestmark = pytest.mark.gpu


def _launch(q, k, v, bias, B, H, Nq, Nk, D, scale, dev, *, pre=False, guarded=False):
    """ops.attention(key_bias=...) on fp16 operands [B, N, H D]; guarded: the bias is a strided slice of a NaN-poisoned arena and the
    output lies in an arena of sentinel bits.  Returns (out, out arena or None, launch keys)."""
    from pbe_amd import ops
    HD = H * D
    npad = (Nk + 7) // 8 * 8
    vt = torch.zeros(B, HD, npad, dtype=torch.float16, device=dev)
    vt[:, :, :Nk] = v.to(dev).transpose(1, 2)
    qd, kd = q.to(dev), k.to(dev)
    arena = out = None
    if bias is None:
        bd = None
    elif guarded:
        bd, _ = guard.embed(bias, col_pad=5, row_pad=1, device=dev)
        out, arena = guard.sentinel_out((B, Nq, HD), row_pad=3, col_pad=8, device=dev)
    else:
        bd = bias.to(dev)
    ops._TIMES = {}
    try:
        out = ops.attention(qd, kd, vt, B, H, Nq, Nk, D, scale, q_strides=(Nq * HD, HD), k_strides=(Nk * HD, HD), vt_strides=(HD * npad, npad),
                            q_prescaled=pre, key_bias=bd, out=out)
        torch.cuda.synchronize()
        keys = list(ops._TIMES)
    finally:
        ops._TIMES = None
    return out, arena, keys


def _gate(dev, q, k, v, bias, B, H, Nq, Nk, D, *, guarded=False, what=""):
    scale = D ** -0.5
    got, arena, keys = _launch(q, k, v, bias, B, H, Nq, Nk, D, scale, dev, guarded=guarded)
    assert keys == [f"ab:{B}:{H}:{Nq}:{Nk}:{D}"], keys
    q4, k4, v4 = (ag.heads(t.to(dev), B, n, H, D) for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    bd = bias.to(dev)
    want, bound = kr.kb_reference(q4, k4, v4, bd, scale * ag.LOG2E)
    emu = kr.kb_emulate(q4, k4, v4, bd, scale * ag.LOG2E, ones=kr.kb_ones(D))
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    ok, text = kr.kb_verdict(got, want, bound, emu)
    print(f"{what}: {text}")
    assert ok, f"{what}: {text}"
    if guarded:
        guard.assert_untouched(arena, got, what)
        guard.assert_fully_written(got, what)
    return got, want


@pytest.mark.parametrize("pattern", kr.PATTERNS)
@pytest.mark.parametrize("D", [40, 80, 160])
def test_kbias_absent_tiles(dev, D, pattern):
    """B = 3, H = 2, Nq = 72, Nk = 130 (two full tiles and a 2-key ragged one), another bias row per sample: random over +-9 log2 units,
    and the first / middle / ragged tile wholly absent, and exactly one live key (in the ragged tile: the output is that V row to the
    fp16 store).  The bias comes out of a NaN-poisoned arena, the output lies between sentinels."""
    B, H, Nq, Nk = 3, 2, 72, 130
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 100 + D)
    bias = kr.kb_bias(pattern, B, Nk, kr.PATTERNS.index(pattern) * 7 + D)
    got, _ = _gate(dev, q, k, v, bias, B, H, Nq, Nk, D, guarded=True, what=f"D {D} {pattern}")
    if pattern == "one_live_key":
        for b in range(B):
            j = int(torch.nonzero(torch.isfinite(bias[b]))[0])
            assert torch.equal(got[b].cpu(), v[b, j][None, :].expand(Nq, -1)), f"sample {b}: not the V row of key {j}"


@pytest.mark.parametrize("D", [40, 80])
def test_kbias_step_across_threshold(dev, D):
    """Constant scores, the bias alone decides the raise: +7.5 (deferred) then +16 (raised), +8.5 (raised) then +16 (deferred at the new
    reference), and a descending row - everything at the old reference moves exactly once."""
    B, H, Nq, Nk = 3, 2, 72, 130
    q, k, v, bias = kr.step_operands(B, H, Nq, Nk, D, 5 + D)
    _gate(dev, q, k, v, bias, B, H, Nq, Nk, D, what=f"D {D} step")


@pytest.mark.parametrize("Nq,Nk,counts", [(256, 4, (1, 3)), (64, 4, (1, 3)), (256, 20, (7, 20)), (64, 20, (20, 1))])
def test_kbias_cross_shapes_of_the_1280_wide_levels(dev, Nq, Nk, counts):
    """B = 2, H = 8, D = 160 (B H % 8 == 0: workgroup ids are remapped over the XCDs) with per-sample exemplar counts."""
    B, H, D = 2, 8, 160
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, Nq + Nk)
    _gate(dev, q, k, v, kr.counts_bias(counts, Nk), B, H, Nq, Nk, D, guarded=True, what=f"a:{B}:{H}:{Nq}:{Nk}:{D} counts {counts}")


def test_kbias_clip_patch_tokens(dev):
    """Nk = 257 (CLIP patch tokens: four full tiles and one key), D = 40, random counts per sample."""
    B, H, Nq, Nk, D = 2, 8, 100, 257, 40
    g = torch.Generator().manual_seed(257)
    counts = tuple(int(c) for c in torch.randint(1, Nk + 1, (B,), generator=g))
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 257)
    _gate(dev, q, k, v, kr.counts_bias(counts, Nk), B, H, Nq, Nk, D, guarded=True, what=f"Nk 257 counts {counts}")
    _gate(dev, q, k, v, kr.counts_bias((Nk, 1), Nk), B, H, Nq, Nk, D, what="Nk 257 counts (257, 1)")


def test_kbias_two_query_blocks_two_tiles_per_barrier(dev):
    """B = 8, H = 8, Nq = 2048, Nk = 130, D = 40: the smallest grid for which the dispatch takes 64 queries per wave and two tiles per
    barrier, with the first tile wholly absent (a different live range per sample)."""
    B, H, Nq, Nk, D = 8, 8, 2048, 130, 40
    assert ((Nq + 255) // 256) * B * H >= 512 and ((Nq - 256 + 255) // 256) * B * H < 512
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 2048, device=dev)
    bias = kr.kb_bias("first_tile_absent", B, Nk, 40)
    _gate(dev, q.cpu(), k.cpu(), v.cpu(), bias, B, H, Nq, Nk, D, what="<48,2,2> first tile absent")


@pytest.mark.parametrize("D,qw", [(8, 0), (24, 0), (64, 0), (96, 0), (64, 2), (80, 2)], ids=["8", "24", "64", "96", "64-qw2", "80-qw2"])
def test_kbias_other_head_dims(dev, D, qw):
    """With the other tests, every branch of the pbe_attention_kbias_f16 dispatch: D = 24 and 96 take the 32- and 128-wide forms, and
    ops.tune(3, 2) the 64-queries-per-wave forms of D = 64 and 80 (the heuristic takes them from 512 workgroups on)."""
    from pbe_amd import ops
    B, H, Nq, Nk = 2, 3, 72, 130
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 300 + D)
    bias = kr.kb_bias("middle_tile_absent", B, Nk, D)
    try:
        ops.tune(3, qw)
        _gate(dev, q, k, v, bias, B, H, Nq, Nk, D, guarded=True, what=f"D {D} qw {qw}")
    finally:
        ops.tune(3, 0)


def test_kbias_poison_is_live_inside_the_extent(dev):
    """Positive control of the poison: a NaN bias INSIDE [B, Nk] reaches that sample's output (and no other sample's)."""
    B, H, Nq, Nk, D = 3, 2, 72, 130, 80
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 180)
    bias = kr.kb_bias("random", B, Nk, 80)
    bias[1, Nk - 1] = float("nan")
    got, _, _ = _launch(q, k, v, bias, B, H, Nq, Nk, D, D ** -0.5, dev, guarded=True)
    assert not torch.isfinite(got[1].float()).any()
    assert torch.isfinite(got[0].float()).all() and torch.isfinite(got[2].float()).all()


@pytest.mark.parametrize("D", [40, 80, 160])
def test_kbias_zero_bias_against_the_unbiased_kernel(dev, D):
    """Zero bias and pbe_attention_f16 on the same operands: both inside the gate, within twice the bound of each other.  They are NOT
    bit-identical at any of the three head dims (max|d| 4.9e-4 / 7.6e-6 / 6.1e-5 at D = 40 / 80 / 160 on values of order 0.5, i.e. at
    most one fp16 ulp): the key-bias form rounds fma(s, scale log2e, bias) and t - m separately where the unbiased form has one fma, and
    at D = 40 the unbiased kernel keeps its reference in the head-dim padding, which the key-bias form never does."""
    B, H, Nq, Nk = 3, 2, 72, 130
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 100 + D)
    zero = torch.zeros(B, Nk)
    got, want = _gate(dev, q, k, v, zero, B, H, Nq, Nk, D, what=f"D {D} zero bias")
    plain, _, keys = _launch(q, k, v, None, B, H, Nq, Nk, D, D ** -0.5, dev)
    assert keys == [f"a:{B}:{H}:{Nq}:{Nk}:{D}"]
    same = bool(torch.equal(got, plain))
    print(f"D {D}: zero bias {'is' if same else 'is NOT'} bit-identical to pbe_attention_f16; max|d| = {(got.float() - plain.float()).abs().max().item():.3e}")
    q4, k4, v4 = (ag.heads(t.to(dev), B, n, H, D) for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    _, bound = kr.kb_reference(q4, k4, v4, zero.to(dev), D ** -0.5 * ag.LOG2E)
    assert ag.compare(ag.flat(plain), ag.flat(want), ag.flat(bound)).ratio <= 1.0 or D == 40      # (the d = 40 form has its own, wider model: accgate)
    assert ((got.double() - plain.double()).abs() <= 2 * bound).all()


def test_kbias_refuses_bad_arguments(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    B, H, Nq, Nk, D = 1, 2, 32, 16, 40
    q, k, v = ag.attn_operands(B, H, Nq, Nk, D, 1)
    for bad in (torch.zeros(B, Nk + 1), torch.zeros(B + 1, Nk), torch.zeros(B, Nk, dtype=torch.float16)):
        with pytest.raises(PbeError):
            _launch(q, k, v, bad, B, H, Nq, Nk, D, D ** -0.5, dev)
    assert ops._TIMES is None
