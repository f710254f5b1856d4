"""ctx_attn_kernel<RW, AM> on the GPU against the per-element gate of tests/ctxgate.py: every element of Y within its derived bound of
the fp64 reference (beside ctxref.verdict's two whole-tensor terms, unchanged), the map within mapref.verdict and its per-element term,
on the shapes that reach NJ = 3, H = 1, H = 16 and raw strides, over six operand recipes and the plain, weighted, row-weight and map
forms; bit-exact pins of Y and the map; and one positive control per form.  tests/test_ctxgate_cpu.py holds the same cases to the
emulation, and plants the faults."""
import pytest
import torch

import ctxgate as cg
import guard
from test_accuracy_gpu import report
from test_ctx_attention_gpu import _device_operands

pytestmark = pytest.mark.gpu

CASES = [(s, r) for s in cg.NEW_SHAPES + [cg.VIEW_SHAPE] for r in cg.RECIPES]
GUARDED = (cg.NEW_SHAPES[0], cg.VIEW_SHAPE)        # an NJ = 3 shape and the raw-stride shape: operands between poison, outputs in sentinel arenas
STAT_LIMITS = dict(rtol=2e-6, atol=1e-4)            # of test_kernel_against_fp64_reference


def _case_id(c):
    return f"{cg.shape_id(c[0])}-{c[1]}"


def _line(what, v):
    report(f"{what:64s} err/bound={v.ratio:.3f} at {v.where} rel_l2={v.r_got:.3e} (emulation {v.r_emu:.3e})")
    print(f"{what}: {v}")


def _with_form(oc, form, table, lw, dev, guarded=False):
    if form == "weights":
        oc.log2w = guard.embed(lw, col_pad=3, row_pad=1, device=dev)[0] if guarded else lw.to(dev)
        return oc
    if form == "regions":
        if guarded:
            B, N, Nk = table.shape
            t = guard.embed(table.reshape(B * N, Nk), col_pad=3, row_pad=2, device=dev)[0].view(B, N, Nk)
            assert t.stride(1) > Nk
            return oc.with_row_weights(t)
        return oc.with_row_weights(table.to(dev).contiguous())
    return oc


def _plain_launch(o, form, table, lw, dev, eps=cg.EPS):
    """(y, row statistics, x, operands, statistics) of a launch on dense operands."""
    from pbe_amd import ops
    x, oc, st = _device_operands(o, dev)
    oc = _with_form(oc, form, table, lw, dev)
    y, rs = ops.ctx_attention(x, oc, st, eps, tokens=o.N)
    return y, rs.buf[0], x, oc, st


def _guarded_launch(o, form, table, lw, dev):
    """The same launch with every operand inside a NaN-poisoned arena - ldx above C, padded Kq / Vo / colsum / kbias rows, ln_stats_ld
    above M - and Y (ldy above C) and the row statistics inside sentinel arenas: fully written, nothing outside touched."""
    from pbe_amd import ops
    B, N, C, H, Nk = o.B, o.N, o.C, o.H, o.Nk
    M = B * N
    x, _ = guard.embed(o.x, col_pad=24, device=dev)
    kq, _ = guard.embed(o.kq, row_pad=3, col_pad=8, device=dev)
    vo, _ = guard.embed(o.vo, row_pad=2, col_pad=0, device=dev)
    colsum, _ = guard.embed(o.colsum, col_pad=3, device=dev)
    kbias, _ = guard.embed(o.kbias, col_pad=3, device=dev)
    bias, _ = guard.embed(o.bias, device=dev)
    parts = o.stats.shape[0]
    sbuf = torch.full((parts, M + 5, 2), float("nan"), device=dev)
    sbuf[:, :M] = o.stats.to(dev)
    st = ops.RowStats(sbuf, parts, M + 5)
    y, y_arena = guard.sentinel_out((M, C), col_pad=40, device=dev)
    rs, rs_arena = guard.sentinel_out((2 * M,), dtype=torch.float32, device=dev)
    assert x.stride(0) > C and y.stride(0) > C
    for t in (x, kq, vo, y):
        guard.assert_aligned(t)
    oc = _with_form(ops.CtxOperands(kq, colsum, kbias, vo, bias, H, Nk), form, table, lw, dev, guarded=True)
    ops.ctx_attention(x, oc, st, cg.EPS, tokens=N, out=y, row_stats=ops.RowStats(rs.view(1, M, 2), 1, M))
    torch.cuda.synchronize()
    guard.assert_fully_written(y, "ctx_attention Y")
    guard.assert_fully_written(rs, "ctx_attention row statistics")
    guard.assert_untouched(y_arena, y, "ctx_attention Y")
    guard.assert_untouched(rs_arena, rs, "ctx_attention row statistics")
    return y.contiguous(), rs.view(M, 2).clone(), x, oc, st


def _map_pair(y, rs, x, oc, st, o, dev, guarded):
    """The map form of the same launch, storing and accumulating: Y and the statistics keep their bits; returns the stored map."""
    from pbe_amd import ops
    B, N, Nk = o.B, o.N, o.Nk
    if guarded:
        sbits = guard.SENTINEL_BITS[torch.float32]
        arena = torch.full((B + 1, N + 1, Nk + 3), sbits, dtype=torch.int32, device=dev).view(torch.float32)
        amap = arena[:B, :N, :Nk]
    else:
        amap = torch.full((B, N, Nk), float("nan"), device=dev)
    y1, rs1 = ops.ctx_attention(x, oc, st, cg.EPS, tokens=N, attn_map=(amap, False))
    assert torch.equal(y1, y) and torch.equal(rs1.buf[0], rs), "the map form changed Y or the row statistics"
    if guarded:
        ib = arena.view(torch.int32).cpu()
        inside = torch.zeros_like(ib, dtype=torch.bool)
        inside[:B, :N, :Nk] = True
        assert bool((ib[inside] != sbits).all()) and bool((ib[~inside] == sbits).all()), "map store outside t < tokens, j < Nk, or not everywhere inside"
    base = torch.randn(B, N, Nk, generator=torch.Generator().manual_seed(9)).to(dev)
    acc = base.clone()
    y2, _ = ops.ctx_attention(x, oc, st, cg.EPS, tokens=N, attn_map=(acc, True))
    assert torch.equal(acc, base + amap) and torch.equal(y2, y), "accumulate is not base + stored, bit for bit"
    return amap.contiguous()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_element_against_fp64(dev, case):
    """Plain, weighted and row-weight launch, each also with the map (stored, then accumulated): every element of Y and of the map."""
    shape, recipe = case
    o = cg.operands(shape, recipe)
    guarded = shape in GUARDED
    for form in cg.FORMS:
        table, lw = cg.form_table(shape, recipe, form)
        y, rs, x, oc, st = (_guarded_launch if guarded else _plain_launch)(o, form, table, lw, dev)
        ref, emu = cg.reference(o, table), cg.emulate(o, table)
        v = cg.verdict(y, o, table, ref=ref, emu=emu[0])
        _line(f"ctx {form} {_case_id(case)}", v)
        assert v.ok, f"{form}: {v}"
        want = torch.stack([y.double().sum(1), (y.double() ** 2).sum(1)], 1).cpu()
        assert torch.allclose(rs.double().cpu(), want, **STAT_LIMITS), f"{form}: row statistics off by {(rs.double().cpu() - want).abs().max():.3e}"
        amap = _map_pair(y, rs, x, oc, st, o, dev, guarded)
        ok, ratio, where, text = cg.map_verdict(amap, o, table, ref=ref, emu=emu[1])
        report(f"{'ctx map ' + form + ' ' + _case_id(case):64s} err/bound={ratio:.3f} at {where}")
        print(f"ctx map {form} {_case_id(case)}: {text}")
        assert ok, f"{form}: {text}"


# ---- exact pins ------------------------------------------------------------------------------------------------------------------------
PINS = [(f, s) for f in cg.FORMS for s in cg.PIN_SHAPES[f]]


@pytest.mark.parametrize("pin", PINS, ids=lambda p: f"{p[0]}-{cg.shape_id(p[1])}")
def test_pins_bit_for_bit(dev, pin):
    """Y of every row of every sample and every channel, with and without the map, and the map itself: the expected bits."""
    from pbe_amd import ops
    form, shape = pin
    o, table, lw, want, hot = cg.pin_case(form, shape)
    y, rs, x, oc, st = _plain_launch(o, form, table, lw, dev)
    bits = want.half()
    diff = (y.cpu() != bits)
    where = cg.locate(int(torch.nonzero(diff.view(-1))[0]), o.N, o.C) if bool(diff.any()) else "-"
    report(f"{'ctx pin ' + form + ' ' + cg.shape_id(shape):64s} {int(diff.sum())} of {diff.numel()} elements differ (first: {where})")
    assert not bool(diff.any()), f"{int(diff.sum())} elements of Y differ, first at {where}"
    amap = torch.full((o.B, o.N, o.Nk), float("nan"), device=dev)
    y1, _ = ops.ctx_attention(x, oc, st, cg.EPS, tokens=o.N, attn_map=(amap, False))
    assert torch.equal(y1, y)
    bad = amap.double().cpu() != hot
    assert not bool(bad.any()), f"{int(bad.sum())} map elements differ, first at (b, t, j) = {tuple(torch.nonzero(bad)[0].tolist())}"


# ---- positive controls: one operand changed in a device copy, judged against the reference of the INTACT operands -----------------------
def _control(name, v):
    report(f"{'ctx control ' + name:64s} err/bound={v.ratio:.3f} at {v.where} (must exceed 1)")
    print(f"control {name}: {v}")
    assert v.ratio > 1.0 and not v.ok, f"{name}: the gate accepted a changed operand: {v}"


def test_control_plain_eps(dev):
    """eps sent as 1e-6 (GroupNorm's) on `flat`."""
    shape = cg.NEW_SHAPES[0]
    o = cg.operands(shape, "flat")
    y = _plain_launch(o, "plain", None, None, dev, eps=1e-6)[0]
    _control("plain: eps 1e-6 on flat", cg.verdict(y, o, None))


def test_control_weighted_swapped_tokens(dev):
    """log2w of the first and the last token of the last sample exchanged (a live token for an absent one)."""
    shape = cg.NEW_SHAPES[0]
    o = cg.operands(shape, "unit")
    table, lw = cg.form_table(shape, "unit", "weights")
    sw = lw.clone()
    sw[-1, 0], sw[-1, -1] = lw[-1, -1], lw[-1, 0]
    assert not torch.equal(sw, lw)
    y = _plain_launch(o, "weights", table, sw, dev)[0]
    _control("weighted: two tokens' log2w exchanged", cg.verdict(y, o, table))


def test_control_row_weight_next_sample(dev):
    """Every sample takes the table of the next one (regionref's next_sample)."""
    shape = cg.NEW_SHAPES[0]
    o = cg.operands(shape, "unit")
    table, _ = cg.form_table(shape, "unit", "regions")
    y = _plain_launch(o, "regions", cg.next_sample_table(shape), None, dev)[0]
    _control("row-weight: the next sample's table", cg.verdict(y, o, table))


def test_control_map_heads_and_tokens_exchanged(dev):
    """H = 8, Nk = 4 sent as H = 4, Nk = 8 (both legal, H Nk unchanged): Y leaves its bound and the map is refused."""
    from pbe_amd import ops
    shape = cg.VIEW_SHAPE
    B, N, C, H, Nk, parts = shape
    o = cg.operands(shape, "unit")
    x, oc, st = _device_operands(o, dev)
    sw = ops.CtxOperands(oc.kq, oc.colsum, oc.kbias, oc.vo, oc.bias, Nk, H)
    amap = torch.full((B, N, H), float("nan"), device=dev)
    y, _ = ops.ctx_attention(x, sw, st, cg.EPS, tokens=N, attn_map=(amap, False))
    _control("map: H and Nk exchanged", cg.verdict(y, o, None))
    assert not cg.mr.verdict(amap, cg.reference(o)[2], cg.emulate(o)[1])[0]
