"""Exemplar attribution maps without a GPU: the verdict of tests/mapref.py accepts the fp32 emulation of the map-emitting kernel form
at every kernel shape and rejects the mistakes a kernel or its host code could make; the host validation of the map target; the
collector's bookkeeping (ldm.modules.attention.ContextMaps) against numpy, with the gather kernel restated in numpy."""
import numpy as np
import pytest
import torch

import ctxref
import kbiasref as kr
import mapref as mr


def _operands(shape, extra=0):
    B, N, C, H, Nk, parts = shape
    return ctxref.random_operands(B + extra, N, C, H, Nk, parts)


def _tables(shape, o):
    """(name, table [o.B, N, Nk]) of the plain and the regional form; the regional case is drawn for o.B samples."""
    B, N, C, H, Nk, parts = shape
    case = mr.region_case((o.B,) + tuple(shape[1:]))
    return [("plain", mr.zeros_table(o)), ("regions", case["table"])]


@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_emulation_passes_the_verdict(shape):
    o = _operands(shape)
    worst = 0.0
    for name, table in _tables(shape, o) + [("weights", mr.weights_table(o, kr.ctx_weights(o.B, o.Nk, 11 + o.C)))]:
        want, emu = mr.reference(o, table), mr.emulate(o, table)
        ok, text = mr.verdict(emu, want, emu, table)
        print(f"{mr.shape_id(shape)} {name}: {text}")
        assert ok, f"{name}: {text}"
        worst = max(worst, float((emu.double() - want).abs().max()))
    assert worst <= 0.5 * mr.ABS_BOUND, worst             # the emulation sits well inside the derived bound


@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_verdict_rejects_wrong_maps(shape):
    B, N, C, H, Nk, parts = shape
    o = _operands(shape, extra=1)                         # one sample more: `next sample` exists at B = 1 too
    for name, table in _tables(shape, o):
        want, emu = mr.reference(o, table), mr.emulate(o, table)
        w0, e0, t0 = want[:B], emu[:B], table[:B]
        assert mr.verdict(e0, w0, e0, t0)[0]
        wrong = {
            "head sum not divided by H": mr.emulate(o, table, no_div=True)[:B],
            "map of sample b + 1": emu[1:B + 1],
            "(row, token) transposed at am_rs = Nk": e0.transpose(1, 2).reshape(B, N, Nk),
            "mean over H - 1 heads": mr.emulate(o, table, fewer_heads=True)[:B],
        }
        if name == "regions":
            wrong["table ignored"] = mr.emulate(o, mr.zeros_table(o))[:B]
        for what, got in wrong.items():
            ok, text = mr.verdict(got, w0, e0, t0)
            assert not ok, f"{mr.shape_id(shape)} {name}: accepted `{what}`: {text}"


def test_map_target_validation():
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    B, N, K = 2, 72, 4
    good = torch.zeros(B, N, K)
    assert ops.ctx_attention_map_check((good, True), B, N, K)[1] is True
    padded = torch.zeros(B, N + 1, K + 3)[:, :N, :K]
    assert ops.ctx_attention_map_check((padded, False), B, N, K)[0] is padded
    bads = {"shape": torch.zeros(B, N, K + 1), "tokens": torch.zeros(B, N + 1, K), "samples": torch.zeros(B + 1, N, K),
            "rank": torch.zeros(B * N, K), "fp32": good.half(), "unit stride": torch.zeros(B, N, 2 * K)[:, :, ::2],
            "rows of": torch.zeros(B, K, N).transpose(1, 2)}
    for what, bad in bads.items():
        with pytest.raises(PbeError, match="attn_map"):
            ops.ctx_attention_map_check((bad, True), B, N, K)
    with pytest.raises(PbeError, match="fp32"):
        ops.ctx_attention_map_check((good.double(), True), B, N, K)
    with pytest.raises(PbeError, match="stride"):
        ops.ctx_attention_map_check((bads["unit stride"], True), B, N, K)
    with pytest.raises(PbeError, match=r"\[2, 72, 4\]"):
        ops.ctx_attention_map_check((bads["shape"], True), B, N, K)
    with pytest.raises(PbeError):
        ops.ctx_attention_map_check(good, B, N, K)        # not a (tensor, accumulate) pair
    with pytest.raises(PbeError, match="is on"):
        ops.ctx_attention_map_check((good, True), B, N, K, torch.device("meta"))


def test_operands_carry_the_map_target_without_refolding():
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    B, H, K, C = 4, 8, 3, 64
    o = ops.CtxOperands(torch.zeros(B, H * K, C), torch.zeros(B, H * K), torch.zeros(B, H * K), torch.zeros(B, C, H * K), torch.zeros(C), H, K,
                        log2w=torch.zeros(B, K))
    acc = torch.zeros(2, 10, K)
    m = o.with_map(acc, True, 2)
    assert m.kq is o.kq and m.vo is o.vo and m.colsum is o.colsum and m.kbias is o.kbias and m.log2w is o.log2w and o.amap is None
    assert m.map_ranges() == [(0, 2), (2, 4)] and o.map_ranges() == [(0, 4)] and o.with_map(torch.zeros(4, 10, K)).map_ranges() == [(0, 4)]
    assert m.rows(0, 2).amap is None
    t, accum, b0 = m.rows(2, 4).amap
    assert t.data_ptr() == acc.data_ptr() and accum is True and b0 == 0 and tuple(t.shape) == (2, 10, K)
    assert m.rows(3, 4).amap[0].data_ptr() == acc[1:].data_ptr()
    assert m.with_row_weights(torch.zeros(B, 10, K)).amap is m.amap
    with pytest.raises(PbeError, match="a part of that range"):
        m.rows(1, 3)


def test_collector_bookkeeping_against_numpy(monkeypatch):
    from ldm.modules import attention as A
    from pbe_amd.lib import PbeError
    calls = []

    def gather(acc, grid, scale=1.0, out=None, accumulate=False, div=1.0):
        h, w = grid
        hw = (h, w) if out is None else tuple(out.shape[2:])
        calls.append((grid, hw, scale, div, accumulate))
        v = torch.from_numpy(mr.gather_numpy(acc.numpy(), grid, hw, scale, div))
        if out is None:
            return v
        out.copy_(out + v if accumulate else v)
        return out
    monkeypatch.setattr(A.ops, "ctx_map_gather", gather)
    B, K, lat = 2, 3, (12, 8)                             # a non-square latent grid and its halvings
    cm = A.ContextMaps().bind(B, K, "cpu")
    with pytest.raises(PbeError):
        cm.bind(B, K + 1, "cpu")
    with pytest.raises(PbeError, match="nothing was collected"):
        cm.result(lat)
    g = torch.Generator().manual_seed(5)
    levels = {(12, 8): 3, (6, 4): 5, (3, 2): 1}
    want = np.zeros((B, K, *lat), dtype=np.float64)
    per = {}
    for (h, w), n in levels.items():
        acc = cm.level(h, w)
        assert tuple(acc.shape) == (B, h * w, K) and acc.dtype == torch.float32 and not acc.any() and cm.level(h, w) is acc
        for _ in range(n):                                # n launches, each adds a softmax-like map
            acc += torch.softmax(torch.randn(B, h * w, K, generator=g), -1)
            cm.note(h, w, 1)
        per[(h, w)] = mr.gather_numpy(acc.numpy(), (h, w), (h, w), 1.0, float(n))
        want += mr.gather_numpy(acc.numpy(), (h, w), lat, 1.0 / 3, float(n)).astype(np.float64)
    assert cm.counts() == levels
    got = cm.result(lat)
    assert tuple(got.shape) == (B, K, *lat) and got.dtype == torch.float32
    assert np.abs(got.numpy() - want).max() <= 3 * 2.0 ** -24          # three fp32 adds of values <= 1
    assert np.abs(got.numpy().sum(1) - 1.0).max() < 1e-5               # shares: they sum to 1 over the exemplars
    pl = cm.per_level()
    assert set(pl) == set(levels)
    for k, v in pl.items():
        assert np.array_equal(v.numpy(), per[k])
    assert [c[3] for c in calls[:3]] == [3.0, 5.0, 1.0] and [c[4] for c in calls[:3]] == [False, True, True]
    with pytest.raises(PbeError, match="whole multiple"):
        cm.result((8, 8))
    # launches recorded inside a tape count when the tape is replayed, not when it is recorded
    cm.begin_tape()
    cm.note(6, 4, 2)
    tape = cm.end_tape()
    assert cm.counts()[(6, 4)] == 5 and tape == {(6, 4): 2}
    cm.replayed(tape)
    cm.replayed(tape)
    assert cm.counts()[(6, 4)] == 9
    # K = 1: nothing is launched, the maps are ones
    one = A.ContextMaps().bind(B, 1, "cpu")
    assert one.level(4, 4) is None
    one.note(4, 4, 0)
    assert torch.equal(one.result(lat), torch.ones(B, 1, *lat)) and torch.equal(one.per_level()[(4, 4)], torch.ones(B, 1, 4, 4))
