"""CPU checks of the tuned-table gate (tests/tilecheck.py): every table key becomes a launch that plans to the table's own (tile,
split-K), the per-element comparator passes an honest fp32 result in another summation order and rejects the ways a tile goes wrong,
and the sampled conv / V^T references agree with whole-tensor references.  Nothing is launched."""
import math

import torch
import torch.nn.functional as F

import tilecheck as tc


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_case_of_builds_every_table_entry():
    table = tc.load_table()
    cases = [tc.case_of(k) for k in table]
    assert len(cases) == len(table) and len({c.id for c in cases}) == len(table)
    for c in cases:
        assert c.planned == (c.tile, c.splits) and c.bm > 0 and c.bn > 0, c.describe()
        assert c.id == c.key + ("|plain" if c.fallback else "")
    assert {c.form for c in cases} == {"g", "gx", "g8", "c"}


def _gemm_operands(M, N, K, seed):
    g = _g(seed)
    a = torch.randn(M, K, generator=g).half().double()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().double()
    bias = torch.randn(N, generator=g).double()
    res = torch.randn(M, N, generator=g).half().double()
    return a, w, bias, res


def _honest(a, w, bias, res, slabs):
    """fp32 partial products over `slabs` k-slabs summed in turn, bias in fp32, fp16 store, fp16 residual add."""
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for s in range(slabs):
        k0, k1 = s * K // slabs, (s + 1) * K // slabs
        acc += a[:, k0:k1].float() @ w[:, k0:k1].float().t()
    y = (acc + bias.float()).half().float()
    return (y + res.float()).half().double()


def _expect(a, w, bias, res):
    return tc.expect(a @ w.t(), a.abs() @ w.abs().t(), a.shape[1], bias=bias, resid=res)


def test_comparator_passes_fp32_result_in_another_order():
    a, w, bias, res = _gemm_operands(256, 192, 24 * 64, 1)
    want, bound = _expect(a, w, bias, res)
    bound = tc.clamp_to_close(want, bound, tc.CLOSE["gemm"])
    rep = tc.check(_honest(a, w, bias, res, 24), want, bound, "24 slabs")
    assert rep.ratio <= 1.0
    tc.check(_honest(a, w, bias, res, 1), want, bound, "one pass")


def test_comparator_rejects_missing_last_kslice_at_largest_k():
    K = max(tc.Case(k, v).K for k, v in tc.load_table().items())
    a, w, bias, res = _gemm_operands(64, 64, K, 2)
    want, bound = _expect(a, w, bias, res)
    bound = tc.clamp_to_close(want, bound, tc.CLOSE["gemm"])
    got = _honest(a[:, :-64], w[:, :-64], bias, res, 1)
    assert tc.compare(got, want, bound).ratio > 1.0


def test_comparator_rejects_one_element_off_by_2_pow_minus_7():
    a, w, bias, res = _gemm_operands(128, 160, 1280, 3)
    want, bound = _expect(a, w, bias, res)
    got = _honest(a, w, bias, res, 4)
    i = int(torch.argmin((bound / want.abs()).view(-1)))          # the element with the tightest relative bound is the one to hide in
    j = int(torch.argmax(want.abs().view(-1)))
    for e in (i, j):
        bad = got.clone().view(-1)
        bad[e] = bad[e] * (1 + 2.0 ** -7)
        assert tc.compare(bad.view_as(got), want, bound).ratio > 1.0, e


def test_comparator_rejects_transposed_8x8_block():
    a, w, bias, res = _gemm_operands(128, 128, 640, 4)
    want, bound = _expect(a, w, bias, res)
    got = _honest(a, w, bias, res, 2)
    bad = got.clone()
    bad[40:48, 72:80] = got[40:48, 72:80].t()
    assert tc.compare(bad, want, bound).ratio > 1.0


def test_comparator_rejects_unwritten_ragged_last_tile():
    M, bm = 300, 128
    a, w, bias, res = _gemm_operands(M, 160, 960, 5)
    want, bound = _expect(a, w, bias, res)
    got = _honest(a, w, bias, res, 3)
    rows = tc.gemm_rows(M, bm, 7)
    assert set(range(256, 300)) <= set(rows) and set(range(128)) <= set(rows)
    stale = _honest(*_gemm_operands(M, 160, 960, 6), 3)
    for fill in (torch.zeros_like(got[256:]), stale[256:]):
        bad = got.clone()
        bad[256:] = fill
        ri = torch.tensor(rows)
        assert tc.compare(bad[ri], want[ri], bound[ri]).ratio > 1.0


# ---- the sampled references against whole-tensor references --------------------------------------------------------------------
def _exact_conv_operands(case, g):
    """Small-integer multiples of powers of two: every product, sum and the phase-summed weights are exact in fp16 / fp64."""
    x1 = (torch.randint(-8, 9, (case.B, case.H, case.W, case.C1), generator=g) / 8).half()
    x2 = (torch.randint(-8, 9, (case.B, case.H, case.W, case.C2), generator=g) / 8).half() if case.C2 else None
    w = (torch.randint(-4, 5, (case.Cout, case.C1 + case.C2, 3, 3), generator=g) / 64).float()
    bias = (torch.randint(-8, 9, (case.Cout,), generator=g) / 8).float()
    return x1, x2, w, bias


def _full_conv(case, x1, x2, w, bias):
    xx = x1 if x2 is None else torch.cat([x1, x2], -1)
    xx = xx.double().permute(0, 3, 1, 2)
    if case.ups:
        xx = F.interpolate(xx, scale_factor=2, mode="nearest")
    if case.pad == 0:
        xx = F.pad(xx, (0, 1, 0, 1))
    y = F.conv2d(xx, w.double(), bias.double(), stride=case.stride, padding=1 if case.pad else 0)
    return y.permute(0, 2, 3, 1)


def test_conv_reference_rows_match_whole_conv():
    from pbe_amd import ops
    for key in ("c:2:8:8:64:0:32:2:0:0", "c:2:8:8:64:0:32:2:1:0", "c:3:6:8:64:64:32:1:1:0", "c:2:4:8:128:0:32:1:1:1", "c:2:4:8:128:0:32:1:1:2"):
        case = tc.Case(key, 3 | (1 << 8))
        case.bm = 64
        x1, x2, w, bias = _exact_conv_operands(case, _g(len(key)))
        full = _full_conv(case, x1, x2, w, bias)
        t = {"x1": x1, "x2": x2, "bias": bias, "out": full.half()}
        if case.ups == 2:
            t["wp"] = ops.pack_conv3x3_up_phases(w)
        else:
            t["w"] = w.half()
        if case.rowvec:
            t["rowvec"] = (torch.randint(-8, 9, (case.B, case.Cout), generator=_g(1)) / 8).half()
            t["resid"] = (torch.randint(-8, 9, full.shape, generator=_g(2)) / 8).half()
            full = full + t["rowvec"].double()[:, None, None, :] + t["resid"].double()
            t["out"] = full.half()
        sel = tc.conv_rows(case, 3)
        assert (0, 0) in sel and (case.B - 1, case.Ho - 1) in sel
        got, want, bound, labels = tc.reference_conv(case, t, sel)
        rows = torch.cat([full[b, oy] for b, oy in sel])
        assert torch.equal(want, rows), key
        tc.check(got, want, bound, key, labels)
        bad = t["out"].clone()
        bad[case.B - 1, case.Ho - 1, -1, -1] += 1.0                     # the last pixel of the last tile
        t["out"] = bad
        assert tc.compare(tc.reference_conv(case, t, sel)[0], want, bound).ratio > 1.0, key


def test_vt_reference_reads_transposed_columns():
    M, K, T = 256, 320, 128
    case = tc.Case(f"gx:{M}:{3 * K}:{K}:1", 3 | (1 << 8))
    case.tokens = T
    g = _g(9)
    a = (torch.randint(-8, 9, (M, K), generator=g) / 8).half()
    w = (torch.randint(-4, 5, (3 * K, K), generator=g) / 64).half()
    bias = (torch.randint(-8, 9, (3 * K,), generator=g) / 8).float()
    colsum = w.double().sum(1).float()
    x = a.double()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    y = (x @ w.double().t() - mean * colsum.double()) / torch.sqrt(var + 1e-5)
    y[:, :K] *= case.alpha
    y += bias.double()
    vt = y[:, 2 * K:].reshape(M // T, T, K).transpose(1, 2).contiguous().half()
    t = {"A": a, "W": w, "bias": bias, "colsum": colsum, "out": y[:, :2 * K].half(), "vt_buf": vt}
    rows = tc.gemm_rows(M, 128, 1, 16)
    got, want, bound, labels = tc.reference_gemm(case, t, [(0, rows)])
    assert got.shape == (len(rows), 3 * K)
    tc.check(got, want, bound, "q | k | v^T", labels)
    t["vt_buf"] = y[:, 2 * K:].reshape(M // T, T, K).half().reshape(M // T, K, T)     # V not transposed: [b, t, c] read as [b, c, t]
    assert tc.compare(tc.reference_gemm(case, t, [(0, rows)])[0], want, bound).ratio > 1.0
