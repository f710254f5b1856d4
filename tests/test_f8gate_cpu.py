"""tests/f8ref.py on the CPU: the e4m3 model against torch's conversion, the exactness claims of the exact tier in numpy float32, the
gate on the plain-fp32 emulation of layernorm_f8_kernel (it passes, under the 2 % cap, for every input recipe the GPU tests use), every
mutation rejected by the part of the gate that is meant to reject it, and ops.pack_linear_f8 (host code) code by code."""
import numpy as np
import pytest
import torch

import f8ref as f8

F = np.float32
EPS = 1e-5


# ---- the format -------------------------------------------------------------------------------------------------------------------------
def test_q_e4m3_is_identity_on_every_finite_code():
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    assert len(codes) == 254
    v = f8.decode(codes)
    assert torch.equal(v, codes.view(torch.float8_e4m3fn).double())
    q = f8.q_e4m3(v)
    assert torch.equal(q, v) and torch.equal(torch.signbit(q), torch.signbit(v))
    assert torch.equal(f8.encode(q), codes)
    assert torch.isnan(f8.decode(torch.tensor([0x7F, 0xFF], dtype=torch.uint8))).all()


def test_q_e4m3_agrees_with_torch_on_every_fp16_value():
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    h = h[torch.isfinite(h) & (h.abs() <= 448)]
    assert h.numel() > 48000
    want = h.to(torch.float8_e4m3fn)                  # one rounding: fp16 -> e4m3
    got = f8.q_e4m3(h.double())
    assert torch.equal(got, want.double())
    assert torch.equal(f8.encode(got), want.view(torch.uint8))


def test_q_e4m3_boundaries():
    q = lambda *v: f8.q_e4m3(torch.tensor(v, dtype=torch.float64)).tolist()
    assert q(2.0 ** -10, 2.0 ** -10 * (1 + 2.0 ** -40), 3 * 2.0 ** -10) == [0.0, 2.0 ** -9, 2.0 ** -8]          # ties to even
    assert q(17.0, 19.0, -17.0, 18.999999999) == [16.0, 20.0, -16.0, 18.0]
    assert q(1e9, -1e9, 463.9, 448 * (1 + 2.0 ** -23)) == [448.0, -448.0, 448.0, 448.0]
    assert f8.q_e4m3(torch.tensor([17.0, 19.0, -17.0]).double(), "away").tolist() == [18.0, 20.0, -18.0]
    assert f8.q_e4m3(torch.tensor([17.9, -19.9]).double(), "trunc").tolist() == [16.0, -18.0]
    assert torch.isnan(f8.q_e4m3(torch.tensor([448 * (1 + 2.0 ** -23)]).double(), saturate=False)).all()


# ---- exact tier: the claims that make byte equality a requirement -----------------------------------------------------------------------
def test_decision_values():
    v, want = f8.decision_values()
    assert v.dtype == F and len(v) == 1010 and len(np.unique(v[:505])) == 505
    i = int(np.nonzero(v == F(2.0 ** -10))[0][0])
    assert want[i] == 0x00 and want[i + 505] == 0x80      # the smallest midpoint rounds to zero, its negative to negative zero
    assert set(want.tolist()) == set(range(256)) - {0x7F, 0xFF}


@pytest.mark.parametrize("k", f8.EXACT_K)
def test_exact_tier_arithmetic_is_exact_in_fp32(k):
    """amax * fl32(1 / 448) == 2^k, 1 / 2^k and y * 2^-k exact, and (x - mean) * rstd * 0 + b == b with or without an fma."""
    two_k = F(2.0 ** k)
    scale = F(448.0) * two_k * (F(1.0) / F(448.0))
    assert scale == two_k and scale.dtype == F
    inv = F(1.0) / scale
    assert np.float64(inv) == 2.0 ** -k
    v, _ = f8.decision_values()
    for case in f8.exact_rows(512, k) + f8.exact_rows(2048, k):
        b = case["beta"].numpy()
        assert ((b * inv).astype(np.float64) == b.astype(np.float64) * 2.0 ** -k).all()      # the product the kernel converts: exact
        assert np.abs(b).max() == F(448.0) * two_k and (b[-2:] == np.array([448, -448], F) * two_k).all()
        x = case["x"].float().numpy()
        assert (x[-1] == x[-1, 0]).all()                                                      # the constant row
        mean = x.sum(1, keepdims=True, dtype=F) / F(x.shape[1])
        d = x - mean
        rstd = F(1.0) / np.sqrt((d * d).sum(1, keepdims=True, dtype=F) / F(x.shape[1]) + F(EPS))
        assert rstd[-1, 0] == F(1.0) / np.sqrt(F(EPS)) and np.isfinite(rstd).all()
        prod = d * rstd * case["gamma"].numpy()                                               # +-0, finite
        assert (prod == 0).all()
        y_mul_add = prod + b                                                                  # two roundings
        y_fma = (prod.astype(np.float64) + b.astype(np.float64)).astype(F)                    # one rounding (the sum is exact in fp64)
        nz = b != 0
        assert (y_mul_add.view(np.uint32) == np.broadcast_to(b, prod.shape).view(np.uint32))[:, nz].all()
        assert (y_fma.view(np.uint32) == np.broadcast_to(b, prod.shape).view(np.uint32))[:, nz].all()
        assert (y_mul_add[:, ~nz] == 0).all() and (y_fma[:, ~nz] == 0).all()
    cover = np.concatenate([c["beta"].numpy()[:-2] for c in f8.exact_rows(512, k)]) / two_k
    assert set(cover.view(np.uint32).tolist()) == set(v.view(np.uint32).tolist())              # all 1010 values are laid out


@pytest.mark.parametrize("C", f8.EXACT_C)
@pytest.mark.parametrize("k", f8.EXACT_K)
def test_exact_tier_on_emulation(C, k):
    """The emulation gives the expected byte for every decision value and the scale 2^k bit for bit; round-half-away and truncation do not."""
    seen = set()
    for case in f8.exact_rows(C, k):
        codes, S = f8.ln8_emulate(case["x"], case["gamma"], case["beta"], EPS)
        assert (S == 2.0 ** k).all()
        bad, z, _ = f8.exact_mismatch(codes, case)
        assert not bad.any()
        seen |= z
        for mutation in ("round-half-away", "truncation"):
            bad = f8.exact_mismatch(f8.ln8_emulate(case["x"], case["gamma"], case["beta"], EPS, **f8.MUTATIONS[mutation])[0], case)[0]
            assert bad.any(), mutation
    assert seen == {0x80}                                        # the emulation keeps the sign of a value that rounds to zero


def test_exact_mismatch_compares_bytes():
    case = f8.exact_rows(1024, 0)[0]
    codes, _ = f8.ln8_emulate(case["x"], case["gamma"], case["beta"], EPS)
    negz = int(torch.nonzero(case["zero"] & case["negative"])[0])
    codes[1, negz] = 0x00                                        # a negative zero may lose its sign
    assert not f8.exact_mismatch(codes, case)[0].any()
    codes[1, negz] = 0x01
    assert f8.exact_mismatch(codes, case)[0].sum() == 1
    posz = int(torch.nonzero(case["zero"] & ~case["negative"])[0])
    codes[1, negz], codes[2, posz] = 0x80, 0x80                  # a positive zero may not gain one
    assert f8.exact_mismatch(codes, case)[0].sum() == 1


# ---- random tier on the emulation -------------------------------------------------------------------------------------------------------
def _recipes():
    """Every (name, x, gamma, beta) the GPU tests gate: test_f8gate_gpu.py's random tier and the launches of test_ops_gpu.py::
    test_layernorm_f8 and test_edges_gpu.py::test_layernorm_f8_padding (x = randn 2 + 0.3, plain gamma and beta)."""
    yield from f8.random_tier()
    g = torch.Generator().manual_seed(8)                         # test_layernorm_f8's own operands, drawn in its order
    for rows, C in ((300, 320), (64, 1280), (17, 640)):
        x = (torch.randn(rows, C, generator=g) * 2 + 0.3).half()
        yield f"test_layernorm_f8 {rows}x{C}", x, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    for rows, C in [(r, c) for r in (1, 5, 257) for c in (16, 64, 320, 2048)]:      # test_layernorm_f8_padding's own operands
        g = torch.Generator().manual_seed(rows * 3 + C)
        x = (torch.randn(rows, C, generator=g) * 2 + 0.3).half()
        yield f"test_layernorm_f8_padding {rows}x{C}", x, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


RECIPES = list(_recipes())


@pytest.mark.parametrize("case", RECIPES, ids=[r[0] for r in RECIPES])
def test_gate_accepts_emulation_under_the_cap(case):
    what, x, gamma, beta = case
    codes, S = f8.ln8_emulate(x, gamma, beta, EPS)
    g = f8.ln8_gate(codes, S, x, gamma, beta, EPS, what)
    print(g.line())
    assert g.ambiguous <= f8.CAP and g.scale_ratio <= 1.0
    assert g.off_nearest <= g.ambiguous                          # a code off the nearest one is an ambiguous element


def _mutant(name, rows, C, seed=100, **kw):
    x, gamma, beta = f8.random_case(rows, C, seed, **kw)
    codes, S = f8.ln8_emulate(x, gamma, beta, EPS, **f8.MUTATIONS[name])
    return f8.ln8_gate(codes, S, x, gamma, beta, EPS, name, check=False)


@pytest.mark.parametrize("name,rows,C", [(n, r, c) for n in ("truncation", "FNUZ encoding", "scale before beta", "variance / (C - 1)")
                                         for r, c in ((33, 320), (6, 1040))]
                         + [("amax over the first 512 columns", 6, 1040), ("amax over the first 512 columns", 5, 2048), ("no saturation", 4000, 16)])
def test_gate_1_rejects(name, rows, C):
    """'amax over the first 512 columns' is the kernel itself at C <= 512.  'no saturation' (a product above 448 becomes NaN) differs from
    the kernel only where fl32(y * inv) exceeds 448 by an ulp, about one row in a thousand: hence 4000 rows of 16."""
    g = _mutant(name, rows, C)
    print(g.line(), g.failed)
    assert any(k.startswith("gate 1") for k in g.failed), (name, g.failed)
    with pytest.raises(AssertionError, match="gate 1"):
        g.check()
    if name == "truncation":
        assert g.off_nearest > 0.3                               # about half of all elements
    if name == "no saturation":
        assert "gate 1 (NaN code)" in g.failed


@pytest.mark.parametrize("rows,C", [(33, 320), (6, 1040), (5, 2048)])
def test_gate_2_rejects_a_reported_scale_that_is_not_the_one_used(rows, C):
    g = _mutant("reported scale off by 2^-9", rows, C)
    print(g.line(), g.failed)
    assert "gate 2 (scale)" in g.failed and g.scale_ratio > 10
    with pytest.raises(AssertionError, match=r"gate 2 \(scale\)"):
        g.check()


def test_random_tier_lets_round_half_away_through():
    """An exact tie of the fp32 product is too rare for random operands to meet: only the exact tier tells round-half-away from
    round-half-even (test_exact_tier_on_emulation)."""
    for rows, C in ((33, 320), (6, 1040)):
        assert not _mutant("round-half-away", rows, C).failed


def test_gate_3_and_nan_codes():
    x, gamma, beta = f8.random_case(9, 512, 5)
    codes, S = f8.ln8_emulate(x, gamma, beta, EPS)
    top = (codes & 0x7F) == 0x7E
    low = codes.clone()
    low[2][top[2]] -= 1                                          # row 2 never reaches 448
    g = f8.ln8_gate(low, S, x, gamma, beta, EPS, check=False)
    assert "gate 3 (row maximum)" in g.failed and "gate 1 (admissible interval)" in g.failed
    nan = codes.clone()
    nan[4, 7] = 0xFF
    assert "gate 1 (NaN code)" in f8.ln8_gate(nan, S, x, gamma, beta, EPS, check=False).failed
    for s in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        bad = S.clone()
        bad[1] = s
        assert "gate 2 (scale not finite, normal and positive)" in f8.ln8_gate(codes, bad, x, gamma, beta, EPS, check=False).failed


def test_cap_is_a_condition():
    """A case whose elements mostly sit on rounding boundaries is refused as a case, whatever the codes are."""
    x = torch.zeros(4, 64, dtype=torch.float16)
    x[:, 0] = 1.0
    gamma, beta = torch.zeros(64), torch.full((64,), 17.0)      # every element at the tie 17 of a row whose maximum is 448
    beta[0] = 448.0
    codes, S = f8.ln8_emulate(x, gamma, beta, EPS)
    g = f8.ln8_gate(codes, S, x, gamma, beta, EPS, check=False)
    assert list(g.failed) == ["cap"] and g.ambiguous > 0.9
    with pytest.raises(AssertionError, match="exceeds the cap of 2 %"):
        g.check()


def test_tiny_rows_need_the_scale_floor():
    """gamma = 0, beta = +-1e-39: amax / 448 is below 448 2^-128, so without the floor the scale is not a normal number and 1 / scale
    overflows (inf where subnormals are kept, and y * inf is NaN where they are flushed)."""
    x, gamma, beta = f8.tiny_case()
    codes, S = f8.ln8_emulate(x, gamma, beta, EPS, floor=None)
    assert (S < f8.F32_MIN_NORMAL).all() and torch.isinf(1.0 / S).all()      # subnormal where kept, zero where flushed: 1 / S overflows
    codes, S = f8.ln8_emulate(x, gamma, beta, EPS)
    f8.tiny_check(codes, S, beta)
    assert (S == f8.SCALE_FLOOR).all()
    # the floor changes no row that does not need it
    x, gamma, beta = f8.random_case(9, 528, 3)
    a, b = f8.ln8_emulate(x, gamma, beta, EPS), f8.ln8_emulate(x, gamma, beta, EPS, floor=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- ops.pack_linear_f8 -----------------------------------------------------------------------------------------------------------------
def _pack_cases():
    g = torch.Generator().manual_seed(11)
    yield "random", torch.randn(48, 320, generator=g) / 18
    w = torch.randn(16, 640, generator=g) / 25
    w[torch.arange(16), torch.randint(0, 640, (16,), generator=g)] = 37.5
    yield "one outlier per row", w
    w = torch.randn(8, 64, generator=g)
    w[3] = 0
    yield "an all-zero row", w
    w = torch.randn(8, 64, generator=g)
    w[5] = torch.randn(64, generator=g) * 1e-40
    assert (w[5] != 0).any() and (w[5].abs() < 2.0 ** -126).all()
    yield "a row of fp32 denormals", w
    w = torch.randn(8, 64, generator=g)
    w[2, 9] = -7.25
    yield "maximum at a negative entry", w


@pytest.mark.parametrize("case", list(_pack_cases()), ids=[c[0] for c in _pack_cases()])
def test_pack_linear_f8(case):
    from pbe_amd import ops
    what, w = case
    w8, scale = ops.pack_linear_f8(w)
    g = f8.pack_gate(w, w8, scale, what)
    print(g.line())
    assert ((w8 & 0x7F) != 0x7F).all()
    if what == "an all-zero row":
        assert scale[3] == 1.0 and (w8[3] == 0).all()
    if what == "a row of fp32 denormals":
        assert scale[5] == f8.SCALE_FLOOR and ((w8[5] & 0x7F) == 0).all()
    if what == "maximum at a negative entry":
        assert w8[2, 9] == 0xFE
    w4 = torch.randn(6, 4, 3, 3)                                  # a conv weight packs as [N, K]
    w8, scale = ops.pack_linear_f8(w4)
    assert w8.shape == (6, 36) and w8.dtype == torch.uint8 and w8.is_contiguous() and scale.shape == (6,) and scale.dtype == torch.float32


def test_pack_gate_rejects_planted_faults():
    from pbe_amd import ops
    w = torch.randn(16, 320, generator=torch.Generator().manual_seed(2))
    w8, scale = ops.pack_linear_f8(w)
    assert "scale" in f8.pack_gate(w, w8, scale * (1 + 2.0 ** -20), check=False).failed
    trunc = f8.encode(f8.q_e4m3(w.double() / scale.double()[:, None], "trunc"))
    assert "gate 1 (admissible interval)" in f8.pack_gate(w, trunc, scale, check=False).failed
    assert "codes layout" in f8.pack_gate(w, w8.t().contiguous().t(), scale, check=False).failed
