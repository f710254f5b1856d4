"""pbe_layernorm_f8 (layernorm_f8_kernel<1..4>, pbe_amd/csrc/norm.hip) code by code on the GPU, against tests/f8ref.py (the gate and its
derivation stand there; tests/test_f8gate_cpu.py shows it rejecting every planted fault and asserts the cap for every recipe used here).

exact tier: gamma = 0 and power-of-two scales make the kernel's arithmetic exact, so every byte of all 1010 decision values and the
scale's bit pattern are compared.  random tier: every code inside its admissible interval, the scale within its bound, 448 in every row,
at most 2 % of the elements ambiguous.  Degenerate rows: all zero, a maximum at both signs, and a row below the scale floor.

Every case appends one line (ambiguous share, share off the nearest code, scale ratio, worst element) to the accuracy report beside the
parity report, as tests/test_accuracy_gpu.py does."""
import pytest
import torch

import f8ref as f8
import guard
from test_accuracy_gpu import report

pytestmark = pytest.mark.gpu
EPS = 1e-5
TIER = list(f8.random_tier())


def _launch(dev, x, gamma, beta):
    from pbe_amd import ops
    codes, S = ops.layernorm_f8(x.to(dev), gamma.to(dev), beta.to(dev), EPS)
    return codes.cpu(), S.cpu()


@pytest.mark.parametrize("C", f8.EXACT_C)
@pytest.mark.parametrize("k", f8.EXACT_K)
def test_exact_tier(dev, C, k):
    """Byte equality on every decision value, in every row (random rows and the constant one), and S == 2^k bit for bit."""
    seen, seen0, n = set(), set(), 0
    for j, case in enumerate(f8.exact_rows(C, k)):
        codes, S = _launch(dev, case["x"], case["gamma"], case["beta"])
        bad, z, z0 = f8.exact_mismatch(codes, case)
        seen |= z
        seen0 |= z0
        n += codes.numel()
        s_ok = S.view(torch.int32) == torch.tensor(2.0 ** k, dtype=torch.float32).view(torch.int32)
        assert s_ok.all(), f"C {C} k {k} launch {j}: scale {S.tolist()} is not 2^{k}"
        if bad.any():
            r, c = torch.nonzero(bad)[0].tolist()
            v = case["beta"][c].item() * 2.0 ** -k
            raise AssertionError(f"C {C} k {k} launch {j}: {int(bad.sum())} bytes differ, first at row {r}, column {c}: value {v!r} ({v.hex()}) "
                                 f"became {int(codes[r, c]):#04x}, want {int(case['want'][c]):#04x}")
    fmt = lambda b: " and ".join(f"{c:#04x}" for c in sorted(b))
    report(f"f8gate exact C {C:4d} k {k:2d}: {n} bytes equal, scale == 2^k bit for bit; a negative value that rounds to zero is emitted as "
           f"{fmt(seen)}, -0 itself (its sign in y is that of x - mean) as {fmt(seen0)}")


@pytest.mark.parametrize("case", TIER[:-1], ids=[c[0] for c in TIER[:-1]])
def test_random_tier(dev, case):
    what, x, gamma, beta = case
    codes, S = _launch(dev, x, gamma, beta)
    g = f8.ln8_gate(codes, S, x, gamma, beta, EPS, what, check=False)
    report(g.line())
    print(g.line())
    g.check()


def test_random_tier_strided(dev):
    """One raw launch with ldx = C + 8 and ldy = C + 16 between poison and sentinels: the same gate, nothing outside the output written,
    the bits of the contiguous launch."""
    from pbe_amd import lib
    what, x, gamma, beta = TIER[-1]
    rows, C = x.shape
    xv, _ = guard.embed(x, row_pad=1, col_pad=8, device=dev)
    gv, bv = guard.embed(gamma, device=dev)[0], guard.embed(beta, device=dev)[0]
    y, arena = guard.sentinel_out((rows, C), row_pad=1, col_pad=16, dtype=torch.uint8, device=dev)
    sc, sarena = guard.sentinel_out((rows,), dtype=torch.float32, device=dev)
    assert xv.stride(0) == C + 8 and y.stride(0) == C + 16
    lib.check(lib.load().pbe_layernorm_f8(xv.data_ptr(), gv.data_ptr(), bv.data_ptr(), y.data_ptr(), sc.data_ptr(), rows, C, xv.stride(0), y.stride(0),
                                          EPS, torch.cuda.current_stream().cuda_stream), "layernorm_f8")
    guard.assert_untouched(arena, y, "layernorm_f8 Y")
    guard.assert_untouched(sarena, sc, "layernorm_f8 row_scale")
    g = f8.ln8_gate(y.cpu(), sc.cpu(), x, gamma, beta, EPS, what + " ldx C+8 ldy C+16", check=False)
    report(g.line())
    g.check()
    codes, S = _launch(dev, x, gamma, beta)
    assert torch.equal(codes, y.cpu()) and torch.equal(S.view(torch.int32), sc.cpu().view(torch.int32))


def test_degenerate_rows(dev):
    C = 64
    x = (torch.randn(5, C, generator=torch.Generator().manual_seed(4)) * 1.5 + 0.3).half()
    codes, S = _launch(dev, x, torch.zeros(C), torch.zeros(C))
    assert (codes == 0).all() and (S == 1.0).all(), "gamma = beta = 0: all codes 0 and S == 1"
    beta = 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(5))
    beta[3], beta[40] = 0.75, -0.75                              # the maximum, attained at both signs
    codes, S = _launch(dev, x, torch.zeros(C), beta)
    assert (codes[:, 3] == 0x7E).all() and (codes[:, 40] == 0xFE).all()
    g = f8.ln8_gate(codes, S, x, torch.zeros(C), beta, EPS, "maximum at both signs 5x64", check=False)
    report(g.line())
    g.check()


def test_row_below_the_scale_floor(dev):
    """gamma = 0, beta = +-1e-39 at C = 32: max|y| / 448 is below 448 2^-128 and 1 / scale would overflow.  Required: no NaN code, S finite,
    normal and positive, |y8 S - y| <= S 2^-10 + dy (f8ref.tiny_check)."""
    x, gamma, beta = f8.tiny_case()
    codes, S = _launch(dev, x, gamma, beta)
    report(f"f8gate row below the scale floor 3x32: S {S.tolist()}, codes {sorted(set(codes.view(-1).tolist()))}")
    f8.tiny_check(codes, S, beta)
