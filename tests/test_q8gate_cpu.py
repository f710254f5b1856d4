"""The quantisation-aware gate of the fp8 block paths (tests/q8ref.py) on the CPU: the pins of its references, the emulation under its
own verdict on every case test_q8gate_gpu.py runs, and the planted wiring faults the verdict must reject - with, for each, whether the
whole-tensor limit against the PLAIN reference (FP8_FWD_TOL 5e-2 / BOTH8_FWD_TOL 7e-2 / ATTN8_FWD_TOL 8.5e-3) would have accepted it.
The printed lines (pytest -s) are the CPU half of profiles/q8gate_report.txt; PBE_Q8_REPORT=<file> appends them there."""
import os

import numpy as np
import pytest
import torch

import block_cases as bc
import f8ref
import mx8ref
import q8ref as Q
from oracle_loader import O


def report(line):
    print(line)
    path = os.environ.get("PBE_Q8_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- pins ---------------------------------------------------------------------------------------------------------------------------------
def test_plain_is_the_oracles_spatial_transformer():
    """plain() (fp64) against oracle/pbe_oracle.py's spatial_transformer (fp32, one block): rel-L2 <= 1e-5, at N = 64 and N = 25."""
    for grid in (8, 5):
        r = Q.refs(grid)
        sd1 = {k: v for k, v in r.sd.items() if not k.startswith("transformer_blocks.1.")}
        want = O.spatial_transformer(sd1, "", r.x.float().permute(0, 3, 1, 2).contiguous(), r.context.float(), bc.HEADS).permute(0, 2, 3, 1)
        got = Q.plain(sd1, r.x, r.context, bc.HEADS)
        rel = Q.rel_l2(want, got)
        assert rel <= 1e-5, (grid, rel)
        assert Q.rel_l2(r.plain(), got) > 1e-2                      # the second block of the fixture is really there


def test_row_quantisers_restate_f8ref_and_the_pack_byte_for_byte():
    g = torch.Generator().manual_seed(5)
    # the fp8 LayerNorm: codes and scales of f8ref.ln8_emulate
    for name, x, gamma, beta in list(f8ref.random_tier())[:4]:
        codes, S = f8ref.ln8_emulate(x, gamma, beta, 1e-5)
        y8, s = Q.ln8(x.float(), gamma.float(), beta.float(), 1e-5)
        assert torch.equal(f8ref.encode(y8.double()), codes), name
        assert torch.equal(s.view(-1), S), name
    # the weight pack: the bytes and scales of ops.pack_linear_f8 (host code: torch converts), which f8ref.pack_gate admits
    from pbe_amd import ops
    w = torch.randn(96, 320, generator=g) / 320 ** 0.5
    w[3] = 0.0                                                       # an all-zero row: scale 1
    w[5] *= 2.0 ** -110                                              # below the floor
    w8, sc = ops.pack_linear_f8(w)
    q, s = Q.pack_f8(w)
    assert torch.equal(f8ref.encode(q.double()), w8) and torch.equal(s, sc)
    f8ref.pack_gate(w, f8ref.encode(q.double()), s)
    # the exact fp64 rule on the same fp32 values: within pack_gate's admissible set too, scale 1 for the zero row, the floor
    q64, s64 = Q.quant_rows(w.double())
    f8ref.pack_gate(w, f8ref.encode(q64), s64.view(-1).float())
    assert s64[3].item() == 1.0 and s64[5].item() == Q.SCALE_FLOOR
    assert bool((q64.abs().amax(1)[torch.arange(96) != 3][:2] == 448.0).all())


@pytest.mark.parametrize("D,N", [(40, 64), (40, 25), (80, 130)])
def test_mx_quantiser_restates_mx8ref_byte_for_byte(D, N):
    B, H = 2, 3
    g = torch.Generator().manual_seed(D + N)
    x = (torch.randn(B * N, H * D, generator=g) * 3).half()
    x[1, :32] = 0.0                                                  # an all-zero block
    x[2, 0] = 3000.0
    x[3, :32] = 448.0 * 2.0 ** -3                                    # amax exactly 448 2^k: the boundary of the scale rule
    x[4, :32] = 464.0
    for alpha in (1.0, 0.25):                                        # (a power of two: alpha x is exact in fp32 and fp64 alike)
        codes, scales = mx8ref.quant_tokens(x.numpy(), B, H, N, D, alpha)
        q, s = Q.mx_quant((x.double() * alpha).view(B * N, H, D))
        DP = (D + 63) // 64 * 64
        want = codes.reshape(B * N, H, DP)[:, :, :q.shape[-1]]
        assert np.array_equal(f8ref.encode(q).numpy() & 0x7F, want & 0x7F)            # (mx8ref emits +0 for a negative value that rounds to zero)
        assert np.array_equal((f8ref.encode(q).numpy() >> 7)[want & 0x7F != 0], (want >> 7)[want & 0x7F != 0])
        se = scales[:, :, :s.shape[-1], :N].transpose(0, 3, 1, 2).reshape(B * N, H, -1)
        assert np.array_equal(torch.log2(s).numpy() + 127, se.astype(np.float64))
    # V^T: blocks along the tokens
    vt = (torch.randn(B * H * D, (N + 7) // 8 * 8, generator=g) * 2).half()
    vt[:, N:] = 0.0
    codes, scales = mx8ref.quant_vt(vt.numpy(), B, H, N, D)
    q, s = Q.mx_quant(vt[:, :N].double())
    want = codes[:, :q.shape[-1]]
    nz = want & 0x7F != 0
    assert np.array_equal(f8ref.encode(q).numpy() & 0x7F, want & 0x7F) and np.array_equal((f8ref.encode(q).numpy() >> 7)[nz], (want >> 7)[nz])
    se = scales[:, :, :s.shape[-1], :D].transpose(0, 1, 3, 2).reshape(B * H * D, -1)
    assert np.array_equal(torch.log2(s).numpy() + 127, se.astype(np.float64))


# ---- the emulation under its own verdict ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", Q.GRIDS)
def test_emulation_passes_its_own_verdict(grid):
    r = Q.refs(grid)
    for name, sw, mode in Q.CASES:
        path = Q.path_of(mode, grid * grid, sw.get("fold_layernorm", True))
        emu = r.emu(mode, path)
        ok, text = r.verdict(emu, mode, path)
        report(f"q8gate cpu  {name + f'-{grid}x{grid}':22s} {path:6s} emulation: {text}")
        assert ok, (name, grid, text)
        if mode is not None:                                         # the quantisation is really there, and is the larger part of the error
            assert Q.rel_l2(r.q64(mode), r.plain()) > 1e-3
        if grid == 8 and name == "attnf8-proj":                      # the MX copy-out is the same arithmetic
            assert Q.emulate(mode, path, r.sd, r.x, r.context, bc.HEADS, copy_out=True).equal(emu)


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
REBLOCK = {"MX blocks of 64": dict(block=64), "V^T blocked along d": dict(vt_along_d=True)}
MUST_PASS_OLD = ("one A scale for all rows", "weights truncated")    # the gap this gate closes: the old limits accept them


@pytest.mark.parametrize("fault", list(Q.FAULTS))
def test_planted_fault_is_rejected(fault):
    grid = 8
    r = Q.refs(grid)
    for mode in Q.FAULTS[fault][0]:
        path = Q.path_of(mode, grid * grid)
        bad = r.emu(mode, path, fault)
        ok, text = r.verdict(bad, mode, path)
        old = Q.rel_l2(bad, r.plain())
        old_ok = old <= Q.OLD_FWD_TOL[mode]
        ratio = Q.rel_l2(bad, r.q64(mode)) / Q.rel_l2(r.emu(mode, path), r.q64(mode))
        report(f"q8gate cpu  fault {fault!r:28s} {mode:9s} {'REJECTED' if not ok else 'accepted'} ({ratio:5.1f} x the emulation); "
               f"vs plain {old:.3e}: the old limit {Q.OLD_FWD_TOL[mode]:.1e} {'ACCEPTS' if old_ok else 'rejects'} it; {text}")
        assert not ok, (fault, mode, text)
        if fault in MUST_PASS_OLD:
            assert old_ok, (fault, mode, old)
        if fault in REBLOCK:
            # The same geometry used CONSISTENTLY by quantiser and core is no fault of value: a power-of-two scale only moves the e4m3
            # exponent, so short of the subnormal range every dequantised operand is the same number.  Hence the two geometry faults are
            # planted as a producer / consumer mismatch (q8ref.attention_mx8_emulate); the consistent form is reported, not asserted.
            same = Q.emulate(mode, path, r.sd, r.x, r.context, bc.HEADS, reblock=REBLOCK[fault])
            report(f"q8gate cpu        {fault!r:28s} {mode:9s} as a CONSISTENT other geometry: {Q.rel_l2(same, r.q64(mode)) / Q.rel_l2(r.emu(mode, path), r.q64(mode)):5.2f}"
                   f" x the emulation, {int((same != r.emu(mode, path)).sum())} of {same.numel()} outputs differ (value-neutral: not a fault the values can show)")
