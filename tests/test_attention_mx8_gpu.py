"""MX-fp8 attention core (pbe_quant_mx8_f16 + pbe_attention_mx8, pbe_amd.precision.set_attention_precision).

Quantiser: bit for bit against the host reference (tests/mx8ref.py).  Kernel: (1) exact integer data pins the operand lane maps, the
scale bytes and the P-register -> key permutation; (2) random data against an fp64 reference computed from the DEQUANTISED operands,
with a per-element bound from the rounding model below; (3) the deferred-maximum branches; (4) determinism; (5) the U-Net forward.

Rounding model of the kernel on dequantised operands (what the reference does not see):
  * P = exp2(s - m) is rounded to e4m3 once: |dP_j| <= max(2^-4 P_j, 2^-10) (3 mantissa bits; quantum 2^-9 below 2^-6).  The same
    rounded P feeds the numerator and the denominator (the ones row of V^T), so with w = softmax weights and Z = sum_j 2^(s_j - smax)
    (m <= smax, hence sum P >= Z):  |dO| <= sum_j max(2^-4 w_j, 2^-10 / Z) |v_j - O| / (1 - 2^-4)
    and |v_j - O| <= |v_j| + |O| keeps it a pair of matrix products;
  * scores accumulated in fp32 (2^-22 sum |q k| log2 units -> relative ln 2 of that on P), PV in fp32 (2^-20 sum w |v|);
  * O stored as fp16: 2^-11 |O| + 2^-24.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx8ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634
REPORT = os.environ.get("PBE_MX8_REPORT")          # optional: append the measured rel-L2 / bound ratios to this file


def report(line):
    if not REPORT:
        return
    os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _quant(x, B, H, N, D, dev, *, vt=False, alpha=1.0, rs=None):
    from pbe_amd import ops
    xd = x.to(dev)
    return ops.quant_mx8(xd, B, H, N, D, rs=rs if rs is not None else x.shape[-1], vt=vt, alpha=alpha)


def _deq(m8):
    f = R.dequant_vt if m8.vt else R.dequant_tokens
    return f(m8.data.cpu().numpy(), m8.scale.cpu().numpy(), m8.B, m8.H, m8.N, m8.D)


class _M8:
    def __init__(self, t, vt):
        self.data, self.scale, self.B, self.H, self.N, self.D, self.vt = t.data, t.scale, t.B, t.H, t.N, t.D, vt


# ---- quantiser ----------------------------------------------------------------------------------------------------------------------
def _adversarial_rows(rows, width, g):
    x = torch.randn(rows, width, generator=g) * 3
    blocks = x.view(rows, -1)
    for r in range(rows):
        kind = r % 6
        if kind == 1:                                       # one outlier per 32 (scale set by it, the rest near / under the subnormal range)
            blocks[r, ::32] = 3000.0 * (1 if r % 12 == 1 else -1)
        elif kind == 2:                                     # exact e4m3 ties at scale 1 (amax 448): 1.0625 -> 1, 1.1875 -> 1.25, 17 -> 16, 3 * 2^-10 -> 2^-8
            vals = torch.tensor([448.0, 1.0625, 1.1875, 17.0, 3 * 2.0 ** -10, 2.0 ** -10, 5 * 2.0 ** -11, -1.0625, -17.0, 240.0, 464.0 - 16])
            blocks[r] = vals.repeat(width // len(vals) + 1)[:width]
        elif kind == 3:                                     # fp16 subnormals and tiny values
            blocks[r] = torch.randn(width, generator=g) * 2.0 ** -20
        elif kind == 4:
            blocks[r] = 0.0                                  # all-zero blocks
    return x.half()


@pytest.mark.parametrize("D", [40, 80, 160])
def test_quant_tokens_bit_exact(dev, D):
    B, H, N = 2, 3, 130
    g = _g(D)
    rs = 2 * H * D                                          # a q | k slice of the projection output
    full = torch.cat([_adversarial_rows(B * N, H * D, g), torch.randn(B * N, H * D, generator=g).half()], 1)
    for alpha, col0 in ((1.0, 0), (D ** -0.5 * LOG2E, 0), (1.0, H * D)):
        src = full.to(dev)[:, col0:]
        from pbe_amd import ops
        got = ops.quant_mx8(src, B, H, N, D, rs=rs, alpha=alpha)
        ref_c, ref_s = R.quant_tokens(full[:, col0:col0 + H * D].numpy(), B, H, N, D, alpha)
        gc, gs = got.data.cpu().numpy(), got.scale.cpu().numpy()
        assert np.array_equal(gs, ref_s), f"D={D} alpha={alpha}: {(gs != ref_s).sum()} scale bytes differ"
        assert np.array_equal(gc, ref_c), f"D={D} alpha={alpha}: {(gc != ref_c).sum()} data bytes differ"
        DP = (D + 63) // 64 * 64
        assert not gc.reshape(B * N, H, DP)[:, :, D:].any()           # head padding is zero
        assert (gs[:, :, :, N:] == 127).all()                          # token padding scales are 1.0
        assert not ((gc & 0x7F) == 0x7F).any()                         # never NaN


@pytest.mark.parametrize("D", [40, 80, 160])
def test_quant_vt_bit_exact(dev, D):
    B, H = 2, 2
    g = _g(100 + D)
    for N in (330, 256):
        npad = (N + 7) // 8 * 8
        x = torch.zeros(B * H * D, npad, dtype=torch.float16)
        x[:, :N] = torch.cat([_adversarial_rows(B * H * D, 128, g).float(), torch.randn(B * H * D, N - 128, generator=g) * 5], 1).half()
        from pbe_amd import ops
        got = ops.quant_mx8(x.to(dev), B, H, N, D, rs=npad, vt=True)
        ref_c, ref_s = R.quant_vt(x.numpy(), B, H, N, D)
        gc, gs = got.data.cpu().numpy(), got.scale.cpu().numpy()
        assert np.array_equal(gs, ref_s), f"D={D} N={N}: {(gs != ref_s).sum()} scale bytes differ"
        assert np.array_equal(gc, ref_c), f"D={D} N={N}: {(gc != ref_c).sum()} data bytes differ"
        assert not gc[:, N:].any()                                      # key padding is zero
        assert (gs[:, :, :, D:] == 127).all()


# ---- the kernel on exact data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [40, 80, 160])
def test_layout_pinning_exact_integers(dev, D):
    """q: one nonzero 2^a (a in {0, 1}) per head at a random channel; k: {0, +-1} x 2^b (b in {0, 1}) per (token, 32-channel block),
    key 0 = 2 everywhere (the maximum of every query, in the first tile: no raise); v: integers in [-4, 4] x 2^e, e in [-2, 2] per (channel,
    32-key block).  Every score is an integer, every P = 2^(s - smax) in [2^-8, 1] is exact in e4m3, every scale differs by block, token
    and channel, and the fp32 sums are exact: O must equal the fp64 result up to the fp16 rounding of O."""
    from pbe_amd import ops
    B, H, N = 1, 2, 256
    g = _g(7 * D)
    q = torch.zeros(B * N, H, D)
    a = torch.randint(0, 2, (B * N, H), generator=g).float()
    dsel = torch.randint(0, D, (B * N, H), generator=g)
    q.scatter_(2, dsel[..., None], (2.0 ** a)[..., None])
    nb = (D + 31) // 32
    bexp = torch.randint(0, 2, (B * N, H, nb), generator=g).float()
    kscale = (2.0 ** bexp).repeat_interleave(32, 2)[:, :, :D]
    k = torch.randint(-1, 2, (B * N, H, D), generator=g).float() * kscale
    k[0] = 2.0
    vexp = torch.randint(-2, 3, (H * D, N // 32), generator=g).float()
    v_t = torch.randint(-4, 5, (B * H * D, N), generator=g).float() * (2.0 ** vexp).repeat_interleave(32, 1)
    q8 = _quant(q.reshape(B * N, H * D).half(), B, H, N, D, dev)
    k8 = _quant(k.reshape(B * N, H * D).half(), B, H, N, D, dev)
    v8 = _quant(v_t.half(), B, H, N, D, dev, vt=True)
    got = ops.attention_mx8(q8, k8, v8, 1.0).float().cpu().double()
    s = torch.einsum("nhd,mhd->hnm", q.double(), k.double())             # integers
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    assert bool((p >= 2.0 ** -8).all())
    v = v_t.double().view(H, D, N)
    ref = torch.einsum("hnm,hdm->nhd", p, v) / p.sum(-1).T[..., None]
    ref = ref.reshape(B, N, H * D)
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14)))) * 2.0 ** -10
    err = (got - ref).abs()
    assert bool((err <= 0.5 * ulp * (1 + 2.0 ** -8) + 2.0 ** -24).all()), f"D={D}: max err {err.max():.3e} ({int((err > ulp).sum())} elements > 1 ulp)"
    # the same with the scale-1 data spread over other scale bytes: all of q scaled by 2^3, all of v by 2^-3 (outputs scale exactly)
    q8b = _quant((q.reshape(B * N, H * D) * 8).half(), B, H, N, D, dev)
    got2 = ops.attention_mx8(q8b, k8, v8, 0.125).float().cpu().double()
    assert torch.equal(got2, got)


def _reference(q8, k8, v8, scale_log2e):
    """fp64 softmax(q k^T) v of the dequantised operands and the per-element bound of the module docstring."""
    qd = torch.from_numpy(_deq(q8))
    kd = torch.from_numpy(_deq(k8))
    vd = torch.from_numpy(_deq(v8))
    dev = q8.data.device
    qd, kd, vd = qd.to(dev), kd.to(dev), vd.to(dev)
    s = (qd @ kd.transpose(-1, -2)) * scale_log2e                     # log2 units, [B, H, Nq, Nk]
    sabs = (qd.abs() @ kd.abs().transpose(-1, -2)) * scale_log2e
    smax = s.max(-1, keepdim=True).values
    e = torch.exp2(s - smax)
    Z = e.sum(-1, keepdim=True)
    w = e / Z
    o = w @ vd
    c = torch.maximum(w * 2.0 ** -4, 2.0 ** -10 / Z) / (1 - 2.0 ** -4) + w * math.log(2) * 2.0 ** -22 * sabs
    bound = c @ vd.abs() + o.abs() * c.sum(-1, keepdim=True) + 2.0 ** -20 * (w @ vd.abs())
    bound = bound + o.abs() * 2.0 ** -11 + 2.0 ** -24
    B, H, Nq, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * D), bound.permute(0, 2, 1, 3).reshape(B, Nq, H * D)


def _check(got, ref, bound, what):
    got = got.to(ref.device).double()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    report(f"{what:60s} rel_l2={rel:.3e} max err/bound={ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} x the bound (rel-L2 {rel:.3e})"
    return rel


def _run(q, k, vt_rows, B, H, Nq, Nk, D, dev, *, q_rs=None, k_rs=None, scale=None):
    from pbe_amd import ops
    scale = D ** -0.5 if scale is None else scale
    q8 = ops.quant_mx8(q, B, H, Nq, D, rs=q_rs or q.shape[-1], alpha=scale * LOG2E)
    k8 = ops.quant_mx8(k, B, H, Nk, D, rs=k_rs or k.shape[-1])
    v8 = ops.quant_mx8(vt_rows, B, H, Nk, D, rs=vt_rows.shape[-1], vt=True)
    got = ops.attention_mx8(q8, k8, v8, 1.0)
    ref, bound = _reference(_M8(q8, False), _M8(k8, False), _M8(v8, True), 1.0)
    return got, ref, bound


@pytest.mark.parametrize("D,Nq,Nk,B,H", [(40, 256, 256, 2, 2), (40, 4096, 4096, 1, 2), (40, 1000, 1000, 1, 3), (40, 330, 1024, 2, 1),
                                          (80, 1024, 1024, 2, 2), (80, 330, 330, 1, 2), (80, 256, 1000, 1, 2),
                                          (160, 256, 256, 2, 2), (160, 1024, 330, 1, 2), (160, 1000, 1000, 1, 1)])
def test_accuracy_against_dequantised_fp64(dev, D, Nq, Nk, B, H):
    g = _g(D * 7 + Nq + Nk)
    q = (torch.randn(B * Nq, H * D, generator=g) * 1.5).half().to(dev)
    k = (torch.randn(B * Nk, H * D, generator=g) * 1.5).half().to(dev)
    npad = (Nk + 7) // 8 * 8
    vt = torch.zeros(B * H * D, npad, dtype=torch.float16)
    vt[:, :Nk] = torch.randn(B * H * D, Nk, generator=g).half()
    got, ref, bound = _run(q, k, vt.to(dev), B, H, Nq, Nk, D, dev)
    _check(got, ref, bound, f"accuracy D={D} Nq={Nq} Nk={Nk} B={B} H={H}")


@pytest.mark.parametrize("D", [40, 80, 160])
def test_accuracy_strided_qk_views(dev, D):
    """The U-Net's operands: q and k are column slices of one [B*N, 2*inner] projection output, V^T is [B, inner, npad]."""
    B, H, N = 2, 320 // D if D < 160 else 2, 1024
    inner = H * D
    g = _g(300 + D)
    qk = (torch.randn(B * N, 2 * inner, generator=g) * 1.2).half().to(dev)
    vt = torch.randn(B * inner, N, generator=g).half().to(dev)
    got, ref, bound = _run(qk, qk[:, inner:], vt, B, H, N, N, D, dev, q_rs=2 * inner, k_rs=2 * inner)
    _check(got, ref, bound, f"strided q|k D={D} N={N}")


@pytest.mark.parametrize("D", [40, 80, 160])
@pytest.mark.parametrize("case", ["first_tile_peak", "negative_start_then_jump", "large_logits", "band_below_threshold", "ragged_jump_in_last_tile"])
def test_mx8_deferred_max_paths(dev, D, case):
    """The five inputs of test_ops_gpu.py::test_attention_deferred_max_paths that force each branch of the deferred maximum."""
    B, H, N = 1, 2, 330 if case == "ragged_jump_in_last_tile" else 384
    g = _g(17 + D)
    q = torch.randn(B, N, H * D, generator=g)
    k = torch.randn(B, N, H * D, generator=g)
    v = torch.randn(B, N, H * D, generator=g)
    q4, k4 = q.view(B, N, H, D), k.view(B, N, H, D)
    if case == "first_tile_peak":
        k4[0, 5] = q4[0, 40] * 3.0
        k4[0, 9] = q4[0, 200] * 3.0
    elif case == "negative_start_then_jump":
        k4[0, :64] = -2.5 * torch.sign(q4[0, 100:101]) * torch.ones(64, H, D)
        k4[0, 300] = q4[0, 100] * 4.0
    elif case == "large_logits":
        q4 *= 7.0
        k4 *= 7.0
    elif case == "band_below_threshold":
        for t in range(1, 6):
            k4[0, 64 * t + 3] = q4[0, 7] * (0.25 * t)
    else:
        k4[0, 325] = q4[0, 33] * 4.0
    npad = (N + 7) // 8 * 8
    vt = torch.zeros(B * H * D, npad)
    vt[:, :N] = v[0].T
    got, ref, bound = _run(q.view(B * N, -1).half().to(dev), k.view(B * N, -1).half().to(dev), vt.half().to(dev), B, H, N, N, D, dev)
    _check(got, ref, bound, f"deferred max {case} D={D}")


def test_deterministic_and_rejects_other_head_dims(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    B, H, N, D = 2, 2, 1000, 80
    g = _g(9)
    q = torch.randn(B * N, H * D, generator=g).half().to(dev)
    vt = torch.randn(B * H * D, 1000, generator=g).half().to(dev)
    q8 = ops.quant_mx8(q, B, H, N, D, rs=H * D)
    v8 = ops.quant_mx8(vt, B, H, N, D, rs=1000, vt=True)
    a = ops.attention_mx8(q8, q8, v8, 0.16)
    b = ops.attention_mx8(q8, q8, v8, 0.16)
    assert torch.equal(a, b)
    for Dx in (64, 32, 48):
        x = torch.randn(256, 2 * Dx, generator=g).half().to(dev)
        t8 = ops.quant_mx8(x, 1, 2, 256, Dx, rs=2 * Dx)
        x8 = ops.quant_mx8(torch.randn(2 * Dx, 256, generator=g).half().to(dev), 1, 2, 256, Dx, rs=256, vt=True)
        with pytest.raises(PbeError, match="head dim"):
            ops.attention_mx8(t8, t8, x8, 1.0)
    with pytest.raises(PbeError):
        ops.quant_mx8(q.cpu(), B, H, N, D, rs=H * D)


# ---- the U-Net ------------------------------------------------------------------------------------------------------------------------
# Bound, derived before measuring: the MX-fp8 core rounds q, k, V^T and P to 3 mantissa bits (relative <= 2^-4, rms ~ 2^-4 / sqrt(3) =
# 3.6e-2 per operand).  An attention output mixes these over many keys; the U-Net's residual stream around it (and everything else
# fp16) dilutes them.  Like the fp8 linear path (tests/test_model_gpu.py, FP8_FWD_TOL), the forward must stay within the error of one
# quantised product, 5e-2; with the linear path too, the two independent error sources add in quadrature: 5e-2 * sqrt(2) = 7e-2.
# Measured on MI355X with the name-seeded weights: attention fp8 2.95e-3 against the fp32 golden, 3.06e-3 against the fp16 path (2.85e-3
# for the shared guidance prefix, 2.82e-3 for the 96x96 guidance pair); attention + linear fp8 3.41e-2 against the golden.  The
# attention-only tolerance is therefore tightened to 3x the smallest of those measurements; the combined one keeps the derived 7e-2
# (2.05x its measurement).
ATTN8_FWD_TOL = 8.5e-3
BOTH8_FWD_TOL = 7e-2


@pytest.fixture(scope="module")
def full(dev):
    import modelbuild as build
    with torch.no_grad():
        return build.full_model(dev, parts=("unet",))


class _Count:
    def __init__(self, monkeypatch):
        from pbe_amd import ops
        self.n = {"attention": 0, "attention_mx8": 0}
        for name in self.n:
            fn = getattr(ops, name)

            def wrap(*a, _fn=fn, _name=name, **kw):
                self.n[_name] += 1
                return _fn(*a, **kw)
            monkeypatch.setattr(ops, name, wrap)


def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    assert torch.isfinite(a).all()
    return ((a - b).norm() / b.norm()).item()


def test_full_unet_attention_fp8(dev, golden_dir, full, monkeypatch):
    import cases
    from pbe_amd import ops
    from pbe_amd.precision import set_attention_precision, set_linear_precision
    gold = np.load(os.path.join(golden_dir, "full.npz"))["unet_y"]
    inp = cases.full_inputs()
    x, t, ctx = inp["unet_x"].to(dev), inp["unet_t"].to(dev), inp["unet_ctx"].to(dev)
    with torch.no_grad():
        y16 = full.apply_model(x, t, ctx)
        cnt = _Count(monkeypatch)
        try:
            assert set_attention_precision(full, "fp8") == 16
            ya = full.apply_model(x, t, ctx)
            assert cnt.n == {"attention": 0, "attention_mx8": 16}, cnt.n
            assert set_linear_precision(full, "fp8") == 16
            yb = full.apply_model(x, t, ctx)
            assert cnt.n == {"attention": 0, "attention_mx8": 32}, cnt.n
            yb2 = full.apply_model(x, t, ctx)
            assert torch.equal(yb, yb2)
            set_linear_precision(full, "fp16")
            # the shared guidance prefix (run_paired) of the fp8 core: once per block at batch B
            g = torch.Generator().manual_seed(5)
            xp = torch.randn(2, 9, 64, 64, generator=g).to(dev)
            cp = torch.randn(4, 1, 768, generator=g).to(dev)
            tp = torch.full((4,), 621, dtype=torch.int64, device=dev)
            unet = full.model.diffusion_model
            before = dict(cnt.n)
            pa = unet.forward_nhwc(ops.plms_pack_input(xp[:, :4], xp[:, 4:8], xp[:, 8:], 1), tp, cp, paired=True)
            assert cnt.n["attention_mx8"] - before["attention_mx8"] == 16 and cnt.n["attention"] == 0, cnt.n
        finally:
            set_attention_precision(full, "fp16")
            set_linear_precision(full, "fp16")
        pf = unet.forward_nhwc(ops.plms_pack_input(xp[:, :4], xp[:, 4:8], xp[:, 8:], 1), tp, cp, paired=True)
        y16b = full.apply_model(x, t, ctx)
    assert torch.equal(y16b, y16)                                        # switching back restores the fp16 bits
    ra, rb = _rel(ya, gold), _rel(yb, gold)
    r16 = _rel(ya, y16.float())
    rp = _rel(pa, pf.float())
    report(f"v1 U-Net forward, attention fp8 vs fp32 golden          rel_l2={ra:.3e} tol={ATTN8_FWD_TOL:.1e}")
    report(f"v1 U-Net forward, attention + linear fp8 vs fp32 golden rel_l2={rb:.3e} tol={BOTH8_FWD_TOL:.1e}")
    report(f"v1 U-Net forward, attention fp8 vs fp16 path            rel_l2={r16:.3e}")
    report(f"v1 U-Net paired prefix, attention fp8 vs fp16 path      rel_l2={rp:.3e}")
    assert ra <= ATTN8_FWD_TOL and rb <= BOTH8_FWD_TOL
    assert 1e-4 < r16 <= ATTN8_FWD_TOL and 1e-4 < rp <= ATTN8_FWD_TOL


def test_configs4_geometry_attention_fp8(dev, full):
    """96x96 latents (N = 9 216 at the top level) under guidance: one guidance-pair evaluation against the fp16 path, then a 10-step
    PLMS trajectory with attention + linear fp8, finite and bit-identical run to run."""
    from ldm.models.diffusion.plms import PLMSSampler
    from pbe_amd.precision import set_attention_precision, set_linear_precision
    g = torch.Generator().manual_seed(31)
    xT = torch.randn(1, 4, 96, 96, generator=g).to(dev)
    z = (torch.randn(1, 4, 96, 96, generator=g) * 0.8).to(dev)
    m = torch.ones(1, 1, 96, 96)
    m[:, :, 30:70, 20:60] = 0
    m = m.to(dev)
    c, uc = torch.randn(1, 1, 768, generator=g).to(dev), torch.randn(1, 1, 768, generator=g).to(dev)
    x9 = torch.cat([xT, z, m], 1)
    t = torch.tensor([981, 981], dtype=torch.int64, device=dev)

    def run():
        smp = PLMSSampler(full)
        lat, _ = smp.sample(S=10, batch_size=1, shape=[4, 96, 96], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                            unconditional_conditioning=uc, eta=0.0, x_T=xT, test_model_kwargs={"inpaint_image": z, "inpaint_mask": m})
        return lat
    with torch.no_grad():
        y16 = full.apply_model(torch.cat([x9, x9]), t, torch.cat([uc, c]))
        try:
            set_attention_precision(full, "fp8")
            y8 = full.apply_model(torch.cat([x9, x9]), t, torch.cat([uc, c]))
            set_linear_precision(full, "fp8")
            a, b = run(), run()
        finally:
            set_attention_precision(full, "fp16")
            set_linear_precision(full, "fp16")
    r = _rel(y8, y16.float())
    report(f"configs[4] geometry 96x96 guidance pair, attention fp8 vs fp16 rel_l2={r:.3e} tol={ATTN8_FWD_TOL:.1e}")
    assert 1e-4 < r <= ATTN8_FWD_TOL
    assert a.shape == (1, 4, 96, 96) and torch.isfinite(a).all() and torch.equal(a, b)
