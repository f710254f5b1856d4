"""Per-element accuracy of the default-path kernels against fp64 (tests/accgate.py holds the references, the rounding models and the
derivation of every bound): pbe_attention_f16 - exact-integer pins of all 14 instantiations, a per-element bound on random data at the
shapes the pipelines launch, and rel-L2 against a plain fp32 restatement of the kernel's arithmetic - and pbe_groupnorm_f16 /
pbe_groupnorm_apply_f16, pbe_layernorm_f16, pbe_softmax_rows_f16, pbe_geglu_f16, pbe_timestep_embedding_f16 on every output element.

All references run in fp64 on the device from the fp16 operands that were sent.  Every case appends one line to
accuracy_gate_report.txt in the directory test_model_gpu.py writes its parity report to: worst |err| / bound, where, rel-L2
(attention: also the emulation's and their ratio).
"""
import os

import pytest
import torch

import accgate as ag
import test_model_gpu as _parity

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(_parity.REPORT), "accuracy_gate_report.txt")      # beside the parity report


def report(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


def _gate(got, want, bound, what, extra=""):
    """Per-element check of every output element; the case's line goes to the report before the assertion."""
    rep = ag.compare(ag.flat(got), ag.flat(want), ag.flat(bound), what)
    rel = ag.rel_l2(got, want)
    report(f"{what:64s} err/bound={rep.ratio:.3f} at {rep.where} rel_l2={rel:.3e}{extra} ({rep.n} elements)")
    print(f"{rep}; rel-L2 {rel:.3e}{extra}")
    assert rep.ratio <= 1.0, str(rep)
    return rel


def _dg(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


# ---- attention ----------------------------------------------------------------------------------------------------------------------
def _attention(q, k, v, B, H, Nq, Nk, D, scale, dev, *, qw, mpad, pre, sliced):
    """Launch pbe_attention_f16 on fp16 operands [B, N, H D] with the dispatch knobs forced (restored afterwards); returns the output
    and the device operands as [B, H, N, D] views."""
    from pbe_amd import ops
    HD = H * D
    npad = (Nk + 7) // 8 * 8
    vt = torch.zeros(B, HD, npad, dtype=torch.float16, device=dev)
    vt[:, :, :Nk] = v.to(dev).transpose(1, 2)
    if sliced:
        assert Nq == Nk
        qk = torch.cat([q, k], -1).to(dev)                                    # the fused [q | k] buffer of the projection GEMM
        qd, kd, rs = qk, qk[..., HD:], 2 * HD
    else:
        qd, kd, rs = q.to(dev), k.to(dev), HD
    try:
        ops.tune(3, qw)
        ops.tune(6, mpad)
        out = ops.attention(qd, kd, vt, B, H, Nq, Nk, D, scale, q_strides=(Nq * rs, rs), k_strides=(Nk * rs, rs), vt_strides=(HD * npad, npad),
                            q_prescaled=pre)
    finally:
        ops.tune(3, 0)
        ops.tune(6, 1)
    torch.cuda.synchronize()
    return out, ag.heads(q.to(dev), B, Nq, H, D), ag.heads(k.to(dev), B, Nk, H, D), ag.heads(v.to(dev), B, Nk, H, D)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("case", ag.PIN_CASES, ids=lambda c: "<%s>-B%dH%d-%dx%d-D%d-qw%d-mpad%d" % c)
def test_attention_pins_exact_integers(dev, case, variant):
    """Exact-integer operands (accgate.pin_operands; exactness proven in test_accgate_cpu.py) through every attn_kernel instantiation:
    variant 1 - every query's maximum is key 0, no reference raised after tile 0; variant 2 - the rescale alpha = 2^-10 runs in a middle
    tile for the even 32-query groups and in the ragged last tile for the odd ones.  Any wrong lane map, key permutation, tail mask,
    ones row or reference hand-over shows as a wrong value, not as noise: |got - fp64| <= 0.5 ulp16 (1 + 2^-8) + 2^-24."""
    inst, B, H, Nq, Nk, D, qw, mpad = case
    assert ag.instantiation(B, H, Nq, Nk, D, qw, mpad) == inst
    q, k, v = ag.pin_operands(B, H, Nq, Nk, D, variant, ag.PIN_CASES.index(case) * 2 + variant)
    got, _, _, _ = _attention(q, k, v, B, H, Nq, Nk, D, 1.0, dev, qw=qw, mpad=mpad, pre=True, sliced=False)
    want, bound, _, _, _ = ag.pin_reference(q.to(dev), k.to(dev), v.to(dev), B, H, Nq, Nk, D)
    _gate(got, want, bound, f"pins attn_kernel<{inst}> variant {variant} B{B} H{H} {Nq}x{Nk} D{D}")


@pytest.mark.parametrize("case", ag.ATTN_CASES, ids=ag.attn_case_id)
def test_attention_per_element_and_rel_l2(dev, case):
    """Random and forced-branch operands at the shapes the pipelines launch: every output element within the rounding model's bound of
    the fp64 result, and rel-L2 no more than 1.5 x that of the plain fp32 restatement of the same instantiation's arithmetic."""
    B, H, Nq, Nk, D, recipe, qw, mpad, pre, sliced = case
    inst = ag.instantiation(B, H, Nq, Nk, D, qw, mpad)
    _, mp, ones = ag.form_of(inst)
    q, k, v, sl, scale, pre = ag.attn_case_operands(case, dev)
    got, q4, k4, v4 = _attention(q, k, v, B, H, Nq, Nk, D, scale, dev, qw=qw, mpad=mpad, pre=pre, sliced=sliced)
    want, bound = ag.attn_reference(q4, k4, v4, sl, mpad=mp, q_prescaled=pre, close=ag.attn_case_close(case))
    emu = ag.attn_emulate(q4, k4, v4, sl, mpad=mp, q_prescaled=pre, ones=ones)
    r_emu = ag.rel_l2(emu, want)
    r_got = ag.rel_l2(got, want)
    what = f"{ag.attn_case_id(case)} <{inst}>"
    _gate(got, want, bound, what, extra=f" rel_l2_emulation={r_emu:.3e} ratio={r_got / r_emu:.3f}")
    assert r_got <= ag.REL_L2_FACTOR * r_emu, f"{what}: rel-L2 {r_got:.3e} is {r_got / r_emu:.2f} x the emulation's {r_emu:.3e}"


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------
def _gn_operands(dev, B, HW, C, seed, far=False):
    g = _dg(dev, seed)
    x = (torch.randn(B, HW, C, generator=g, device=dev) * (0.5 if far else 2.0) + (8.0 if far else 0.5)).half()
    gamma = 1 + 0.1 * torch.randn(C, generator=g, device=dev)
    beta = 0.1 * torch.randn(C, generator=g, device=dev)
    return x, gamma, beta


UNET_GN = [(8, 4096, 320, 0), (8, 4096, 640, 320), (8, 4096, 320, 320), (8, 1024, 320, 0), (8, 1024, 640, 0), (8, 1024, 1280, 640),
           (8, 1024, 640, 640), (8, 1024, 640, 320), (8, 256, 640, 0), (8, 256, 1280, 0), (8, 256, 1280, 1280), (8, 256, 1280, 640),
           (8, 64, 1280, 0), (8, 64, 1280, 1280)]
VAE_GN = [(2, 262144, 128, 0), (2, 262144, 256, 0), (4, 65536, 128, 0), (4, 65536, 256, 0), (4, 65536, 512, 0), (4, 16384, 256, 0), (4, 16384, 512, 0),
          (4, 4096, 512, 0)]
EDGE_GN = [(2, 1000, 960, 0), (1, 4097, 128, 0), (3, 63, 128, 0), (2, 256, 1280, 0), (3, 64, 2560, 0), (2, 256, 1280, 1280), (3, 64, 1280, 1280)]
GN_CASES = [(s, 1e-5) for s in UNET_GN] + [(s, 1e-6) for s in VAE_GN] + [(s, 1e-5) for s in EDGE_GN]


def _groupnorm_case(dev, B, HW, C1, C2, eps, silu, rpt=16, far=False):
    from pbe_amd import ops
    C = C1 + C2
    x, gamma, beta = _gn_operands(dev, B, HW, C, C + HW + (8 if far else 0), far)
    x1, x2 = (x, None) if not C2 else (x[..., :C1].contiguous(), x[..., C1:].contiguous())
    try:
        ops.tune(7, rpt)
        got = ops.groupnorm(x1, gamma, beta, eps, silu, x2=x2)
    finally:
        ops.tune(7, 16)
    n = ag.gn_chain(HW, C, rows_per_thread=rpt)
    want, bound = ag.gn_reference(x, gamma, beta, eps, silu, n)
    path = "small-map" if ag.gn_small(HW, C) else "two-pass"
    _gate(got, want, bound, f"n:{B}:{HW}:{C1}:{C2} eps={eps:g} silu={int(silu)} rows/thread={rpt}{' mean>>std' if far else ''} [{path}, n={n}]")


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("shape,eps", GN_CASES, ids=lambda v: "n:%d:%d:%d:%d" % v if isinstance(v, tuple) else f"{v:g}")
def test_groupnorm_every_element(dev, shape, eps, silu):
    """The U-Net's and the VAE's GroupNorm launches (two-pass, single-launch small-map, two sources), HW off every block size: every
    output element against fp64; n is the fp32 chain of the path the launch takes (accgate.gn_chain)."""
    _groupnorm_case(dev, *shape, eps, silu)


@pytest.mark.parametrize("shape,eps", [((8, 4096, 320, 0), 1e-5), ((2, 262144, 128, 0), 1e-6), ((2, 1000, 960, 0), 1e-5), ((8, 1024, 1280, 640), 1e-5)],
                         ids=lambda v: "n:%d:%d:%d:%d" % v if isinstance(v, tuple) else f"{v:g}")
def test_groupnorm_other_rows_per_thread(dev, shape, eps):
    """pbe_tune key 7 (rows per thread of the statistics pass) at 5 instead of 16: other block boundaries, another n."""
    _groupnorm_case(dev, *shape, eps, True, rpt=5)


@pytest.mark.parametrize("B,HW,C", [(2, 4096, 320), (1, 65536, 128), (2, 64, 1280)])
def test_groupnorm_mean_far_above_std_every_element(dev, B, HW, C):
    """randn * 0.5 + 8 (mean = 16 std): the A term of the model - the fp32 x sc + sh with |mean sc| >> |y| - is what grows here."""
    _groupnorm_case(dev, B, HW, C, 0, 1e-5, True, far=True)


@pytest.mark.parametrize("B,H,Cin,Cout,resid", [(8, 64, 320, 320, False), (8, 64, 320, 320, True), (8, 32, 640, 640, True)])
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm_from_conv_statistics_every_element(dev, B, H, Cin, Cout, resid, silu):
    """pbe_groupnorm_apply_f16 fed by a conv's group_stats=32 partials: against the fp64 GroupNorm of the conv's STORED output; the fp32
    chain is one conv tile's rows x C / groups."""
    from pbe_amd import ops
    g = _dg(dev, B + H + Cin + Cout)
    x = (torch.randn(B, H, H, Cin, generator=g, device=dev) * 0.7).half()
    w = torch.randn(Cout, Cin, 3, 3, generator=g, device=dev) / (3 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g, device=dev) * 0.1
    kw = dict(resid=(torch.randn(B, H, H, Cout, generator=g, device=dev) * 0.8 + 0.3).half()) if resid else \
        dict(rowvec=(torch.randn(B, Cout, generator=g, device=dev) * 0.3).half())
    gamma, beta = 1 + 0.1 * torch.randn(Cout, generator=g, device=dev), 0.1 * torch.randn(Cout, generator=g, device=dev)
    y = ops.conv3x3(x, ops.pack_conv3x3(w.cpu()).to(dev), bias, group_stats=32, **kw)
    st = getattr(y, "_pbe_gstats", None)
    assert st is not None and st.groups == 32 and st.blocks > 0 and (H * H) % st.blocks == 0, "the conv left no group statistics"
    got = ops.groupnorm(y, gamma, beta, 1e-5, silu)
    n = ag.gn_chain(H * H, Cout, conv_blocks=st.blocks)
    want, bound = ag.gn_reference(y.view(B, H * H, Cout), gamma, beta, 1e-5, silu, n)
    _gate(got.view(B, H * H, Cout), want, bound, f"n:{B}:{H * H}:{Cout}:0 from conv partials ({st.blocks} blocks) resid={int(resid)} silu={int(silu)} [n={n}]")


# ---- LayerNorm, softmax rows, GEGLU, timestep embedding ----------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(100, 320), (257, 1024), (33, 1280), (7, 64), (5, 2048),
                                    (32768, 320), (16384, 320), (8192, 640), (2048, 1280), (512, 1280), (1028, 1024), (4, 1024)])
def test_layernorm_every_element(dev, rows, C):
    from pbe_amd import ops
    g = _dg(dev, C + rows)
    x = (torch.randn(rows, C, generator=g, device=dev) * 1.5 + 0.3).half()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g, device=dev), 0.1 * torch.randn(C, generator=g, device=dev)
    got = ops.layernorm(x, gamma, beta, 1e-5)
    want, bound = ag.ln_reference(x, gamma, beta, 1e-5)
    _gate(got, want, bound, f"l:{rows}:{C}")


@pytest.mark.parametrize("rows,cols,scale,sd", [(4096, 4096, 512 ** -0.5, 20.0), (300, 4096, 0.37, 4.0)])
def test_softmax_rows_every_element(dev, rows, cols, scale, sd):
    from pbe_amd import ops
    x = (torch.randn(rows, cols, generator=_dg(dev, 12), device=dev) * sd).half()
    got = ops.softmax_rows(x, scale)
    want, bound = ag.softmax_reference(x, scale)
    _gate(got, want, bound, f"softmax rows {rows}x{cols} scale={scale:.4f}")


@pytest.mark.parametrize("M,F", [(32768, 1280), (130, 1280)])
def test_geglu_every_element(dev, M, F):
    from pbe_amd import ops
    g = _dg(dev, M + F)
    h = torch.cat([torch.randn(M, F, generator=g, device=dev) * 1.5, torch.rand(M, F, generator=g, device=dev) * 24 - 12], 1).half()
    got = ops.geglu(h)
    want, bound = ag.geglu_reference(h)
    _gate(got, want, bound, f"geglu {M}x{F}, gate in [-12, 12]")


@pytest.mark.parametrize("dim", [320, 1280])
def test_timestep_embedding_every_timestep(dev, dim):
    from pbe_amd import ops
    t = torch.arange(0, 1000, dtype=torch.int64, device=dev)
    got = ops.timestep_embedding(t, dim)
    want, bound = ag.temb_reference(t, dim)
    _gate(got, want, bound, f"timestep embedding t=0..999 dim={dim}")
