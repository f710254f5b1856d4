"""Per-kernel parity on the GPU, through the C-ABI (pbe_amd.ops -> libpbe_hip.so), against plain
fp32 torch on the CPU evaluated on the SAME fp16-rounded inputs.

Tolerances (stated, fp16 I/O with fp32 accumulation): an output element may differ from the
fp32 result by fp16 rounding of the result (2^-11 relative) plus accumulation-order noise, so
we require  max|d| <= 2e-3 * max|ref| + 1e-3  per op unless a test says otherwise.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _close(got, ref, rtol=2e-3, atol=1e-3, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs().max().item()
    lim = rtol * ref.abs().max().item() + atol
    assert err <= lim, f"{what}: max|d|={err:.4e} > {lim:.4e}"


def _h(t, dev):
    return t.to(torch.float16).to(dev)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
def test_gemm_integer_layout_exact(dev):
    """A = small asymmetric integers: exact in fp16/fp32, so any fragment-layout error shows as a
    wrong integer (cdna guide: check MFMA maps with exact, asymmetric data)."""
    from pbe_amd import ops
    M, N, K = 192, 160, 128
    a = (torch.arange(M * K).reshape(M, K) % 7 - 3).float()
    w = ((torch.arange(N * K).reshape(N, K) * 5) % 11 - 5).float()
    ref = a @ w.t()
    got = ops.gemm(_h(a, dev), _h(w, dev))
    assert torch.equal(got.float().cpu(), ref)


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (257, 320, 768), (8, 1280, 320), (1024, 2560, 320), (300, 4, 2880),
                                   (96, 72, 72), (4096, 64, 128), (64, 64, 8)])
def test_gemm_shapes(dev, M, N, K):
    from pbe_amd import ops
    g = _g(M * 7 + N)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    bias = torch.randn(N, generator=g)
    ref = a.float() @ w.float().t() + bias
    got = ops.gemm(a.to(dev), w.to(dev), bias.to(dev))
    _close(got, ref, what=f"gemm {M}x{N}x{K}")


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm_epilogue(dev, act):
    from pbe_amd import ops
    g = _g(act)
    M, N, K, G = 384, 320, 256, 128
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    bias = torch.randn(N, generator=g)
    rv = torch.randn(M // G, N, generator=g).half()
    res = torch.randn(M, N, generator=g).half()
    pre = 0.5 * (a.float() @ w.float().t()) + bias + rv.float().repeat_interleave(G, 0)
    fn = {0: lambda v: v, 1: F.silu, 2: F.gelu, 3: lambda v: v * torch.sigmoid(1.702 * v)}[act]
    ref = fn(pre).half().float() + res.float()
    got = ops.gemm(a.to(dev), w.to(dev), bias.to(dev), rowvec=rv.to(dev), group_rows=G, resid=res.to(dev), act=act, alpha=0.5)
    _close(got, ref, what=f"gemm epilogue act={act}")
    # and per element against fp64 (tests/tilecheck.py expect: accumulation, epilogue, activation arm, the two fp16 stores)
    import tilecheck
    A, W = a.double(), w.double()
    want, bound = tilecheck.expect(A @ W.t(), A.abs() @ W.abs().t(), K, alpha=torch.full((N,), 0.5, dtype=torch.float64), bias=bias.double(),
                                   rowvec=rv.double().repeat_interleave(G, 0), act=act, resid=res.double())
    tilecheck.check(got.cpu(), want, tilecheck.clamp_to_close(want, bound, (2e-3, 1e-3)), f"gemm epilogue act={act}")


@pytest.mark.parametrize("M,N,K", [(512, 1280, 5120), (256, 640, 2048), (130, 320, 4096)])
def test_gemm_split_k_reduction(dev, M, N, K):
    """Few tiles + deep K -> the kernel splits K across workgroups and reduces fp32 slabs; epilogue must match."""
    from pbe_amd import ops
    g = _g(M + K)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    bias = torch.randn(N, generator=g)
    rv = torch.randn((M + 63) // 64, N, generator=g).half()
    res = torch.randn(M, N, generator=g).half()
    pre = a.float() @ w.float().t() + bias + rv.float().repeat_interleave(64, 0)[:M]
    ref = F.silu(pre).half().float() + res.float()
    got = ops.gemm(a.to(dev), w.to(dev), bias.to(dev), rowvec=rv.to(dev), group_rows=64, resid=res.to(dev), act=1)
    _close(got, ref, what=f"gemm split-K {M}x{N}x{K}")
    got2 = ops.gemm(a.to(dev), w.to(dev), bias.to(dev), rowvec=rv.to(dev), group_rows=64, resid=res.to(dev), act=1)
    assert torch.equal(got, got2), "split-K reduction must be deterministic"


def test_gemm_split_k_sources_and_bias_per_row(dev):
    from pbe_amd import ops
    g = _g(5)
    M, N, K1, K2 = 200, 136, 128, 192
    a1 = torch.randn(M, K1, generator=g).half()
    a2 = torch.randn(M, K2, generator=g).half()
    w = (torch.randn(N, K1 + K2, generator=g) / 16).half()
    bias = torch.randn(M, generator=g)
    ref = torch.cat([a1, a2], 1).float() @ w.float().t() + bias[:, None]
    got = ops.gemm(a1.to(dev), w.to(dev), bias.to(dev), a2=a2.to(dev), bias_per_row=True)
    _close(got, ref, what="gemm split-K sources")


def test_gemm_batched_strided(dev):
    from pbe_amd import ops
    g = _g(6)
    Bt, M, N, K = 3, 130, 264, 64
    a = torch.randn(Bt, M, K, generator=g).half()
    w = (torch.randn(Bt, N, K, generator=g) / 8).half()
    ref = torch.bmm(a.float(), w.float().transpose(1, 2))
    got = ops.gemm(a.to(dev), w.to(dev))
    _close(got, ref, what="gemm batched")
    # strided views: columns sliced out of a fused buffer (lda > K)
    buf = torch.randn(M, 3 * K, generator=g).half()
    w2 = (torch.randn(N, K, generator=g) / 8).half()
    got2 = ops.gemm(buf.to(dev)[:, K:2 * K], w2.to(dev))
    _close(got2, buf[:, K:2 * K].float() @ w2.float().t(), what="gemm strided A")


# ---------------------------------------------------------------------------------------------
def _conv_ref(x, w, b, stride, pad, ups, x2=None):
    xx = x if x2 is None else torch.cat([x, x2], -1)
    xx = xx.float().permute(0, 3, 1, 2)
    if ups:
        xx = F.interpolate(xx, scale_factor=2, mode="nearest")
    if pad == 0:
        xx = F.pad(xx, (0, 1, 0, 1))
    y = F.conv2d(xx, w.float(), b, stride=stride, padding=1 if pad else 0)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("B,H,W,Ci,Co,stride,pad,ups", [
    (2, 16, 16, 64, 128, 1, 1, False), (1, 12, 20, 128, 64, 1, 1, False), (2, 16, 16, 64, 64, 2, 1, False),
    (2, 16, 16, 64, 64, 2, 0, False), (2, 8, 8, 128, 128, 1, 1, True), (3, 9, 7, 192, 320, 1, 1, False),
    (1, 64, 64, 320, 320, 1, 1, False), (8, 8, 8, 1280, 1280, 1, 1, False), (4, 16, 16, 640, 640, 2, 1, False), (2, 8, 8, 640, 320, 1, 1, True)])
def test_conv3x3(dev, B, H, W, Ci, Co, stride, pad, ups):
    from pbe_amd import ops
    g = _g(H * 31 + Ci)
    x = torch.randn(B, H, W, Ci, generator=g).half()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)).half()
    b = torch.randn(Co, generator=g)
    ref = _conv_ref(x, w, b, stride, pad, ups)
    got = ops.conv3x3(x.to(dev), ops.pack_conv3x3(w.float()).to(dev), b.to(dev), stride=stride, pad=pad, upsample=ups)
    _close(got, ref, what=f"conv3x3 {B}x{H}x{W}x{Ci}->{Co} s{stride} p{pad} u{ups}")


def test_conv3x3_concat_rowvec_resid(dev):
    from pbe_amd import ops
    g = _g(9)
    B, H, W, C1, C2, Co = 2, 16, 16, 128, 64, 128
    x1 = torch.randn(B, H, W, C1, generator=g).half()
    x2 = torch.randn(B, H, W, C2, generator=g).half()
    w = (torch.randn(Co, C1 + C2, 3, 3, generator=g) / math.sqrt(9 * (C1 + C2))).half()
    b = torch.randn(Co, generator=g)
    emb = torch.randn(B, Co + 64, generator=g).half()          # rowvec taken as a column slice of a wider buffer
    res = torch.randn(B, H, W, Co, generator=g).half()
    ref = (_conv_ref(x1, w, b, 1, 1, False, x2) + emb[:, 64:].float()[:, None, None, :]).half().float() + res.float()
    got = ops.conv3x3(x1.to(dev), ops.pack_conv3x3(w.float(), split=(C1, C2)).to(dev), b.to(dev), x2=x2.to(dev), rowvec=emb.to(dev)[:, 64:], resid=res.to(dev))
    _close(got, ref, what="conv3x3 concat+emb+resid")


@pytest.mark.parametrize("B,H,W,C1,C2,Co,cfg", [
    (8, 64, 64, 320, 0, 320, 10), (8, 64, 64, 320, 0, 320, 11), (8, 64, 64, 320, 0, 320, 12), (2, 64, 64, 128, 64, 160, 10),
    (4, 32, 32, 640, 0, 640, 10), (4, 32, 32, 640, 0, 640, 11), (4, 32, 32, 128, 192, 640, 12), (8, 32, 32, 128, 0, 256, 13),
    (8, 16, 16, 256, 0, 320, 10), (8, 16, 16, 256, 0, 320, 11), (16, 8, 8, 192, 64, 160, 11), (16, 8, 8, 128, 0, 320, 10), (16, 8, 8, 128, 0, 320, 12),
    (1, 128, 128, 128, 0, 128, 14), (2, 128, 128, 64, 0, 256, 14)])
def test_conv3x3_halo_tiles(dev, B, H, W, C1, C2, Co, cfg):
    """The halo-resident conv tiles (tile configs 10 .. 14: activation halo staged once per 64-channel block, the 9 taps read
    shifted windows of it) against torch fp32 AND against the gather kernel on the same operands: same K order, same fp32
    accumulation order, so the two kernels must agree BIT for BIT when neither splits K; image borders, the two-source concat, the
    per-sample row vector, the fused residual, several images per tile (8x8) and one image row per tile (128 wide) are all covered."""
    from pbe_amd import ops
    g = _g(H * 7 + C1 + Co + cfg)
    x1 = torch.randn(B, H, W, C1, generator=g).half()
    x2 = torch.randn(B, H, W, C2, generator=g).half() if C2 else None
    w = (torch.randn(Co, C1 + C2, 3, 3, generator=g) / math.sqrt(9 * (C1 + C2))).half()
    b = torch.randn(Co, generator=g)
    emb = torch.randn(B, Co, generator=g).half()
    res = torch.randn(B, H, W, Co, generator=g).half()
    ref = (_conv_ref(x1, w, b, 1, 1, False, x2) + emb.float()[:, None, None, :]).half().float() + res.float()
    wp = ops.pack_conv3x3(w.float(), split=(C1, C2) if C2 else None).to(dev)
    args = dict(x2=None if x2 is None else x2.to(dev), rowvec=emb.to(dev), resid=res.to(dev))
    try:
        outs = {}
        for c in (cfg, 9):
            ops.tune(1, c | (1 << 8))                    # forced tile, split-K factor 1
            ops._PLANS = []
            outs[c] = ops.conv3x3(x1.to(dev), wp, b.to(dev), **args)
            plan, ops._PLANS = ops._PLANS[0], None
            assert plan[1] == c and plan[2] == 1, f"tile {c} did not apply to this shape: plan {plan}"
    finally:
        ops.tune(1, -1)
        ops._PLANS = None
    _close(outs[cfg], ref, what=f"halo conv cfg{cfg} {B}x{H}x{W}x({C1}+{C2})->{Co}")
    assert torch.equal(outs[cfg], outs[9]), f"halo tile {cfg} and the gather kernel differ in {int((outs[cfg] != outs[9]).sum())} elements"


def test_conv3x3_halo_pingpong_race_screen(dev):
    """The ping-pong main loop of the large halo tiles is a hand-placed barrier / vmcnt schedule (hazards argued in igemm.hip): screen it
    over repeated launches at three sizes - every launch must reproduce the gather kernel's bits (an early LDS read or a premature slot
    refill would show as rare wrong tiles; cdna_hip_programming.md: "screen a new sync structure over many runs at several sizes")."""
    from pbe_amd import ops
    for (B, H, C1, Co, cfg) in ((8, 64, 320, 320, 10), (8, 32, 640, 640, 12), (8, 16, 1280, 640, 10)):
        g = _g(H + C1 + cfg)
        x = torch.randn(B, H, H, C1, generator=g).half().to(dev)
        wp = ops.pack_conv3x3((torch.randn(Co, C1, 3, 3, generator=g) / math.sqrt(9 * C1))).to(dev)
        b = torch.randn(Co, generator=g).to(dev)
        noise = torch.randn(64 << 20, device=dev)            # a streaming kernel in between: uneven memory load on the CUs
        try:
            ops.tune(1, 9 | (1 << 8))
            ref = ops.conv3x3(x, wp, b)
            ops.tune(1, cfg | (1 << 8))
            bad = 0
            for i in range(60):
                if i % 3 == 0:
                    noise.mul_(1.0001)
                bad += int(not torch.equal(ops.conv3x3(x, wp, b), ref))
            assert bad == 0, f"{bad} of 60 launches of halo tile {cfg} at {H}x{H} differ from the gather kernel"
        finally:
            ops.tune(1, -1)


def test_conv3x3_halo_split_k(dev):
    """Halo tiles split K at channel-block boundaries: 1280 -> 1280 at 8x8 (20 blocks) with factors 2 .. 7 against torch fp32."""
    from pbe_amd import ops
    g = _g(4242)
    B, H, W, Ci, Co = 8, 8, 8, 1280, 320
    x = torch.randn(B, H, W, Ci, generator=g).half()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)).half()
    b = torch.randn(Co, generator=g)
    ref = _conv_ref(x, w, b, 1, 1, False)
    wp = ops.pack_conv3x3(w.float()).to(dev)
    try:
        for cfg in (10, 11):
            for sp in (2, 3, 5, 7):
                ops.tune(1, cfg | (sp << 8))
                ops._PLANS = []
                got = ops.conv3x3(x.to(dev), wp, b.to(dev))
                plan, ops._PLANS = ops._PLANS[0], None
                assert plan[1] == cfg and plan[2] >= 2
                _close(got, ref, what=f"halo conv cfg{cfg} split {sp}")
    finally:
        ops.tune(1, -1)
        ops._PLANS = None


def test_conv3x3_small_cin(dev):
    from pbe_amd import ops
    g = _g(10)
    B, H, W, Ci, Co = 2, 16, 16, 9, 64
    x = torch.randn(B, Ci, H, W, generator=g)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / 9).half()
    b = torch.randn(Co, generator=g)
    xh = ops.nchw_to_nhwc(x.to(dev), 16)
    ref = F.conv2d(x.half().float(), w.float(), b, padding=1).permute(0, 2, 3, 1)
    got = ops.conv3x3_small(xh, ops.pack_conv3x3(w.float(), 16).to(dev), b.to(dev))
    _close(got, ref, what="conv3x3 small Cin")
    back = ops.nhwc_to_nchw(xh, 9)
    assert torch.equal(back.cpu(), x.half().float())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,silu,eps", [(2, 256, 320, True, 1e-5), (3, 64, 64, False, 1e-6), (2, 64, 2560, True, 1e-5),
                                              (1, 4096, 128, True, 1e-6), (2, 1000, 960, True, 1e-5), (1, 65536, 128, True, 1e-6)])
def test_groupnorm(dev, B, HW, C, silu, eps):
    from pbe_amd import ops
    g = _g(C + HW)
    x = (torch.randn(B, HW, C, generator=g) * 2 + 0.5).half()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.group_norm(x.float().transpose(1, 2), 32, gamma, beta, eps).transpose(1, 2)
    ref = F.silu(ref) if silu else ref
    got = ops.groupnorm(x.to(dev), gamma.to(dev), beta.to(dev), eps, silu)
    _close(got, ref, rtol=3e-3, what=f"groupnorm C={C} HW={HW}")


def test_groupnorm_concat(dev):
    from pbe_amd import ops
    g = _g(77)
    B, HW, C1, C2 = 2, 256, 640, 320
    x1 = torch.randn(B, HW, C1, generator=g).half()
    x2 = (torch.randn(B, HW, C2, generator=g) * 3).half()
    gamma, beta = 1 + 0.1 * torch.randn(C1 + C2, generator=g), 0.1 * torch.randn(C1 + C2, generator=g)
    ref = F.silu(F.group_norm(torch.cat([x1, x2], -1).float().transpose(1, 2), 32, gamma, beta, 1e-5)).transpose(1, 2)
    got = ops.groupnorm(x1.to(dev), gamma.to(dev), beta.to(dev), 1e-5, True, x2=x2.to(dev))
    _close(got, ref, rtol=3e-3, what="groupnorm concat")


@pytest.mark.parametrize("rows,C", [(100, 320), (257, 1024), (33, 1280), (7, 64), (5, 2048)])
def test_layernorm(dev, rows, C):
    from pbe_amd import ops
    g = _g(C)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).half()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.layer_norm(x.float(), (C,), gamma, beta, 1e-5)
    got = ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5)
    _close(got, ref, rtol=3e-3, what=f"layernorm C={C}")


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,N,D", [(2, 8, 256, 40), (1, 8, 1024, 40), (2, 8, 256, 80), (2, 8, 64, 160), (1, 16, 257, 64),
                                      (2, 8, 256, 8), (2, 4, 130, 32), (1, 2, 64, 16), (1, 8, 4096, 40), (1, 3, 200, 128)])
def test_attention(dev, B, H, N, D):
    from pbe_amd import ops
    g = _g(N + D)
    Cc = H * D
    qk = torch.randn(B, N, 2 * Cc, generator=g).half()          # fused [q | k] buffer, as the projection GEMM writes it
    v = torch.randn(B, N, Cc, generator=g).half()
    npad = (N + 7) // 8 * 8
    vt = torch.zeros(B, Cc, npad, dtype=torch.float16)
    vt[:, :, :N] = v.transpose(1, 2)
    scale = D ** -0.5
    q4 = qk[..., :Cc].float().reshape(B, N, H, D).transpose(1, 2)
    k4 = qk[..., Cc:].float().reshape(B, N, H, D).transpose(1, 2)
    v4 = v.float().reshape(B, N, H, D).transpose(1, 2)
    ref = torch.softmax(q4 @ k4.transpose(-1, -2) * scale, -1) @ v4
    ref = ref.transpose(1, 2).reshape(B, N, Cc)
    qkd, vtd = qk.to(dev), vt.to(dev)
    got = ops.attention(qkd, qkd[..., Cc:], vtd, B, H, N, N, D, scale, q_strides=(N * 2 * Cc, 2 * Cc), k_strides=(N * 2 * Cc, 2 * Cc),
                        vt_strides=(Cc * npad, npad))
    _close(got, ref, rtol=4e-3, atol=2e-3, what=f"attention B{B} H{H} N{N} D{D}")


def test_attention_softmax_spike(dev):
    """Force the online-softmax rescale: one key row aligned with a query so the running max jumps late."""
    from pbe_amd import ops
    B, H, N, D = 1, 2, 320, 40
    g = _g(3)
    q = torch.randn(B, N, H * D, generator=g).half()
    k = torch.randn(B, N, H * D, generator=g).half()
    k[0, 300] = (q[0, 17].float() * 4).half()
    v = torch.randn(B, N, H * D, generator=g).half()
    vt = v.transpose(1, 2).contiguous()
    scale = D ** -0.5
    q4, k4, v4 = (t.float().reshape(B, N, H, D).transpose(1, 2) for t in (q, k, v))
    ref = (torch.softmax(q4 @ k4.transpose(-1, -2) * scale, -1) @ v4).transpose(1, 2).reshape(B, N, H * D)
    got = ops.attention(q.to(dev), k.to(dev), vt.to(dev), B, H, N, N, D, scale, q_strides=(N * H * D, H * D), k_strides=(N * H * D, H * D),
                        vt_strides=(H * D * N, N))
    _close(got, ref, rtol=4e-3, atol=2e-3, what="attention spike")


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 16, 128, 192), (1, 32, 32, 64, 64), (3, 8, 8, 320, 320), (1, 24, 40, 128, 128)])
def test_upsample_conv_phase_form(dev, B, H, W, Cin, Cout):
    """Nearest-2x upsample + 3x3 conv (openaimodel.py:109-119) as four 2x2 convs on the source grid (pbe_conv3x3_desc.upsample = 2,
    ops.pack_conv3x3_up_phases): against torch fp32 interpolate + conv2d, and against the fused-gather form (upsample = 1) it replaces."""
    from pbe_amd import ops
    g = _g(B * H + Cin)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(F.interpolate(x.half().float(), scale_factor=2.0, mode="nearest"), w, b, padding=1).permute(0, 2, 3, 1)
    xh = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    got = ops.conv3x3(xh, ops.pack_conv3x3_up_phases(w).to(dev), b.to(dev), upsample=True)
    old = ops.conv3x3(xh, ops.pack_conv3x3(w).to(dev), b.to(dev), upsample=True)
    assert got.shape == (B, 2 * H, 2 * W, Cout)
    _close(got, ref, rtol=2e-3, atol=2e-3, what="upsample conv, phase form")
    e_new, e_old = (got.float().cpu() - ref).norm() / ref.norm(), (old.float().cpu() - ref).norm() / ref.norm()
    assert e_new <= 1.5 * e_old + 1e-4, (e_new, e_old)


# ---- extended GEMM epilogue: the transformer block's chain (attention.py:198-252) in 5 launches --------------------------------------
def _ln_ref(x, g, b, eps=1e-5):
    return F.layer_norm(x.float(), (x.shape[-1],), g, b, eps)


@pytest.mark.parametrize("M,N,K", [(512, 320, 320), (300, 640, 640), (2048, 1280, 1280), (64, 1920, 320), (1000, 960, 320)])
def test_gemm_row_statistics_epilogue(dev, M, N, K):
    """row_stats=True: the epilogue's per-column-tile partial (sum, sumsq) of the STORED fp16 rows, with bias + row vector + residual, summed
    over the partials, against the same sums taken from the output tensor (fp64), and against pbe_row_stats_f16."""
    from pbe_amd import ops
    g = _g(M + N)
    a, w = _h(torch.randn(M, K, generator=g) * 0.7, dev), _h(torch.randn(N, K, generator=g) / K ** 0.5, dev)
    bias, resid = torch.randn(N, generator=g).to(dev), _h(torch.randn(M, N, generator=g) * 2 + 0.5, dev)
    for kw in (dict(), dict(resid=resid), dict(resid=resid, rowvec=_h(torch.randn((M + 63) // 64, N, generator=g), dev), group_rows=64)):
        plain = ops.gemm(a, w, bias, **kw)
        y, st = ops.gemm(a, w, bias, row_stats=True, **kw)
        # same tile, same k order; the two instantiations differ only in how hipcc rounds acc * alpha + bias to fp16 (fused
        # v_fma_mixlo_f16 = one rounding in the plain tile's arm, v_fma_f32 + v_cvt = two in the extended one): <= 1 ulp on a few elements
        dy = (y.float() - plain.float()).abs()
        assert (dy <= 2.0 ** -9 * plain.float().abs().clamp(min=1.0)).all() and (dy > 0).float().mean() < 1e-3
        got = st.buf[:st.parts].double().sum(0).cpu()                       # [M, 2]
        want = torch.stack([y.double().sum(1), (y.double() ** 2).sum(1)], 1).cpu()
        assert torch.allclose(got, want, rtol=2e-6, atol=1e-4), (kw.keys(), (got - want).abs().max())
        one = ops.row_stats(y)
        assert one.parts == 1 and torch.allclose(one.buf[0].double().cpu(), want, rtol=2e-6, atol=1e-4)
        y2, st2 = ops.gemm(a, w, bias, row_stats=True, **kw)
        assert torch.equal(st.buf, st2.buf)                                 # deterministic (fixed order, no atomics)


@pytest.mark.parametrize("M,N,K,act", [(512, 640, 320, 0), (777, 2560, 320, 4), (2048, 2560, 1280, 0), (64, 10240, 1280, 4), (8192, 1920, 640, 0)])
def test_gemm_layernorm_fold(dev, M, N, K, act):
    """ln=...: Linear(LayerNorm(x)) with the LayerNorm folded into the GEMM (weights x gain, bias = W beta + b, row statistics applied in
    the epilogue) against torch fp32 - rows with a large common offset included (mean >> std: the cancellation case of the fold)."""
    from pbe_amd import ops
    g = _g(N + K + act)
    x = torch.randn(M, K, generator=g) * 1.3 + 0.4
    x[: M // 4] += 6.0                                                      # |mean| = 5 std
    x = x.half()
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, 0.1 * torch.randn(N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    h = F.linear(_ln_ref(x, gamma, beta), w, b)
    if act == 4:
        Fh = N // 2
        ref = h[:, :Fh] * F.gelu(h[:, Fh:])
        wi, bi = torch.stack([w[:Fh], w[Fh:]], 1).reshape(N, K), torch.stack([b[:Fh], b[Fh:]], 1).reshape(N)
    else:
        ref, wi, bi = h, w, b
    wg, c2, c1 = ops.pack_linear_ln(wi, bi, gamma, beta)
    xd = x.to(dev)
    for st in (ops.row_stats(xd),):
        got = ops.gemm(xd, wg.to(dev), c2.to(dev), act=act, ln=(st, c1.to(dev), 1e-5))
        _close(got, ref, rtol=3e-3, atol=3e-3, what=f"LayerNorm-folded GEMM {M}x{N}x{K} act={act}")
        # and per element against fp64 on the first and last row tile and 64 seeded rows (tests/actref.py ln_fold_expect)
        import actref
        import tilecheck
        rows = tilecheck.gemm_rows(M, 128, N + K + act, 64)
        want, bound = actref.ln_fold_expect(x[rows], wg, c2, c1, act)
        tilecheck.check(got[rows].cpu(), want, tilecheck.clamp_to_close(want, bound, (3e-3, 3e-3)), f"LayerNorm-folded GEMM {M}x{N}x{K} act={act}", rows)
    old = ops.gemm(ops.layernorm(xd, gamma.to(dev), beta.to(dev), 1e-5), wi.half().to(dev), bi.to(dev), act=act)
    e_new, e_old = (got.float().cpu() - ref).norm() / ref.norm(), (old.float().cpu() - ref).norm() / ref.norm()
    assert e_new <= 1.5 * e_old + 1e-4, (e_new, e_old)                      # no worse than the separate-LayerNorm path it replaces


@pytest.mark.parametrize("B,H,Cin,Cout,resid,cfg", [(8, 64, 320, 320, False, -1), (8, 64, 320, 320, True, -1), (8, 32, 640, 640, True, -1), (2, 64, 320, 320, True, 9),
                                                     (2, 32, 640, 640, False, 11), (4, 32, 320, 640, False, 3), (3, 64, 640, 320, True, 13), (8, 16, 1280, 1280, False, -1)])
def test_conv_group_statistics_feed_groupnorm(dev, B, H, Cin, Cout, resid, cfg):
    """conv3x3(group_stats=32): the conv's copy-out leaves the following GroupNorm's partial statistics (halo, gather and 4-wave tiles, with and
    without the fused residual) and ops.groupnorm then runs its normalisation pass only - against the two-pass GroupNorm of the same
    tensor (summation order differs: close, not identical) and torch fp32.  Where the tile cannot (split-K at 16x16) the tensor carries none."""
    from pbe_amd import ops
    g = _g(B + H + Cin + Cout)
    x = (torch.randn(B, H, H, Cin, generator=g) * 0.7).half().to(dev)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    bias, emb = torch.randn(Cout, generator=g).to(dev) * 0.1, (torch.randn(B, Cout, generator=g) * 0.3).half().to(dev)
    r = (torch.randn(B, H, H, Cout, generator=g) * 0.8 + 0.3).half().to(dev) if resid else None
    gamma, beta = (1 + 0.1 * torch.randn(Cout, generator=g)).to(dev), (0.1 * torch.randn(Cout, generator=g)).to(dev)
    wp = ops.pack_conv3x3(w).to(dev)
    kw = dict(resid=r) if resid else dict(rowvec=emb)
    try:
        ops._FORCE_CFG = None if cfg < 0 else cfg
        y = ops.conv3x3(x, wp, bias, group_stats=32, **kw)
        plain = ops.conv3x3(x, wp, bias, **kw)
    finally:
        ops._FORCE_CFG = None
    assert torch.equal(y, plain)                                           # the stored values do not depend on the statistics path
    st = getattr(y, "_pbe_gstats", None)
    if H == 16 or (cfg >= 0 and st is None):
        assert st is None                                                  # split-K (the reduce kernel stores the output), or a forced tile whose columns
        got = ops.groupnorm(y, gamma, beta, 1e-5, True)                    # are not whole groups (128 columns): the two-pass norm runs as before
        assert torch.equal(got, ops.groupnorm(plain, gamma, beta, 1e-5, True))
        return
    assert st is not None and st.groups == 32 and st.blocks > 0 and (H * H) % st.blocks == 0
    tot = st.view().double().sum(1).cpu()                                  # [B, 32, 2]
    yg = y.double().cpu().view(B, H * H, 32, Cout // 32)
    want = torch.stack([yg.sum((1, 3)), (yg ** 2).sum((1, 3))], -1)
    assert torch.allclose(tot, want, rtol=2e-6, atol=1e-3), (tot - want).abs().max()
    got = ops.groupnorm(y, gamma, beta, 1e-5, True)
    two = ops.groupnorm(plain, gamma, beta, 1e-5, True)
    assert (got.float() - two.float()).abs().max().item() <= 4e-3         # two summation orders of the same statistics
    ref = F.silu(F.group_norm(y.float().cpu().permute(0, 3, 1, 2), 32, gamma.cpu(), beta.cpu(), 1e-5)).permute(0, 2, 3, 1)
    _close(got, ref, rtol=3e-3, atol=3e-3, what="GroupNorm from the conv's statistics")
    y2 = ops.conv3x3(x, wp, bias, group_stats=32, **kw)
    assert torch.equal(y2._pbe_gstats.view(), st.view())                   # deterministic


def test_conv_group_statistics_are_dropped_after_an_in_place_edit(dev):
    """The statistics a conv leaves with its output describe the values it stored: an in-place edit of the tensor afterwards (its
    _version moves) must send ops.groupnorm back to the two-pass kernels."""
    from pbe_amd import ops
    g = _g(5)
    x = (torch.randn(2, 64, 64, 320, generator=g) * 0.7).half().to(dev)
    wp = ops.pack_conv3x3(torch.randn(320, 320, 3, 3, generator=g) / 54.0).to(dev)
    gamma, beta = torch.ones(320, device=dev), torch.zeros(320, device=dev)
    y = ops.conv3x3(x, wp, None, group_stats=32)
    assert getattr(y, "_pbe_gstats", None) is not None
    y.mul_(2.0)
    got = ops.groupnorm(y, gamma, beta, 1e-5, False)
    ref = F.group_norm(y.float().cpu().permute(0, 3, 1, 2), 32, None, None, 1e-5).permute(0, 2, 3, 1)
    _close(got, ref, rtol=3e-3, atol=3e-3, what="GroupNorm after an in-place edit")
    z = ops.conv3x3(x, wp, None, group_stats=32)
    _close(ops.groupnorm(z, gamma, beta, 1e-5, False), F.group_norm(z.float().cpu().permute(0, 3, 1, 2), 32, None, None, 1e-5).permute(0, 2, 3, 1),
           rtol=3e-3, atol=3e-3, what="GroupNorm from the conv's statistics, no affine")


@pytest.mark.parametrize("M", [32768, 16384, 2048, 1280])
def test_gemm_a_stationary_matches_streaming_tile(dev, M):
    """Tile configs 19 / 20 (igemm_astat.hip: the K = 320 LayerNorm-folded GEGLU projection with the A block in registers and only the
    weights streaming) against the streaming 128x160 tile: bit-identical (same accumulation order, same epilogue association), and against
    torch fp32.  M = 1280 gives 10 row blocks - short runs, a ragged share of the chip."""
    from pbe_amd import ops
    K, N = 320, 2560
    g = _g(M)
    x = torch.randn(M, K, generator=g) * 1.3 + 0.4
    x[: M // 4] += 6.0
    x = x.half()
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, 0.1 * torch.randn(N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    h = F.linear(_ln_ref(x, gamma, beta), w, b)
    Fh = N // 2
    ref = h[:, :Fh] * F.gelu(h[:, Fh:])
    wi, bi = torch.stack([w[:Fh], w[Fh:]], 1).reshape(N, K), torch.stack([b[:Fh], b[Fh:]], 1).reshape(N)
    wg, c2, c1 = (t.to(dev) for t in ops.pack_linear_ln(wi, bi, gamma, beta))
    xd = x.to(dev)
    st = ops.row_stats(xd)
    outs = {}
    try:
        for cfg in (9, 19, 20):
            ops._FORCE_CFG = cfg
            ops._PLANS = []
            outs[cfg] = ops.gemm(xd, wg, c2, act=ops.ACT_GEGLU, ln=(st, c1, 1e-5))
            assert ops._PLANS[0][1] == cfg, ops._PLANS                    # the forced tile really ran
            again = ops.gemm(xd, wg, c2, act=ops.ACT_GEGLU, ln=(st, c1, 1e-5))
            assert torch.equal(outs[cfg], again)
    finally:
        ops._FORCE_CFG, ops._PLANS = None, None
    _close(outs[19], ref, rtol=3e-3, atol=3e-3, what=f"A-stationary GEGLU projection M={M}")
    assert torch.equal(outs[19], outs[9]) and torch.equal(outs[20], outs[9])


@pytest.mark.parametrize("B,N", [(8, 4096), (4, 4096), (3, 1024), (2, 160)])
def test_gemm_a_stationary_qkv_matches_streaming_tile(dev, B, N):
    """Tile 20 on the fused q | k | v^T projection (K = 320, LayerNorm folded, alpha on the q columns only, v stored transposed) against the
    streaming 128x160 tile: bit-identical q | k and V^T, and against torch fp32.  N = 160 tokens: 32 | N but a 128-row block spans samples."""
    from pbe_amd import ops
    C, M = 320, B * N
    g = _g(M + 3)
    x = (torch.randn(M, C, generator=g) * 1.3 + 0.4).half()
    w, b = torch.randn(3 * C, C, generator=g) / C ** 0.5, 0.1 * torch.randn(3 * C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.linear(_ln_ref(x, gamma, torch.zeros(C)), w)                    # alpha scales the product, not the folded bias W beta + b
    ref[:, :C] *= 0.2281
    ref += w @ beta + b
    wg, c2, c1 = (t.to(dev) for t in ops.pack_linear_ln(w, b, gamma, beta))
    xd = x.to(dev)
    st = ops.row_stats(xd)
    outs = {}
    try:
        for cfg in (9, 20):
            ops._FORCE_CFG = cfg
            ops._PLANS = []
            qk = torch.zeros(M, 2 * C, dtype=torch.float16, device=dev)
            vt = torch.zeros(B, C, N, dtype=torch.float16, device=dev)
            ops.gemm(xd, wg, c2, ln=(st, c1, 1e-5), alpha=0.2281, alpha_cols=C, out=qk, vt=vt, vt_col0=2 * C, vt_tokens=N)
            if M % 128 == 0:
                assert ops._PLANS[0][1] == cfg, ops._PLANS
            outs[cfg] = (qk, vt)
    finally:
        ops._FORCE_CFG, ops._PLANS = None, None
    assert torch.equal(outs[20][0], outs[9][0]) and torch.equal(outs[20][1], outs[9][1])
    _close(outs[20][0], ref[:, :2 * C], rtol=3e-3, atol=3e-3, what="q | k")
    _close(outs[20][1].transpose(1, 2).reshape(M, C), ref[:, 2 * C:], rtol=3e-3, atol=3e-3, what="v^T")


@pytest.mark.parametrize("B,N,C,heads", [(2, 256, 320, 8), (8, 64, 1280, 8), (1, 1024, 640, 8), (3, 256, 1280, 8)])
def test_fused_qkv_projection_and_attention(dev, B, N, C, heads):
    """ONE launch for to_q | to_k | to_v with norm1 folded in, q pre-scaled by scale log2(e) in the fp32 epilogue and v stored transposed
    (CrossAttention.self_attention_fused), then the attention core with q_prescaled: against torch fp32 attention on LayerNorm(x)."""
    from ldm.modules.attention import BasicTransformerBlock
    from pbe_amd import ops
    from pbe_amd.weights import fill_module_
    blk = BasicTransformerBlock(C, heads, C // heads, context_dim=768)
    fill_module_(blk, prefix=f"tfq{C}.")
    blk = blk.to(dev).eval()
    g = _g(B * N + C)
    x = (torch.randn(B * N, C, generator=g) * 1.5 + 0.3).half()
    a = blk.attn1
    xn = _ln_ref(x, blk.norm1.weight.cpu(), blk.norm1.bias.cpu(), blk.norm1.eps)
    q, k, v = (F.linear(xn, m.weight.cpu().float()).view(B, N, heads, C // heads).transpose(1, 2) for m in (a.to_q, a.to_k, a.to_v))
    ref = (torch.softmax(q @ k.transpose(-1, -2) * a.scale, -1) @ v).transpose(1, 2).reshape(B * N, C)
    xd = x.to(dev)
    with torch.no_grad():
        got = a.self_attention_fused(xd, ops.row_stats(xd), blk.pk(), B, N)
        old = a.self_attention(ops.layernorm(xd, blk.pk().g1, blk.pk().b1, blk.pk().eps1), B, N)
    _close(got, ref, rtol=4e-3, atol=3e-3, what=f"fused q|k|v^T + attention B{B} N{N} C{C}")
    e_new, e_old = (got.float().cpu() - ref).norm() / ref.norm(), (old.float().cpu() - ref).norm() / ref.norm()
    assert e_new <= 1.5 * e_old + 1e-4, (e_new, e_old)


def test_gemm_alpha_cols_and_transposed_columns(dev):
    """alpha_cols and VT alone (no LayerNorm): C[:, :c0] scaled, columns >= vt_col0 land in VT[b, n - vt_col0, token]."""
    from pbe_amd import ops
    g = _g(91)
    B, T, K, N, c0 = 4, 64, 320, 960, 320
    a, w, bias = _h(torch.randn(B * T, K, generator=g), dev), _h(torch.randn(N, K, generator=g) / K ** 0.5, dev), torch.randn(N, generator=g).to(dev)
    ref = F.linear(a.float().cpu(), w.float().cpu())
    ref[:, :c0] *= 0.37
    ref = ref + bias.cpu()
    vt = torch.zeros(B, N - 640, T, dtype=torch.float16, device=dev)
    out = ops.gemm(a, w, bias, alpha=0.37, alpha_cols=c0, vt=vt, vt_col0=640, vt_tokens=T)
    assert out.shape == (B * T, 640)
    _close(out, ref[:, :640], rtol=2e-3, atol=2e-3, what="alpha_cols")
    _close(vt.transpose(1, 2).reshape(B * T, N - 640), ref[:, 640:], rtol=2e-3, atol=2e-3, what="VT columns")


@pytest.mark.parametrize("D", [40, 80, 64])
@pytest.mark.parametrize("case", ["first_tile_peak", "negative_start_then_jump", "large_logits", "band_below_threshold", "ragged_jump_in_last_tile"])
def test_attention_deferred_max_paths(dev, D, case):
    """The deferred reference maximum (attention.hip, ATTN_THR) and, at d = 40, the reference carried in the head-dim padding: inputs
    that FORCE each branch (cdna guide rule 26) against a full fp32 reference - the maximum in the first tile and never again, a
    first tile far below the rest (negative reference, then one big raise), logits of +-3000 log2 units (the fp16 m / 64 form), growth
    that stays inside the threshold band (no raise: P up to 2^8), and a raise inside the ragged last tile."""
    from pbe_amd import ops
    B, H, N = 1, 2, 330 if case == "ragged_jump_in_last_tile" else 384
    g = _g(17 + D)
    q = torch.randn(B, N, H * D, generator=g)
    k = torch.randn(B, N, H * D, generator=g)
    v = torch.randn(B, N, H * D, generator=g)
    q4, k4 = q.view(B, N, H, D), k.view(B, N, H, D)
    if case == "first_tile_peak":
        k4[0, 5] = q4[0, 40] * 3.0                                    # every query block sees its largest scores in tile 0
        k4[0, 9] = q4[0, 200] * 3.0
    elif case == "negative_start_then_jump":
        k4[0, :64] = -2.5 * torch.sign(q4[0, 100:101]) * torch.ones(64, H, D)      # tile 0 anti-aligned with query 100: its first reference is far below 0
        k4[0, 300] = q4[0, 100] * 4.0
    elif case == "large_logits":
        q4 *= 7.0
        k4 *= 7.0
    elif case == "band_below_threshold":
        for t in range(1, 6):                                          # each tile's best key beats the previous by ~1 log2 unit for query 7
            k4[0, 64 * t + 3] = q4[0, 7] * (0.25 * t)
    else:
        k4[0, 325] = q4[0, 33] * 4.0
    q, k, v = q.half(), k.half(), v.half()
    npad = (N + 7) // 8 * 8
    vt = torch.zeros(B, H * D, npad, dtype=torch.float16)
    vt[:, :, :N] = v.transpose(1, 2)
    scale = D ** -0.5
    q4, k4, v4 = (t.double().reshape(B, N, H, D).transpose(1, 2) for t in (q, k, v))
    ref = (torch.softmax(q4 @ k4.transpose(-1, -2) * scale, -1) @ v4).transpose(1, 2).reshape(B, N, H * D).float()
    args = (q.to(dev), k.to(dev), vt.to(dev), B, H, N, N, D, scale)
    kw = dict(q_strides=(N * H * D, H * D), k_strides=(N * H * D, H * D), vt_strides=(H * D * npad, npad))
    got = ops.attention(*args, **kw)
    assert torch.isfinite(got).all()
    # d = 40 with logits of +-400 log2 units: the in-kernel fold of scale log2e into Q rounds q once more (2^-11 per element, i.e.
    # ~0.03 log2 units on such logits -> 2 % on a P that competes with the row maximum); the product path pre-scales Q in the fp32
    # epilogue of the projection GEMM instead (pbe_attn_desc.q_prescaled) and the multiply-add form below has no such term
    loose = case == "large_logits" and D == 40
    _close(got, ref, rtol=1.2e-2 if loose else 4e-3, atol=2e-3, what=f"attention {case} D={D}")
    if D == 40:                                                        # the multiply-add form of the same kernel agrees
        ops.tune(6, 0)
        try:
            plain = ops.attention(*args, **kw)
        finally:
            ops.tune(6, 1)
        _close(plain, ref, rtol=4e-3, atol=2e-3, what=f"attention {case} D={D}, multiply-add form")


def test_softmax_rows_and_geglu(dev):
    from pbe_amd import ops
    g = _g(12)
    x = (torch.randn(300, 4096, generator=g) * 4).half()
    got = ops.softmax_rows(x.to(dev), 0.37)
    _close(got, torch.softmax(x.float() * 0.37, -1), rtol=3e-3, atol=1e-6, what="softmax_rows")
    h = torch.randn(130, 2 * 1280, generator=g).half()
    a, gate = h.float().chunk(2, -1)
    _close(ops.geglu(h.to(dev)), a * F.gelu(gate), what="geglu")


def test_timestep_embedding(dev, golden_dir):
    import numpy as np
    from pbe_amd import ops
    gold = np.load(f"{golden_dir}/primitives.npz")
    got = ops.timestep_embedding(torch.from_numpy(gold["temb_t"]).to(dev), 320)
    _close(got, torch.from_numpy(gold["temb"]), rtol=1e-3, atol=2e-3, what="timestep_embedding vs reference golden")


def test_plms_kernels(dev):
    from pbe_amd import ops
    g = _g(21)
    B, H, W = 2, 16, 16
    x, z, m = torch.randn(B, 4, H, W, generator=g), torch.randn(B, 4, H, W, generator=g), torch.rand(B, 1, H, W, generator=g)
    x9 = ops.plms_pack_input(x.to(dev), z.to(dev), m.to(dev), 2).float().cpu()
    ref = torch.cat([x, z, m], 1).permute(0, 2, 3, 1).half().float()
    assert torch.equal(x9[:B, ..., :9], ref) and torch.equal(x9[B:, ..., :9], ref) and (x9[..., 9:] == 0).all()
    eps = torch.randn(2 * B, H, W, 8, generator=g).half()
    h1, h2, h3 = (torch.randn(B, 4, H, W, generator=g) for _ in range(3))
    coef = [55 / 24, -59 / 24, 37 / 24, -9 / 24, 0.6, 1.25, 0.9, 0.43]
    e_u, e_c = eps[:B, ..., :4].float().permute(0, 3, 1, 2), eps[B:, ..., :4].float().permute(0, 3, 1, 2)
    e = e_u + 5.0 * (e_c - e_u)
    ep = coef[0] * e + coef[1] * h1 + coef[2] * h2 + coef[3] * h3
    px0 = (x - coef[4] * ep) * coef[5]
    xp = coef[6] * px0 + coef[7] * ep
    gx, gp, ge = ops.plms_update(eps.to(dev), 2, 5.0, x.to(dev), [h1.to(dev), h2.to(dev), h3.to(dev)], coef)
    _close(ge, e, rtol=1e-5, atol=1e-5, what="plms e_t")
    _close(gp, px0, rtol=1e-5, atol=1e-5, what="plms pred_x0")
    _close(gx, xp, rtol=1e-5, atol=1e-5, what="plms x_prev")


def test_posterior_latent_image_kernels(dev):
    from pbe_amd import ops
    g = _g(22)
    B, H, W = 2, 8, 8
    mom = (torch.randn(B, H, W, 8, generator=g) * 3).half()
    eps = torch.randn(B, 4, H, W, generator=g)
    mean, logvar = mom.float()[..., :4].permute(0, 3, 1, 2), mom.float()[..., 4:].permute(0, 3, 1, 2)
    ref = 0.18215 * (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * eps)
    _close(ops.posterior_sample(mom.to(dev), eps.to(dev), 0.18215), ref, rtol=1e-5, atol=1e-5, what="posterior")
    z = torch.randn(B, 9, H, W, generator=g)
    zl = ops.scale_latent(z.to(dev), 1 / 0.18215).float().cpu()
    assert torch.equal(zl[..., :4], (z[:, :4] / 0.18215 if False else (z[:, :4] * (1 / 0.18215))).permute(0, 2, 3, 1).half().float())
    assert (zl[..., 4:] == 0).all()
    img = (torch.randn(B, H, W, 8, generator=g) * 2).half()
    _close(ops.image_post(img.to(dev)), ((img.float()[..., :3] + 1) / 2).clamp(0, 1).permute(0, 3, 1, 2), rtol=1e-6, atol=1e-6, what="image_post")


def test_clip_patchify(dev):
    from pbe_amd import ops
    g = _g(23)
    px = torch.randn(2, 3, 224, 224, generator=g)
    got = ops.clip_patchify(px.to(dev), 14, 592).float().cpu()
    ref = F.unfold(px, 14, stride=14).transpose(1, 2).reshape(2 * 256, 588).half().float()
    assert torch.equal(got[:, :588], ref) and (got[:, 588:] == 0).all()


def test_errors_are_loud(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError):
        ops.gemm(torch.zeros(8, 8, dtype=torch.float16), torch.zeros(8, 8, dtype=torch.float16))      # CPU tensors
    with pytest.raises(PbeError):
        ops.gemm(torch.zeros(8, 12, dtype=torch.float16, device=dev), torch.zeros(8, 12, dtype=torch.float16, device=dev))  # K % 8
    with pytest.raises(PbeError):
        ops.conv3x3(torch.zeros(1, 4, 4, 9, dtype=torch.float16, device=dev), torch.zeros(8, 81, dtype=torch.float16, device=dev), None)


@pytest.mark.parametrize("M,F,K", [(300, 256, 64), (4096, 1280, 320), (64, 5120, 1280)])
def test_gemm_fused_geglu(dev, M, F, K):
    """attention.py:41-45: x, gate = proj(x).chunk(2); x * gelu(gate) — fused in the GEMM epilogue (interleaved rows)."""
    from pbe_amd import ops
    g = _g(M + F)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(2 * F, K, generator=g) / math.sqrt(K)).half()
    b = torch.randn(2 * F, generator=g) * 0.1
    h = a.float() @ w.float().t() + b
    ref = h[:, :F] * F_gelu(h[:, F:])
    wi, bi = ops.pack_geglu(w.float().to(dev), b.to(dev))
    got = ops.gemm(a.to(dev), wi, bi, act=ops.ACT_GEGLU)
    assert got.shape == (M, F)
    _close(got, ref, what=f"fused GEGLU {M}x{F}x{K}")


def F_gelu(x):
    return F.gelu(x)


@pytest.mark.parametrize("B,HW,C", [(2, 256, 1280), (8, 64, 1280), (3, 64, 2560), (2, 256, 2560)])
def test_groupnorm_small_map_single_launch(dev, B, HW, C):
    from pbe_amd import ops
    g = _g(C + HW + 1)
    x = (torch.randn(B, HW, C, generator=g) * 2 + 0.5).half()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.silu(F.group_norm(x.float().transpose(1, 2), 32, gamma, beta, 1e-5)).transpose(1, 2)
    _close(ops.groupnorm(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5, True), ref, rtol=3e-3, what=f"groupnorm small C={C} HW={HW}")
    x1, x2 = x[..., :C // 2].contiguous(), x[..., C // 2:].contiguous()
    _close(ops.groupnorm(x1.to(dev), gamma.to(dev), beta.to(dev), 1e-5, True, x2=x2.to(dev)), ref, rtol=3e-3, what="groupnorm small concat")


@pytest.mark.parametrize("cfg", list(range(10)) + [15, 16, 17, 18] + [0 | (3 << 8), 4 | (2 << 8), 17 | (2 << 8)])
def test_every_tile_config_with_every_epilogue(dev, cfg):
    """Each block-tile config (and two forced split-K factors) through the epilogue variants that have their own code path:
    bias + per-sample row vector staged in LDS with 1, 2 and 4 samples per tile (8x8 level: 64 pixels per sample), the
    unaligned fall-back (row groups that do not tile), SiLU / GEGLU, residual, per-row bias; M and N off the tile grid."""
    from pbe_amd import ops
    g = _g(77 + (cfg & 255))
    ops.tune(1, cfg)
    try:
        # conv, 8 samples of 8x8 (M = 512): a 256-row tile spans 4 samples, a 128-row tile 2, a 64-row tile 1
        B, H, W, Ci, Co = 8, 8, 8, 64, 200
        x = torch.randn(B, H, W, Ci, generator=g).half()
        w = (torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)).half()
        b = torch.randn(Co, generator=g)
        emb = torch.randn(B, Co, generator=g).half()
        res = torch.randn(B, H, W, Co, generator=g).half()
        ref = F.silu((_conv_ref(x, w, b, 1, 1, False) + emb.float()[:, None, None, :])).half().float() + res.float()
        got = ops.conv3x3(x.to(dev), ops.pack_conv3x3(w.float()).to(dev), b.to(dev), rowvec=emb.to(dev), resid=res.to(dev), act=ops.ACT_SILU)
        _close(got, ref, what=f"cfg {cfg}: conv 8x8x8 emb+silu+resid")
        # GEMM with row groups of 48 rows (do not tile 64/128/256): generic path
        M, N, K, grp = 336, 328, 192, 48
        a = torch.randn(M, K, generator=g).half()
        wl = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
        bias = torch.randn(N, generator=g)
        rv = torch.randn(M // grp, N, generator=g).half()
        ref = (a.float() @ wl.float().t() + bias + rv.float().repeat_interleave(grp, 0)).half().float()
        got = ops.gemm(a.to(dev), wl.to(dev), bias.to(dev), rowvec=rv.to(dev), group_rows=grp)
        _close(got, ref, what=f"cfg {cfg}: gemm rowvec groups of 48")
        # per-row bias (the V^T projection's orientation) and alpha
        bm = torch.randn(M, generator=g)
        ref = (0.5 * (a.float() @ wl.float().t()) + bm[:, None]).half().float()
        got = ops.gemm(a.to(dev), wl.to(dev), bm.to(dev), bias_per_row=True, alpha=0.5)
        _close(got, ref, what=f"cfg {cfg}: gemm per-row bias, alpha")
        # fused GEGLU (value / gate rows interleaved by pack_geglu), rows off the tile grid
        Fo = 160
        w2 = (torch.randn(2 * Fo, K, generator=g) / math.sqrt(K)).half()
        b2 = torch.randn(2 * Fo, generator=g)
        h = a.float() @ w2.float().t() + b2
        ref = (h[:, :Fo] * F.gelu(h[:, Fo:])).half().float()
        wi, bi = ops.pack_geglu(w2.float(), b2)
        got = ops.gemm(a.to(dev), wi.to(dev), bi.to(dev), act=ops.ACT_GEGLU)
        _close(got, ref, what=f"cfg {cfg}: fused GEGLU")
    finally:
        ops.tune(1, -1)


def test_resize_bilinear_against_torch(dev):
    """pbe_resize_bilinear_f32 (the mask resize of scripts/inference.py:332) against torch's F.interpolate on the CPU (fp32), both
    antialias settings, the 512 -> 64 case of the path on a real bundled mask plus ragged / up-scaling sizes."""
    import os
    import numpy as np
    from PIL import Image
    from pbe_amd import ops
    here = os.path.dirname(os.path.abspath(__file__))
    m = np.array(Image.open(os.path.join(here, "golden", "examples", "mask_example_1.png")).convert("L"))[None, None]
    mask = torch.from_numpy((1 - m.astype(np.float32) / 255.0 >= 0.5).astype(np.float32))
    g = torch.Generator().manual_seed(11)
    cases_ = [(mask, (64, 64)), (torch.rand(2, 3, 224, 224, generator=g), (512, 512)), (torch.rand(3, 1, 100, 77, generator=g), (13, 31)),
              (torch.rand(1, 2, 96, 96, generator=g), (96, 96)), (torch.rand(1, 1, 768, 768, generator=g), (96, 96))]
    for x, size in cases_:
        for aa in (True, False):
            got = ops.resize_bilinear(x.to(dev), size, aa).cpu()
            ref = F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=aa)
            assert got.shape == ref.shape
            err = (got - ref).abs().max().item()
            assert err <= 2e-6, (tuple(x.shape), size, aa, err)
    binary = ops.resize_bilinear(mask.to(dev), (64, 64), True).cpu()
    assert -1e-6 <= binary.min() and binary.max() <= 1.0 + 1e-6 and ((binary > 1e-3) & (binary < 1 - 1e-3)).any()        # edges are NOT re-binarised


# ---- fp8 (OCP e4m3) operand path: BASELINE configs[4] ----------------------------------------------------------------------
def _deq(w8, scale):
    return w8.view(torch.float8_e4m3fn).float() * scale[:, None]


@pytest.mark.parametrize("M,N,K,geglu,resid", [(192, 160, 128, False, False), (4096, 640, 320, False, True), (2048, 2560, 320, True, False),
                                               (1000, 96, 1280, False, False), (256, 1280, 640, False, True), (64, 64, 16, False, False)])
def test_gemm_f8_exact_against_dequantised_operands(dev, M, N, K, geglu, resid):
    """The fp8 operand form of pbe_gemm_f16 computes EXACTLY the product of the dequantised operands (e4m3 x e4m3 products are exact
    in fp32; only the fp32 accumulation order and the fp16 output rounding remain): compared with torch fp32 on a8 * sa, w8 * sw."""
    from pbe_amd import ops
    g = _g(M + N + K)
    a = torch.randn(M, K, generator=g) * torch.rand(M, 1, generator=g) * 3
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    a8, sa = ops.pack_linear_f8(a)                       # same quantiser for both operands in this test
    w8, sw = ops.pack_linear_f8(w)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).half() if resid else None
    ref = _deq(a8, sa) @ _deq(w8, sw).t() + bias
    if geglu:
        wi = torch.stack([w8[:N // 2], w8[N // 2:]], 1).reshape(N, K)
        si = torch.stack([sw[:N // 2], sw[N // 2:]], 1).reshape(N)
        bi = torch.stack([bias[:N // 2], bias[N // 2:]], 1).reshape(N)
        got = ops.gemm_f8(a8.to(dev), sa.to(dev), wi.to(dev), si.to(dev), bi.to(dev), act=ops.ACT_GEGLU)
        ref = ref[:, :N // 2] * F.gelu(ref[:, N // 2:])
    else:
        got = ops.gemm_f8(a8.to(dev), sa.to(dev), w8.to(dev), sw.to(dev), bias.to(dev), resid=None if res is None else res.to(dev))
        if res is not None:
            ref = ref.half().float() + res.float()
    _close(got, ref, rtol=1.5e-3, atol=1.5e-3, what=f"gemm_f8 {M}x{N}x{K}")


def test_gemm_f8_batched_vt_layout(dev):
    """The V^T projection form: weights as the A operand (shared over the batch, scale per channel), activations as W (scale per token)."""
    from pbe_amd import ops
    g = _g(5)
    B, N, Cc, inner = 3, 200, 320, 256
    x = torch.randn(B, N, Cc, generator=g)
    w = torch.randn(inner, Cc, generator=g) / math.sqrt(Cc)
    x8, sx = ops.pack_linear_f8(x.reshape(B * N, Cc))
    w8, sw = ops.pack_linear_f8(w)
    npad = (N + 7) // 8 * 8
    vt = torch.zeros(B, inner, npad, dtype=torch.float16, device=dev)
    ops.gemm_f8(w8.to(dev).unsqueeze(0).expand(B, -1, -1), sw.to(dev), x8.to(dev).view(B, N, Cc), sx.to(dev).view(B, N), out=vt[:, :, :N])
    ref = torch.einsum("ik,bnk->bin", _deq(w8, sw), _deq(x8, sx).view(B, N, Cc))
    _close(vt[:, :, :N], ref, rtol=1.5e-3, atol=1.5e-3, what="gemm_f8 V^T")


def test_layernorm_f8(dev):
    """pbe_layernorm_f8: y8 * scale reproduces LayerNorm within e4m3 rounding (relative 2^-4 per element), the scale is max|LN| / 448
    within 2e-3 relative, the row maximum maps to +-448 exactly, and every code lies in its admissible interval of the fp64 LayerNorm
    over the reported scale (f8ref.ln8_gate: at most 2 % of the elements may have more than one admissible code; byte equality proper
    is test_f8gate_gpu.py's exact tier)."""
    import f8ref
    from pbe_amd import ops
    g = _g(8)
    for rows, Cc in ((300, 320), (64, 1280), (17, 640)):
        x = (torch.randn(rows, Cc, generator=g) * 2 + 0.3).half()
        gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
        y8, sc = ops.layernorm_f8(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5)
        ref = F.layer_norm(x.float(), (Cc,), gamma, beta, 1e-5)
        deq = y8.cpu().view(torch.float8_e4m3fn).float() * sc.cpu()[:, None]
        assert torch.allclose(sc.cpu(), ref.abs().amax(1) / 448.0, rtol=2e-3)
        err = (deq - ref).abs()
        assert (err <= ref.abs() * 2 ** -4 + sc.cpu()[:, None] * 2 ** -9 + 2e-3).all(), err.max()
        assert (y8.cpu().view(torch.float8_e4m3fn).float().abs().amax(1) == 448.0).all()
        f8ref.ln8_gate(y8, sc, x, gamma, beta, 1e-5, f"test_layernorm_f8 {rows}x{Cc}")


def test_cross_attention_general_context(dev):
    """CrossAttention.forward with a multi-token context (attention.py:207-230 in full: separate q / k / v projections, softmax over the
    context tokens) - not on the Paint-by-Example path (its context is ONE exemplar token) but part of the class's contract - and the
    self-attention form, against torch fp32."""
    from ldm.modules.attention import CrossAttention
    g = _g(77)
    B, N, Nk, Cq, Cc, heads, dh = 2, 130, 7, 320, 768, 8, 40
    m = CrossAttention(query_dim=Cq, context_dim=Cc, heads=heads, dim_head=dh)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) / math.sqrt(p_.shape[-1]))
    x = torch.randn(B, N, Cq, generator=g)
    ctx = torch.randn(B, Nk, Cc, generator=g)

    def ref(mod, xq, c):
        c = xq if c is None else c
        q, k, v = xq @ mod.to_q.weight.t(), c @ mod.to_k.weight.t(), c @ mod.to_v.weight.t()
        sp = lambda t: t.view(t.shape[0], t.shape[1], heads, dh).permute(0, 2, 1, 3)
        a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * dh ** -0.5, -1) @ sp(v)
        return a.permute(0, 2, 1, 3).reshape(xq.shape[0], xq.shape[1], heads * dh) @ mod.to_out[0].weight.t() + mod.to_out[0].bias
    want = ref(m, x, ctx)
    md = m.to(dev)
    with torch.no_grad():
        got = md(x.to(dev), context=ctx.to(dev))
    _close(got, want, rtol=4e-3, atol=4e-3, what="CrossAttention, 7-token context")
    ms = CrossAttention(query_dim=Cq, heads=heads, dim_head=dh)
    with torch.no_grad():
        for p_ in ms.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) / math.sqrt(p_.shape[-1]))
        want_s = ref(ms, x, None)
        got_s = ms.to(dev)(x.to(dev))
    _close(got_s, want_s, rtol=4e-3, atol=4e-3, what="CrossAttention, self-attention form")


@pytest.mark.parametrize("K1,K2", [(96, 104), (32, 40), (128, 72), (64, 64), (96, 96)])
def test_gemm_ragged_k_and_straddling_concat(dev, K1, K2):
    """The two k-tiles that leave the lean DMA form (igemm.hip, loader state): a last k-tile with K % 64 != 0 (per-lane zeros beyond K)
    and a k-tile that straddles the two concatenated sources (K1 % 64 != 0), alone and together, with rows off the tile grid (the
    clamped rows of the lean form) - every dense tile family, forced."""
    from pbe_amd import ops
    g = _g(K1 * 7 + K2)
    M, N = 200, 136
    a1 = torch.randn(M, K1, generator=g).half()
    a2 = torch.randn(M, K2, generator=g).half()
    w = (torch.randn(N, K1 + K2, generator=g) / math.sqrt(K1 + K2)).half()
    bias = torch.randn(N, generator=g)
    ref = (torch.cat([a1, a2], 1).float() @ w.float().t() + bias).half().float()
    try:
        for cfg in (-1, 3, 6, 9, 1, 17, 21):               # 21: 8 waves x 160 columns - 20 weight pieces over 8 waves, the padding pieces repeat the last one
            ops.tune(1, cfg)
            _close(ops.gemm(a1.to(dev), w.to(dev), bias.to(dev), a2=a2.to(dev)), ref, what=f"gemm K1={K1} K2={K2} cfg {cfg}")
            ops.tune(1, -1)
        aw = torch.cat([a1, a2], 1).contiguous()
        _close(ops.gemm(aw.to(dev), w.to(dev), bias.to(dev)), ref, what=f"gemm K={K1 + K2} single source")
    finally:
        ops.tune(1, -1)


def test_dense_256x160_tile_matches_128x160(dev):
    """Tile 21 (256x160, 8 waves, ring of 3: the ff-out / out-projection of the 64x64 level through the tuned table) against the 4-wave
    128x160 tile: same accumulation order, bit-identical with and without the fused residual, on the tile grid and off it."""
    from pbe_amd import ops
    g = _g(21)
    for (M, N, K) in ((4096, 320, 1280), (1000, 300, 320), (512, 640, 704)):
        a = (torch.randn(M, K, generator=g) * 0.5).half().to(dev)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).half().to(dev)
        b = torch.randn(N, generator=g).to(dev)
        r = torch.randn(M, N, generator=g).half().to(dev)
        outs = {}
        try:
            for cfg in (9, 21):
                ops._FORCE_CFG = cfg
                ops._PLANS = []
                outs[cfg] = (ops.gemm(a, w, b), ops.gemm(a, w, b, resid=r if N % 8 == 0 else None))
                assert ops._PLANS[0][1] == cfg, ops._PLANS
        finally:
            ops._FORCE_CFG, ops._PLANS = None, None
        assert torch.equal(outs[9][0], outs[21][0]) and torch.equal(outs[9][1], outs[21][1])
        _close(outs[21][0], a.float().cpu() @ w.float().cpu().t() + b.cpu(), rtol=3e-3, atol=3e-3, what=f"dense 256x160 {M}x{N}x{K}")


def test_xcd_tile_order_is_bit_neutral(dev):
    """The per-launch XCD tile order (m fastest where the weight panel is the big operand: igemm.hip, launch_cfg; pbe_tune key 5) only
    renumbers which workgroup computes which tile: outputs with the choice on and forced off must be identical, on a deep-weight
    conv (16x16, 1280 channels: m fastest is chosen), its split-K form, and a GEGLU-shaped GEMM."""
    from pbe_amd import ops
    g = _g(4242)
    x = torch.randn(8, 16, 16, 1280, generator=g).half().to(dev)
    w = (torch.randn(1280, 1280, 3, 3, generator=g) / math.sqrt(9 * 1280)).half()
    wp = ops.pack_conv3x3(w.float()).to(dev)
    b = torch.randn(1280, generator=g).to(dev)
    a = torch.randn(2048, 1280, generator=g).half().to(dev)
    wl = (torch.randn(10240, 1280, generator=g) / math.sqrt(1280)).half().to(dev)
    outs = {}
    try:
        for v in (1, 0):
            ops.tune(5, v)
            outs[v] = (ops.conv3x3(x, wp, b), ops.gemm(a, wl))
            ops.tune(1, 10 | (4 << 8))
            outs[v] += (ops.conv3x3(x, wp, b),)
            ops.tune(1, -1)
    finally:
        ops.tune(5, 1)
        ops.tune(1, -1)
    for got, want in zip(outs[1], outs[0]):
        assert torch.equal(got, want)
