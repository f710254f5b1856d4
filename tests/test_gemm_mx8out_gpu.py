"""MX-fp8 output of the q|k|v^T projections (pbe_gemm_mx8out_f16): every byte of data and scales, padding included, equals the fp16
projection followed by pbe_quant_mx8_f16 - on the LayerNorm-folded fp16 launch (streaming tiles and the A-stationary tile 20), on the
two fp8-operand launches, with adversarial values, and through the whole U-Net with the switch on and off."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634

# (tokens per sample, channels) of every self-attention of the U-Net at 512 and 768 whose N is a multiple of 64 (8 heads, d = C / 8)
SHAPES = [(4096, 320), (1024, 640), (256, 1280), (64, 1280), (9216, 320), (2304, 640), (576, 1280)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _same(a, b, what):
    assert a.data.shape == b.data.shape and a.scale.shape == b.scale.shape, what
    bad = (a.data != b.data).sum().item()
    bads = (a.scale != b.scale).sum().item()
    assert bad == 0 and bads == 0, f"{what}: {bad} data bytes and {bads} scales differ"


def _qkv_weights(C, seed, dev):
    from pbe_amd import ops
    g = _g(seed)
    W = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w, c2, c1 = ops.pack_linear_ln(W.to(dev), None, gamma.to(dev), beta.to(dev))
    qscale = (C // 8) ** -0.5 * LOG2E
    c2[:C] *= qscale
    return w, c2, c1, qscale


def _folded_reference(x, stats, w, c2, c1, qscale, B, N, D, eps=1e-5):
    """Today's path: the fp16 projection (q pre-scaled, V^T transposed), then the three quantiser launches."""
    from pbe_amd import ops
    H = x.shape[1] // D
    inner = H * D
    qk = torch.empty((B * N, 2 * inner), dtype=torch.float16, device=x.device)
    vt = torch.empty((B, inner, N), dtype=torch.float16, device=x.device)
    ops.gemm(x, w, c2, ln=(stats, c1, eps), alpha=qscale, alpha_cols=inner, out=qk, vt=vt, vt_col0=2 * inner, vt_tokens=N)
    return (ops.quant_mx8(qk, B, H, N, D, rs=2 * inner), ops.quant_mx8(qk[:, inner:], B, H, N, D, rs=2 * inner),
            ops.quant_mx8(vt, B, H, N, D, rs=N, vt=True))


def _targets(B, H, N, D, dev):
    """(q, k, vt) MX targets pre-filled with a sentinel byte: every byte the reference holds, padding included, must be written."""
    from pbe_amd import ops
    out = []
    for m in (ops.MX8_TOKENS, ops.MX8_TOKENS, ops.MX8_VT):
        t = ops._mx8_target(m, B, H, N, D, dev)
        t.data.fill_(0xA5)
        t.scale.fill_(0xA5)
        out.append(t)
    return tuple(out)


def _mx_plans(fn):
    """Run fn with ops._PLANS recording; return the MX launches' (key, tile, splits, BM, BN, workgroups)."""
    from pbe_amd import ops
    prev, ops._PLANS = ops._PLANS, []
    try:
        out = fn()
        return out, list(ops._PLANS)
    finally:
        ops._PLANS = prev


def _tokens_whole(bn, C, D, half):
    step = bn // 2 if half else bn
    return all((x % D) % 32 == 0 for x in range(step, C, step))


def _folded_case(dev, N, C, B):
    """Every byte of the MX-out projection against the two-launch path; returns the tile that launched."""
    from pbe_amd import ops
    D = C // 8
    g = _g(N + C + B)
    x = (torch.randn(B * N, C, generator=g) * 2 + 0.5).half().to(dev)
    w, c2, c1, qscale = _qkv_weights(C, N + B, dev)
    stats = ops.row_stats(x)
    ref = _folded_reference(x, stats, w, c2, c1, qscale, B, N, D)
    got, plans = _mx_plans(lambda: ops.qkv_mx8(x, w, c2, ln=(stats, c1, 1e-5), B=B, H=8, N=N, D=D, alpha=qscale, alpha_cols=C,
                                               out=_targets(B, 8, N, D, dev)))
    for r, m, what in zip(ref, got, ("q", "k", "vt")):
        _same(r, m, f"{what} N={N} C={C} B={B}")
    (key, cfg, splits, bm, bn, _), = plans
    assert key == f"gx:{B * N}:{3 * C}:{C}:1" and splits == 1
    assert _tokens_whole(bn, C, D, cfg == 20) and (2 * C) % bn == 0, plans
    return cfg


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,C", SHAPES)
def test_folded_projection_bit_identical(dev, N, C, B):
    _folded_case(dev, N, C, B)


@pytest.mark.parametrize("N", [4096, 9216])
def test_folded_projection_a_stationary_tile(dev, N):
    """K = 320 at batch 8 (gx:32768 / gx:73728 :960:320:1): the tuned A-stationary tile 20 launches its MX form (form 2)."""
    assert _folded_case(dev, N, 320, 8) == 20


@pytest.mark.parametrize("N,C,B", [(4096, 320, 2), (1024, 640, 2), (256, 1280, 2), (64, 1280, 2), (4096, 320, 4)])
def test_folded_projection_pinned_batch(dev, N, C, B):
    """run_paired: the batch-B launch takes the MX tile of the batch-2B layer, which keeps every block whole too; same bytes.  B = 4 at
    64x64 is pinned to the batch-8 layer: tile 20."""
    from pbe_amd import ops
    D = C // 8
    g = _g(7 * N + C)
    x = torch.randn(B * N, C, generator=g).half().to(dev)
    w, c2, c1, qscale = _qkv_weights(C, 3 + N, dev)
    stats = ops.row_stats(x)
    ref = _folded_reference(x, stats, w, c2, c1, qscale, B, N, D)

    def run():
        with ops.pinned_batch_scale(2):
            return ops.qkv_mx8(x, w, c2, ln=(stats, c1, 1e-5), B=B, H=8, N=N, D=D, alpha=qscale, alpha_cols=C, out=_targets(B, 8, N, D, dev))
    got, plans = _mx_plans(run)
    for r, m, what in zip(ref, got, ("q", "k", "vt")):
        _same(r, m, f"pinned {what} N={N} C={C}")
    (_, cfg, splits, bm, bn, _), = plans
    x2 = torch.cat([x, x])                            # the plan of the batch-2B layer
    _, plans2 = _mx_plans(lambda: ops.qkv_mx8(x2, w, c2, ln=(ops.row_stats(x2), c1, 1e-5), B=2 * B, H=8, N=N, D=D, alpha=qscale, alpha_cols=C))
    assert cfg == plans2[0][1] and splits == 1 and _tokens_whole(bn, C, D, cfg == 20), (plans, plans2)
    if (N, B) == (4096, 4):
        assert cfg == 20, plans


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,C", SHAPES)
def test_fp8_projections_bit_identical(dev, N, C, B):
    from pbe_amd import ops
    D, H = C // 8, 8
    g = _g(3 * N + C + B)
    x = (torch.randn(B * N, C, generator=g) * 1.5).half().to(dev)
    x8, sx = ops.layernorm_f8(x, (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev), 1e-5)
    wqk8, sqk = ops.pack_linear_f8((torch.randn(2 * C, C, generator=g) / math.sqrt(C)).to(dev))
    wv8, sv = ops.pack_linear_f8((torch.randn(C, C, generator=g) / math.sqrt(C)).to(dev))
    qa = D ** -0.5 * LOG2E
    qk = ops.gemm_f8(x8, sx, wqk8, sqk)
    vt = torch.empty((B, C, N), dtype=torch.float16, device=dev)
    ops.gemm_f8(wv8.unsqueeze(0).expand(B, -1, -1), sv, x8.view(B, N, -1), sx.view(B, N), out=vt)
    ref = (ops.quant_mx8(qk, B, H, N, D, rs=2 * C, alpha=qa), ops.quant_mx8(qk[:, C:], B, H, N, D, rs=2 * C), ops.quant_mx8(vt, B, H, N, D, rs=N, vt=True))
    got, plans = _mx_plans(lambda: ops.qkv_mx8_f8(x8, sx, wqk8, sqk, wv8, sv, B=B, H=H, N=N, D=D, q_alpha=qa, out=_targets(B, H, N, D, dev)))
    for r, m, what in zip(ref, got, ("q", "k", "vt")):
        _same(r, m, f"fp8 {what} N={N} C={C} B={B}")
    assert [p[0] for p in plans] == [f"g8:{B * N}:{2 * C}:{C}:1", f"g8:{C}:{N}:{C}:{B}"]
    assert all(p[2] == 1 for p in plans) and _tokens_whole(plans[0][4], C, D, False) and plans[1][4] % 32 == 0, plans


def _adversarial_rows(rows, width, g):
    """The quantiser tests' adversarial rows: outliers, exact e4m3 ties at amax 448, +-448 saturation, fp16 subnormals, all-zero blocks."""
    x = torch.randn(rows, width, generator=g) * 3
    for r in range(rows):
        kind = r % 6
        if kind == 1:
            x[r, ::32] = 3000.0 * (1 if r % 12 == 1 else -1)
        elif kind == 2:
            vals = torch.tensor([448.0, 1.0625, 1.1875, 17.0, 3 * 2.0 ** -10, 2.0 ** -10, 5 * 2.0 ** -11, -1.0625, -17.0, 240.0, 464.0 - 16])
            x[r] = vals.repeat(width // len(vals) + 1)[:width]
        elif kind == 3:
            x[r] = torch.randn(width, generator=g) * 2.0 ** -20
        elif kind == 4:
            x[r] = 0.0
    return x.half()


@pytest.mark.parametrize("N,C,B", [(4096, 320, 1), (1024, 640, 1), (256, 1280, 1), (4096, 320, 8)])
def test_adversarial_values_bit_identical(dev, N, C, B):
    """Weights [I; I; I] and row statistics of mean 0 / rstd 1 make the projection output the adversarial rows themselves (exact in fp32
    and fp16), in q, k and, transposed, V^T.  B = 8 at 64x64 runs tile 20."""
    from pbe_amd import ops
    D = C // 8
    x = _adversarial_rows(B * N, C, _g(N)).to(dev)
    eye = torch.eye(C, dtype=torch.float16, device=dev)
    w = torch.cat([eye, eye, eye]).contiguous()
    buf = torch.zeros((1, B * N, 2), dtype=torch.float32, device=dev)
    buf[..., 1] = float(C)                            # sum 0, sum of squares C: mean 0, variance 1, rstd = rsq(1 + eps), eps = 0
    stats = ops.RowStats(buf, 1, B * N)
    c1 = torch.zeros(3 * C, dtype=torch.float32, device=dev)
    ref = _folded_reference(x, stats, w, None, c1, 1.0, B, N, D, eps=0.0)
    got, plans = _mx_plans(lambda: ops.qkv_mx8(x, w, None, ln=(stats, c1, 0.0), B=B, H=8, N=N, D=D, alpha=1.0, alpha_cols=C,
                                               out=_targets(B, 8, N, D, dev)))
    if B == 8:
        assert plans[0][1] == 20, plans
    qk = torch.empty((B * N, 2 * C), dtype=torch.float16, device=dev)
    vt = torch.empty((B, C, N), dtype=torch.float16, device=dev)
    ops.gemm(x, w, None, ln=(stats, c1, 0.0), alpha=1.0, alpha_cols=C, out=qk, vt=vt, vt_col0=2 * C, vt_tokens=N)
    assert torch.equal(qk[:, :C], x) and torch.equal(vt[0], x[:N].t())      # the values reach the copy-out unchanged
    for r, m, what in zip(ref, got, ("q", "k", "vt")):
        _same(r, m, f"adversarial {what} N={N} C={C}")
    assert (got[0].scale == 127).any() and (got[0].data.view(-1) == 0x7E).any()


def test_refusals_raise(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    C = 1280
    x = torch.randn(144, C).half().to(dev)
    w, c2, c1, qscale = _qkv_weights(C, 1, dev)
    with pytest.raises(PbeError, match="multiple of 64"):        # the 12x12 mid block at 768 keeps the quantiser path
        ops.qkv_mx8(x, w, c2, ln=(ops.row_stats(x), c1, 1e-5), B=1, H=8, N=144, D=160, alpha=qscale, alpha_cols=C)
    x = torch.randn(256, 512).half().to(dev)
    w, c2, c1, qscale = _qkv_weights(512, 2, dev)
    with pytest.raises(PbeError, match="head dim"):
        ops.qkv_mx8(x, w, c2, ln=(ops.row_stats(x), c1, 1e-5), B=1, H=8, N=256, D=64, alpha=qscale, alpha_cols=512)
    with pytest.raises(PbeError, match="row statistics for every row"):
        ops.qkv_mx8(x, w, c2, ln=(ops.RowStats(torch.zeros((1, 128, 2), device=dev), 1, 128), c1, 1e-5), B=1, H=8, N=256, D=64)


def _launch(d, mx):
    from pbe_amd import lib
    import ctypes as C
    lib.check(lib.load().pbe_gemm_mx8out_f16(C.byref(d), C.byref(mx), torch.cuda.current_stream().cuda_stream), "pbe_gemm_mx8out_f16")


@pytest.mark.parametrize("case", ["qk_only", "k_vt_only", "split_k", "residual", "geglu", "row_stats", "unaligned_tile"])
def test_launch_entry_point_refuses(dev, case):
    """Every refused combination comes back from the launch entry point as PBE_EINVAL (PbeError), before any kernel runs; the targets
    keep their sentinel."""
    from pbe_amd import lib, ops
    from pbe_amd.lib import PbeError
    B, N, C, D = 8, 4096, 320, 40                  # tile 20 where it plans
    x = torch.randn(B * N, C).half().to(dev)
    w, c2, c1, qscale = _qkv_weights(C, 9, dev)
    st = ops.row_stats(x)
    q, k, v = _targets(B, 8, N, D, dev)
    d = lib.GemmDesc(x.data_ptr(), None, w.data_ptr(), None, c2.data_ptr(), None, None, B * N, 3 * C, C, C, C, 0, C, 0, 0, 0, 1, 0, 0, 0, 0, 1,
                     float(qscale), 0, 0, None, 0, 20 | (1 << 8))
    d.alpha_cols, d.ln_stats, d.ln_parts, d.ln_stats_ld, d.ln_colsum, d.ln_eps = C, st.ptr(), st.parts, st.ld, c1.data_ptr(), 1e-5
    d.vt_col0, d.vt_tokens = 2 * C, N
    ranges = [(q, 0, 1.0), (k, C, 1.0), (v, 2 * C, 1.0)]
    other = torch.zeros((B * N, 3 * C), dtype=torch.float16, device=dev)
    msg = {"qk_only": "exactly the q", "k_vt_only": "exactly the q", "split_k": "split-K", "residual": "no residual", "geglu": "no activation",
           "row_stats": "no row statistics", "unaligned_tile": "splits an MX block"}[case]
    if case == "qk_only":
        ranges = ranges[:2]
    elif case == "k_vt_only":
        ranges = ranges[1:]
    elif case == "split_k":
        d.tile_cfg = 9 | (2 << 8)
    elif case == "residual":
        d.resid, d.ldr = other.data_ptr(), 3 * C
    elif case == "geglu":
        d.act = ops.ACT_GEGLU
    elif case == "row_stats":
        d.row_stats_out = other.data_ptr()
    else:
        d.tile_cfg = 3 | (1 << 8)                    # 128 columns: 128 = 3 * 40 + 8
    with pytest.raises(PbeError, match=msg):
        _launch(d, ops._mx8_desc(ranges, False))
    torch.cuda.synchronize()
    assert all((t.data == 0xA5).all() and (t.scale == 0xA5).all() for t in (q, k, v))


@pytest.fixture(scope="module")
def full(dev):
    import modelbuild as build
    with torch.no_grad():
        return build.full_model(dev, parts=("unet",))


def _set_mx8(on):
    from ldm.modules.attention import CrossAttention
    CrossAttention.mx8_from_projection = on


def test_unet_bit_identical_switch_on_off_and_no_quantiser(dev, full, monkeypatch):
    import cases
    from pbe_amd import ops
    from pbe_amd.precision import set_attention_precision, set_linear_precision
    inp = cases.full_inputs()
    x, t, ctx = inp["unet_x"].to(dev), inp["unet_t"].to(dev), inp["unet_ctx"].to(dev)
    g = _g(5)
    xp = torch.randn(2, 9, 64, 64, generator=g).to(dev)
    cp = torch.randn(4, 1, 768, generator=g).to(dev)
    tp = torch.full((4,), 621, dtype=torch.int64, device=dev)
    unet = full.model.diffusion_model
    n = {"quant_mx8": 0, "attention_mx8": 0}
    for name in n:
        fn = getattr(ops, name)

        def wrap(*a, _fn=fn, _name=name, **kw):
            n[_name] += 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    out = {}
    with torch.no_grad():
        try:
            set_attention_precision(full, "fp8")
            for lin in ("fp16", "fp8"):
                set_linear_precision(full, lin)
                for on in (True, False):
                    _set_mx8(on)
                    n.update(quant_mx8=0, attention_mx8=0)
                    y = full.apply_model(x, t, ctx)
                    assert n == ({"quant_mx8": 0, "attention_mx8": 16} if on else {"quant_mx8": 48, "attention_mx8": 16}), (lin, on, n)
                    n.update(quant_mx8=0, attention_mx8=0)
                    yp = unet.forward_nhwc(ops.plms_pack_input(xp[:, :4], xp[:, 4:8], xp[:, 8:], 1), tp, cp, paired=True)
                    assert n["attention_mx8"] == 16 and (n["quant_mx8"] == 0) == on, (lin, on, n)
                    out[(lin, on)] = (y, yp)
        finally:
            _set_mx8(True)
            set_attention_precision(full, "fp16")
            set_linear_precision(full, "fp16")
    for lin in ("fp16", "fp8"):
        (a, ap), (b, bp) = out[(lin, True)], out[(lin, False)]
        assert torch.isfinite(a).all() and torch.equal(a, b), f"run, linear {lin}"
        assert torch.isfinite(ap).all() and torch.equal(ap, bp), f"run_paired, linear {lin}"
