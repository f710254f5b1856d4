"""Multi-token cross-attention on the GPU: pbe_ctx_attention_f16 against the fp64 reference of tests/ctxref.py (gate: rel-L2 <=
REL_L2_FACTOR x the fp32 emulation's, and the whole-tensor limit CLOSE["attention"]), its padding / bounds / reproducibility contract, and
the block, U-Net, sampler and CLI paths that accept a context of several tokens against the CPU oracle (oracle/pbe_oracle.py)."""
import os

import numpy as np
import pytest
import torch

import cases
import ctxref
import guard
import modelbuild as build
from accgate import CLOSE, close_verdict, rel_l2
from oracle_loader import O
from test_accuracy_gpu import report as accuracy_report
from test_model_gpu import BLOCK_TOL, FWD_TOL, SAMPLER_OPT_TOL, report      # the project's tolerances and its parity report (same file, same format)

pytestmark = pytest.mark.gpu


def check(name, got, ref, tol):
    got = got.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    v = rel_l2(got, ref.double())
    report(name, v, tol)
    assert v <= tol, f"{name}: rel-L2 {v:.3e} > {tol:.1e}"


def _device_operands(o, dev):
    """(x, ops.CtxOperands, RowStats) on the GPU from ctxref.Operands; vo rows padded to a multiple of 8 columns (zeros)."""
    from pbe_amd import ops
    HJ = o.H * o.Nk
    vo = torch.zeros(o.B, o.C, (HJ + 7) // 8 * 8, dtype=torch.float16)
    vo[:, :, :HJ] = o.vo
    st = o.stats.to(dev).contiguous()
    return o.x.to(dev), ops.CtxOperands(o.kq.to(dev), o.colsum.to(dev), o.kbias.to(dev), vo.to(dev), o.bias.to(dev), o.H, o.Nk), \
        ops.RowStats(st, st.shape[0], st.shape[1])


def _gate(name, got, o):
    want, emu = ctxref.reference(o)[0], ctxref.emulate(o)
    ok, text = ctxref.verdict(got.cpu(), want, emu)
    r = rel_l2(got.cpu(), want)
    report(f"ctx_attention {name}", r, ctxref.REL_L2_FACTOR * rel_l2(emu, want))
    print(f"ctx_attention {name}: {text}")
    assert ok, f"{name}: {text}"
    import ctxgate                                                           # beside it: every element within its own bound (tests/ctxgate.py)
    v = ctxgate.verdict(got, o, emu=emu)
    accuracy_report(f"{'ctx_attention ' + name:64s} err/bound={v.ratio:.3f} at {v.where} rel_l2={v.r_got:.3e} (emulation {v.r_emu:.3e})")
    assert v.ok, f"{name}: {v}"


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C,H,Nk,parts", ctxref.KERNEL_SHAPES, ids=lambda v: str(v))
def test_kernel_against_fp64_reference(dev, B, N, C, H, Nk, parts):
    from pbe_amd import ops
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=1)
    x, oc, st = _device_operands(o, dev)
    y, rs = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N)
    _gate(f"B{B} N{N} C{C} H{H} Nk{Nk} parts{parts}", y, o)
    # row statistics: (sum, sumsq) of the STORED fp16 rows, one partial (limits of test_gemm_row_statistics_epilogue)
    assert rs.parts == 1
    want = torch.stack([y.double().sum(1), (y.double() ** 2).sum(1)], 1).cpu()
    assert torch.allclose(rs.buf[0].double().cpu(), want, rtol=2e-6, atol=1e-4), (rs.buf[0].double().cpu() - want).abs().max()
    one = ops.row_stats(y)
    assert torch.allclose(one.buf[0].double().cpu(), want, rtol=2e-6, atol=1e-4)
    # run to run: bit-identical
    y2, rs2 = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N)
    assert torch.equal(y, y2) and torch.equal(rs.buf, rs2.buf)


def test_kernel_large_logits(dev):
    """Scores of about +-200 log2 units: finite, and the same gate (the group maximum is subtracted before exp2)."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = ctxref.LARGE_LOGITS_SHAPE
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=3, logit_scale=60.0)
    xd = o.x.double().view(B, N, C)
    xh = (xd - xd.mean(-1, keepdim=True)) / xd.std(-1, unbiased=False, keepdim=True)
    peak = (xh @ o.kq.double().transpose(1, 2) + o.kbias.double()[:, None]).abs().max().item()
    assert 150 <= peak <= 400, peak
    x, oc, st = _device_operands(o, dev)
    y, _ = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N)
    assert torch.isfinite(y).all()
    _gate("large logits", y, o)


def test_kernel_ignores_padding_and_stays_in_bounds(dev):
    """Every operand inside a poisoned arena (NaN in the leading-dimension padding, before and after), Y and the statistics inside
    sentinel arenas: the result passes the gate, is fully written, and nothing outside Y / the statistics is touched.  N = 72: the
    second row tile of every sample ends in the middle of a tile."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = 2, 72, 320, 5, 5, 1          # HJ = 25: the last 16-byte chunk of a Vo row is partly padding
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=5)
    M, HJ = B * N, H * Nk
    x, _ = guard.embed(o.x, col_pad=24, device=dev)
    kq, _ = guard.embed(o.kq, row_pad=3, col_pad=8, device=dev)
    vo, _ = guard.embed(o.vo, row_pad=2, col_pad=0, device=dev)                # ld = 32: columns 25 .. 31 of every row hold NaN
    colsum, _ = guard.embed(o.colsum, col_pad=3, device=dev)
    kbias, _ = guard.embed(o.kbias, col_pad=3, device=dev)
    bias, _ = guard.embed(o.bias, device=dev)
    stats, _ = guard.embed(o.stats.reshape(-1), device=dev)
    y, y_arena = guard.sentinel_out((M, C), col_pad=40, device=dev)
    rs, rs_arena = guard.sentinel_out((2 * M,), dtype=torch.float32, device=dev)
    for v in (x, kq, vo, y):
        guard.assert_aligned(v)
    oc = ops.CtxOperands(kq, colsum, kbias, vo, bias, H, Nk)
    got, _ = ops.ctx_attention(x, oc, ops.RowStats(stats.view(1, M, 2), 1, M), ctxref.EPS, tokens=N, out=y, row_stats=ops.RowStats(rs.view(1, M, 2), 1, M))
    torch.cuda.synchronize()
    guard.assert_fully_written(y, "ctx_attention Y")
    guard.assert_fully_written(rs, "ctx_attention row statistics")
    guard.assert_untouched(y_arena, y, "ctx_attention Y")
    guard.assert_untouched(rs_arena, rs, "ctx_attention row statistics")
    _gate("poisoned padding", y.contiguous(), o)
    # a launch over the first sample only (M ends in the middle of the second row tile) leaves the second sample's rows alone
    y1, y1_arena = guard.sentinel_out((M, C), device=dev)
    ops.ctx_attention(x[:N], oc.rows(0, 1), ops.RowStats(stats.view(1, M, 2), 1, M), ctxref.EPS, tokens=N, out=y1[:N], row_stats=False)
    torch.cuda.synchronize()
    guard.assert_untouched(y1_arena, y1[:N], "ctx_attention Y (one sample)")
    assert torch.equal(y1[:N], y[:N])


def test_one_token_equals_rowvec_path(dev):
    """Nk = 1: the softmax is 1 and the kernel reduces to the constant the one-token path adds in the out-projection epilogue:
    gemm(a, Wo, bo, rowvec=single_token_context, resid=x) == ctx_attention(gemm(a, Wo, bo, resid=x)) within CLOSE["attention"]."""
    from ldm.modules.attention import BasicTransformerBlock
    from pbe_amd import ops
    from pbe_amd.weights import fill_module_
    B, N, C, H = 3, 8, 128, 8
    blk = BasicTransformerBlock(C, H, C // H, context_dim=768)
    fill_module_(blk, prefix="blk.")
    blk = blk.to(dev)
    g = torch.Generator().manual_seed(9)
    a = torch.randn(B * N, C, generator=g).half().to(dev)
    x = torch.randn(B * N, C, generator=g).half().to(dev)
    ctx = torch.randn(B, 1, 768, generator=g).half().to(dev)
    with torch.no_grad():
        a1 = blk.attn1.pk()
        old = ops.gemm(a, a1.wo, a1.bo, rowvec=blk.attn2.single_token_context(ctx), group_rows=N, resid=x)
        x1, st = ops.gemm(a, a1.wo, a1.bo, resid=x, row_stats=True)
        new, _ = ops.ctx_attention(x1, blk._fused_operands(ctx), st, blk.norm2.eps, tokens=N)
    ok, err, lim = close_verdict(new.cpu(), old.double().cpu(), CLOSE["attention"])
    assert ok, f"Nk = 1 vs the rowvec path: max|d| {err:.3e} > {lim:.3e}"


# ---- blocks and the narrow model against the oracle ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def narrow_sd(narrow):
    return {k: v.detach().float().cpu() for k, v in narrow.state_dict().items()}


def _st(C, H, dev, tag):
    from ldm.modules.attention import SpatialTransformer
    from pbe_amd.weights import fill_module_
    st = SpatialTransformer(C, H, C // H, depth=1, context_dim=768)
    fill_module_(st, prefix=tag)
    torch.nn.init.normal_(st.proj_out.weight, std=0.05)                      # (zero_module: the block would not reach the output)
    sd = {tag + k: v.detach().float() for k, v in st.state_dict().items()}
    return st.to(dev), sd


@pytest.mark.parametrize("C,H", [(64, 8), (320, 8), (1280, 8)])
def test_spatial_transformer_multi_token_against_oracle(dev, C, H):
    """4 context tokens; C = 1280 lies beyond the measured dispatch bound of the fused kernel and takes the existing kernels."""
    st, sd = _st(C, H, dev, "st.")
    assert st.transformer_blocks[0]._ctx_fused(4) == (C <= 640)
    g = torch.Generator().manual_seed(C)
    x, ctx = torch.randn(2, C, 8, 8, generator=g), torch.randn(2, 4, 768, generator=g)
    with torch.no_grad():
        want = O.spatial_transformer(sd, "st.", x, ctx, H)
        got = st(x.to(dev), ctx.to(dev))
    check(f"SpatialTransformer C={C}, 4-token context", got, want, BLOCK_TOL)


def test_route_by_context_length(dev):
    """16 tokens take the fused kernel, 20 the q projection / pbe_attention_f16 / to_out route; both agree with the oracle, and the
    recorded launch keys show which ran."""
    from pbe_amd import ops
    C, H = 320, 8
    st, sd = _st(C, H, dev, "st.")
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, C, 8, 8, generator=g)
    for K, fused in ((16, True), (20, False)):
        ctx = torch.randn(2, K, 768, generator=g)
        with torch.no_grad():
            want = O.spatial_transformer(sd, "st.", x, ctx, H)
            ops._TIMES = {}
            try:
                got = st(x.to(dev), ctx.to(dev))
                keys = list(ops._TIMES)
            finally:
                ops._TIMES = None
        check(f"SpatialTransformer C={C}, {K}-token context", got, want, BLOCK_TOL)
        assert any(k.startswith("xa:") for k in keys) == fused, keys
        assert any(k.startswith(f"a:2:{H}:64:{K}:") for k in keys) == (not fused), keys


def test_narrow_unet_forward_multi_token(dev, narrow, narrow_sd):
    inp = cases.narrow_inputs()
    g = torch.Generator().manual_seed(404)
    ctx = torch.randn(4, 3, 768, generator=g)
    sd = {k[len("model.diffusion_model."):]: v for k, v in narrow_sd.items() if k.startswith("model.diffusion_model.")}
    with torch.no_grad():
        want = O.unet_forward(sd, inp["unet_x"], inp["unet_t"], ctx, cases.UNET_NARROW)
        got = narrow.apply_model(inp["unet_x"].to(dev), inp["unet_t"].to(dev), ctx.to(dev))
        one = narrow.apply_model(inp["unet_x"].to(dev), inp["unet_t"].to(dev), ctx[:, :1].to(dev))
        rep = narrow.apply_model(inp["unet_x"].to(dev), inp["unet_t"].to(dev), ctx[:, :1].expand(-1, 4, -1).contiguous().to(dev))
    check("narrow UNetModel forward, 3-token context", got, want, FWD_TOL)
    check("narrow UNetModel: 4 copies of one token vs the one-token path", rep, one.float().cpu(), FWD_TOL)


def test_narrow_paired_prefix_is_bit_identical_multi_token(dev, narrow):
    """forward_nhwc(paired=True) with a 3-token context against the duplicated 2B evaluation (test_full_unet_shared_guidance_prefix at
    narrow size): the shared part now reaches to attn1's output projection, the halves part at the ctx_attention launch."""
    from pbe_amd import ops
    g = torch.Generator().manual_seed(6)
    unet = narrow.model.diffusion_model
    for B, K in ((2, 3), (1, 3), (2, 20)):                  # 20 tokens: the halves part at the existing-kernel route instead
        x = torch.randn(B, 4, 16, 16, generator=g).to(dev)
        z = torch.randn(B, 4, 16, 16, generator=g).to(dev)
        m = (torch.rand(B, 1, 16, 16, generator=g) > 0.3).float().to(dev)
        ctx = torch.randn(2 * B, K, 768, generator=g).to(dev)
        t = torch.full((2 * B,), 621, dtype=torch.int64, device=dev)
        with torch.no_grad():
            a = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 2), t, ctx)
            b = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 1), t, ctx, paired=True)
        assert torch.equal(a, b), f"B={B} K={K}: {int((a != b).sum())} of {a.numel()} elements differ"
        assert not torch.equal(b[:B], b[B:])


def test_narrow_plms_multi_token_against_oracle(dev, narrow, narrow_sd, golden_dir):
    """4 PLMS steps at scale 5, a 3-token conditioning (three exemplars through the CLIP path) and the one-token learnable vector as the
    unconditional context; the oracle is handed the vector repeated to 3 tokens (exact: test_repeated_token_equals_single_token)."""
    from ldm.models.diffusion.plms import PLMSSampler
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    z_inp, m = torch.from_numpy(gold["z_inpaint"]), torch.from_numpy(gold["mask_lat"])
    g = torch.Generator().manual_seed(8)
    refs = torch.randn(2, 3, 3, 224, 224, generator=g)
    with torch.no_grad():
        c = narrow.proj_out(narrow.get_learned_conditioning(refs.to(dev)))
        assert c.shape == (2, 3, 768)
        c1 = narrow.proj_out(narrow.get_learned_conditioning(refs[:, 1].to(dev)))
        assert torch.equal(c[:, 1:2], c1)                                        # each exemplar is encoded on its own
        z0, _ = PLMSSampler(narrow).sample(S=4, batch_size=2, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                                           unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
                                           test_model_kwargs={"inpaint_image": z_inp.to(dev), "inpaint_mask": m.to(dev)})
        sd = {k[len("model.diffusion_model."):]: v for k, v in narrow_sd.items() if k.startswith("model.diffusion_model.")}
        uc = narrow_sd["learnable_vector"].expand(2, 3, -1)
        want, info = O.plms_sample(lambda x9, t, ctx: O.unet_forward(sd, x9, t, ctx, cases.UNET_NARROW), 4, inp["x_T"], c.float().cpu(), uc, 5.0,
                                   z_inp, m, O.schedule_buffers()["alphas_cumprod"])
    assert info["calls"] == 5
    check("narrow PLMS 4 steps, 3-token c / one-token uc", z0, want, SAMPLER_OPT_TOL)


def test_inference_cli_two_references(dev, golden_dir, tmp_path):
    """scripts/inference.py with two --reference_path images on bundled example 1 (2 steps, narrow weights, as
    test_inference_cli_matches_oracle_pipeline builds them): the PNG against the oracle pipeline fed the same two context tokens."""
    import importlib.util
    import yaml
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbe_inference_cli", os.path.join(root, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    d = os.path.join(golden_dir, "examples")
    img_p, msk_p = os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png")
    ref_p = [os.path.join(d, "reference_example_1.jpg"), os.path.join(d, "reference_example_2.jpg")]
    cfg, dump, steps, seed = str(tmp_path / "narrow.yaml"), str(tmp_path / "dump.npz"), 2, 321
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)
    out = cli.main(["--plms", "--outdir", str(tmp_path), "--config", cfg, "--ddim_steps", str(steps), "--image_path", img_p, "--mask_path", msk_p,
                    "--reference_path", ref_p[0], ref_p[1], "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights", "--dump_tensors", dump])
    t = np.load(dump)
    assert t["c"].shape == (1, 2, 768)
    img = np.asarray(Image.open(img_p).convert("RGB"))
    msk = np.asarray(Image.open(msk_p).convert("L"))
    model = build.narrow_model("cpu")
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    with torch.no_grad():
        cs = []
        for p in ref_p:
            oi, _, om, oref = O.preprocess_triple(img, msk, np.asarray(Image.open(p).convert("RGB").resize((224, 224))))
            cs.append(O.learned_conditioning(sd, oref, cases.CLIP_NARROW, cases.MAPPER_NARROW))
        c = torch.cat(cs, 1)
        z_inp = O.first_stage_encode(sd, oi * om, torch.from_numpy(t["post_eps"]), cases.VAE_NARROW, "first_stage_model.")
        m64 = O.resize_mask(om, z_inp.shape[-2:])
        usd = {k[len("model.diffusion_model."):]: v for k, v in sd.items() if k.startswith("model.diffusion_model.")}
        z0, info = O.plms_sample(lambda x9, tt, ctx: O.unet_forward(usd, x9, tt, ctx, cases.UNET_NARROW), steps, torch.from_numpy(t["x_T"]), c,
                                 sd["learnable_vector"].float().expand(1, 2, -1), 5.0, z_inp, m64, O.schedule_buffers()["alphas_cumprod"])
        image = torch.clamp((O.first_stage_decode(sd, z0, cases.VAE_NARROW, "first_stage_model.") + 1.0) / 2.0, 0.0, 1.0)
    assert info["calls"] == steps + 1
    check("CLI two references: conditioning c", torch.from_numpy(t["c"]), c, 4e-3)
    check("CLI two references: final latent (2 PLMS steps)", torch.from_numpy(t["latent"]), z0, 8e-3)
    png = np.asarray(Image.open(os.path.join(str(tmp_path), "results", f"image_example_1_{seed}.png"))).astype(np.float32)
    exp = (255.0 * image[0].permute(1, 2, 0).numpy()).astype(np.uint8).astype(np.float32)
    mad = float(np.abs(png - exp).mean())
    report("CLI two references: result PNG vs oracle, mean |d| in grey levels", mad, 0.55)
    assert png.shape == (512, 512, 3) and mad <= 0.55
    assert torch.equal(out, torch.from_numpy(t["image"]))
