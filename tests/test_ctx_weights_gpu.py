"""Exemplar weights and per-sample exemplar counts on the GPU: pbe_ctx_attention_w_f16 against the fp64 reference of tests/ctxref.py
with log2 w folded into its kbias (tests/kbiasref.py), and the block, U-Net, sampler and CLI paths that take the weights against the
CPU oracle run per sample on the equivalent context - weight-0 tokens removed, integer-weighted tokens repeated."""
import os

import numpy as np
import pytest
import torch

import cases
import ctxref
import guard
import kbiasref as kr
import modelbuild as build
from oracle_loader import O
from test_ctx_attention_gpu import _device_operands, _gate, _st, check
from test_model_gpu import BLOCK_TOL, FWD_TOL, SAMPLER_OPT_TOL, report

pytestmark = pytest.mark.gpu

W4 = [[2.0, 1.0, 0.0, 3.0], [0.0, 0.0, 1.0, 0.0]]          # sample 0: [t0, t0, t1, t3, t3, t3]; sample 1: [t2]
EQ4 = [[0, 0, 1, 3, 3, 3], [2]]


def _keys(fn):
    from pbe_amd import ops
    ops._TIMES = {}
    try:
        out = fn()
        return out, list(ops._TIMES)
    finally:
        ops._TIMES = None


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", kr.CTX_SHAPES, ids=lambda s: "B%d-N%d-C%d-H%d-K%d-p%d" % s)
def test_weighted_kernel_against_fp64_reference(dev, shape):
    """exp2(3 randn) weights on the first 1 / 3 / 5 tokens of the samples, 0 on the rest, against ctxref.reference on kbias + log2 w."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts)
    w = kr.ctx_weights(B, Nk, 11 + C)
    x, oc, st = _device_operands(o, dev)
    oc.log2w = torch.log2(w).float().to(dev)
    (y, _), keys = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N))
    assert keys == [f"xaw:{B * N}:{C}:{H}:{Nk}"], keys
    _gate(f"weighted B{B} N{N} C{C} H{H} Nk{Nk} parts{parts}", y, kr.fold_log2w(o, w, through_fp32=True))
    # the folded operands do not depend on the weights: the same operands with other weights, no re-folding
    w2 = kr.ctx_weights(B, Nk, 99 + C, counts=(Nk, 2, 1))
    oc.log2w = torch.log2(w2).float().to(dev)
    y2, _ = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N)
    _gate(f"weighted (second weights) B{B} N{N} C{C} H{H} Nk{Nk}", y2, kr.fold_log2w(o, w2, through_fp32=True))


@pytest.mark.parametrize("shape", kr.CTX_SHAPES, ids=lambda s: "B%d-N%d-C%d-H%d-K%d-p%d" % s)
def test_all_ones_weights_are_bit_identical(dev, shape):
    from pbe_amd import ops
    B, N, C, H, Nk, parts = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts)
    x, oc, st = _device_operands(o, dev)
    (plain, rs0), k0 = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N))
    oc.log2w = torch.zeros(B, Nk, device=dev)
    (ones, rs1), k1 = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N))
    assert k0 == [f"xa:{B * N}:{C}:{H}:{Nk}"] and k1 == [f"xaw:{B * N}:{C}:{H}:{Nk}"]
    assert torch.equal(plain, ones) and torch.equal(rs0.buf, rs1.buf)


def test_weighted_kernel_ignores_padding_and_stays_in_bounds(dev):
    """log2 w sliced out of a NaN-poisoned arena, Y between sentinels; a NaN inside [B, Nk] does reach that sample (positive control)."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = 2, 72, 320, 5, 5, 1
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=5)
    w = kr.ctx_weights(B, Nk, 5, counts=(3, 5))
    x, oc, st = _device_operands(o, dev)
    lw, _ = guard.embed(torch.log2(w).float(), col_pad=3, row_pad=1, device=dev)
    oc.log2w = lw
    y, arena = guard.sentinel_out((B * N, C), col_pad=40, device=dev)
    ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, out=y, row_stats=False)
    torch.cuda.synchronize()
    guard.assert_fully_written(y, "weighted ctx_attention Y")
    guard.assert_untouched(arena, y, "weighted ctx_attention Y")
    _gate("weighted, poisoned padding", y.contiguous(), kr.fold_log2w(o, w, through_fp32=True))
    bad = torch.log2(w).float()
    bad[1, 0] = float("nan")
    oc.log2w = bad.to(dev)
    yb, _ = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, row_stats=False)
    assert torch.isfinite(yb[:N]).all() and not torch.isfinite(yb[N:]).any()


def test_weighted_launch_refuses_bad_weights(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    B, N, C, H, Nk, parts = kr.CTX_SHAPES[0]
    x, oc, st = _device_operands(ctxref.random_operands(B, N, C, H, Nk, parts), dev)
    for bad in (torch.zeros(B, Nk + 1, device=dev), torch.zeros(B, Nk, device=dev, dtype=torch.float16), torch.zeros(B, Nk)):
        oc.log2w = bad
        with pytest.raises(PbeError):
            ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N)


# ---- blocks against the oracle ---------------------------------------------------------------------------------------------------------
def _oracle_per_sample(fn, ctx, eq):
    """fn(b, context [1, K', Dc]) for every sample b on its equivalent context (the listed tokens), concatenated."""
    return torch.cat([fn(b, ctx[b:b + 1, eq[b]]) for b in range(ctx.shape[0])])


@pytest.mark.parametrize("C,H", [(64, 8), (320, 8), (1280, 8)])
def test_spatial_transformer_weighted_against_oracle(dev, C, H):
    """4 tokens, weights (2, 1, 0, 3) / (0, 0, 1, 0): the oracle sees [t0, t0, t1, t3, t3, t3] and [t2].  The weighted fused kernel runs at
    C <= 640, the key-bias attention kernel at C = 1280."""
    st, sd = _st(C, H, dev, "st.")
    g = torch.Generator().manual_seed(C)
    x, ctx = torch.randn(2, C, 8, 8, generator=g), torch.randn(2, 4, 768, generator=g)
    with torch.no_grad():
        want = _oracle_per_sample(lambda b, c: O.spatial_transformer(sd, "st.", x[b:b + 1], c, H), ctx, EQ4)
        got, keys = _keys(lambda: st(x.to(dev), ctx.to(dev), context_weights=torch.tensor(W4)))
    check(f"SpatialTransformer C={C}, weighted 4-token context", got, want, BLOCK_TOL)
    fused = C <= 640
    assert any(k.startswith("xaw:") for k in keys) == fused, keys
    assert any(k.startswith(f"ab:2:{H}:64:4:") for k in keys) == (not fused), keys
    assert not any(k.startswith("xa:") or k.startswith(f"a:2:{H}:64:4:") for k in keys), keys


def test_twenty_tokens_with_counts_take_the_key_bias_route(dev):
    from ldm.modules.attention import prepare_context_weights  # noqa: F401  (the public helper exists)
    C, H, K = 320, 8, 20
    st, sd = _st(C, H, dev, "st.")
    g = torch.Generator().manual_seed(78)
    x, ctx = torch.randn(2, C, 8, 8, generator=g), torch.randn(2, K, 768, generator=g)
    counts = (20, 7)
    w = (torch.arange(K)[None, :] < torch.tensor(counts)[:, None]).double()
    with torch.no_grad():
        want = _oracle_per_sample(lambda b, c: O.spatial_transformer(sd, "st.", x[b:b + 1], c, H), ctx, [list(range(n)) for n in counts])
        got, keys = _keys(lambda: st(x.to(dev), ctx.to(dev), context_weights=w))
    check(f"SpatialTransformer C={C}, 20-token context with counts {counts}", got, want, BLOCK_TOL)
    assert any(k.startswith(f"ab:2:{H}:64:{K}:") for k in keys) and not any(k.startswith("xa") for k in keys), keys


def test_linear_fp8_still_refuses_a_multi_token_context(dev):
    from pbe_amd.lib import PbeError
    st, _ = _st(64, 8, dev, "st.")
    blk = st.transformer_blocks[0]
    blk.linear_fp8 = True
    try:
        with pytest.raises(PbeError):
            blk.context_operands(torch.randn(2, 4, 768).to(dev), torch.tensor(W4))
    finally:
        blk.linear_fp8 = False


# ---- the narrow model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def narrow_sd(narrow):
    return {k: v.detach().float().cpu() for k, v in narrow.state_dict().items()}


def _unet_sd(narrow_sd):
    return {k[len("model.diffusion_model."):]: v for k, v in narrow_sd.items() if k.startswith("model.diffusion_model.")}


def test_narrow_unet_forward_ragged_batch(dev, narrow, narrow_sd):
    """A padded ragged batch, 4 samples with 3 / 1 / 2 / 3 tokens (pipeline.pad_conditionings), against the oracle per sample; the
    count-1 sample against today's one-token path."""
    from pbe_amd.pipeline import pad_conditionings
    inp = cases.narrow_inputs()
    g = torch.Generator().manual_seed(405)
    conds = [torch.randn(k, 768, generator=g) for k in (3, 1, 2, 3)]
    ctx, w = pad_conditionings(conds)
    assert tuple(ctx.shape) == (4, 3, 768)
    sd = _unet_sd(narrow_sd)
    x, t = inp["unet_x"], inp["unet_t"]
    with torch.no_grad():
        want = torch.cat([O.unet_forward(sd, x[b:b + 1], t[b:b + 1], conds[b][None], cases.UNET_NARROW) for b in range(4)])
        got = narrow.apply_model(x.to(dev), t.to(dev), ctx.to(dev), context_weights=w)
        one = narrow.apply_model(x[1:2].to(dev), t[1:2].to(dev), conds[1][None].to(dev))
    check("narrow UNetModel forward, ragged batch 3 / 1 / 2 / 3 tokens", got, want, FWD_TOL)
    check("narrow UNetModel: the count-1 sample of the ragged batch vs the one-token path", got[1:2], one.float().cpu(), FWD_TOL)


def test_context_cache_key_includes_the_weights(dev, narrow):
    """The same context tensor with two different weight tensors: different outputs, each equal to a freshly built model's."""
    inp = cases.narrow_inputs()
    g = torch.Generator().manual_seed(406)
    ctx = torch.randn(4, 3, 768, generator=g).to(dev)
    x, t = inp["unet_x"].to(dev), inp["unet_t"].to(dev)
    wa = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.5, 3.0]])
    wb = torch.tensor([[1.0, 0.0, 2.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [4.0, 0.5, 0.0]])
    with torch.no_grad():
        a = narrow.apply_model(x, t, ctx, context_weights=wa)
        b = narrow.apply_model(x, t, ctx, context_weights=wb)
        a2 = narrow.apply_model(x, t, ctx, context_weights=wa)
        plain = narrow.apply_model(x, t, ctx)
        wa.mul_(2.0)                                          # in place: another version of the same tensor (uniform scaling: same result to rounding)
        a3 = narrow.apply_model(x, t, ctx, context_weights=wa)
        wa.div_(2.0)
        fresh = build.narrow_model(dev)
        fa = fresh.apply_model(x, t, ctx, context_weights=wa)
        fresh = build.narrow_model(dev)
        fb = fresh.apply_model(x, t, ctx, context_weights=wb)
    assert not torch.equal(a, b) and not torch.equal(a, plain)
    assert torch.equal(a, fa) and torch.equal(b, fb) and torch.equal(a, a2)
    assert torch.isfinite(a3.float()).all()


def test_narrow_paired_prefix_is_bit_identical_weighted(dev, narrow):
    """forward_nhwc(paired=True) with weights against the duplicated 2B evaluation, on both routes (3 tokens: the weighted fused kernel;
    20 tokens: the key-bias attention kernel)."""
    from pbe_amd import ops
    g = torch.Generator().manual_seed(7)
    unet = narrow.model.diffusion_model
    for B, K in ((2, 3), (2, 20)):
        x = torch.randn(B, 4, 16, 16, generator=g).to(dev)
        z = torch.randn(B, 4, 16, 16, generator=g).to(dev)
        m = (torch.rand(B, 1, 16, 16, generator=g) > 0.3).float().to(dev)
        ctx = torch.randn(2 * B, K, 768, generator=g).to(dev)
        w = torch.exp2(2.0 * torch.randn(2 * B, K, generator=g, dtype=torch.float64))
        w[:, K - 1] = 0.0
        w[1, 1:] = 0.0
        t = torch.full((2 * B,), 621, dtype=torch.int64, device=dev)
        with torch.no_grad():
            a = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 2), t, ctx, context_weights=w)
            b = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 1), t, ctx, paired=True, context_weights=w)
            plain = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 2), t, ctx)
        assert torch.equal(a, b), f"B={B} K={K}: {int((a != b).sum())} of {a.numel()} elements differ"
        assert not torch.equal(a, plain)


def _ragged_conditioning(narrow, dev):
    """Two samples through the CLIP path: 3 exemplars with weights (2, 1, 0) and (0, 0, 1) -> the oracle's [t0, t0, t1] and [t2]."""
    g = torch.Generator().manual_seed(8)
    refs = torch.randn(2, 3, 3, 224, 224, generator=g)
    c = narrow.proj_out(narrow.get_learned_conditioning(refs.to(dev)))
    return c, torch.tensor([[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), [[0, 0, 1], [2]]


@pytest.mark.parametrize("which", ["plms", "ddim"])
def test_narrow_samplers_weighted_against_oracle(dev, narrow, narrow_sd, golden_dir, which):
    """4 steps at scale 5, ragged conditioning with weights, against the oracle sampler per sample on the equivalent repeated / removed
    contexts (the one-token unconditional vector repeated to each sample's length: exact)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    z_inp, m = torch.from_numpy(gold["z_inpaint"]), torch.from_numpy(gold["mask_lat"])
    sd = _unet_sd(narrow_sd)
    ac = O.schedule_buffers()["alphas_cumprod"]
    model = lambda x9, t, ctx: O.unet_forward(sd, x9, t, ctx, cases.UNET_NARROW)      # noqa: E731
    with torch.no_grad():
        c, w, eq = _ragged_conditioning(narrow, dev)
        cls = PLMSSampler if which == "plms" else DDIMSampler
        z0, _ = cls(narrow).sample(S=4, batch_size=2, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                                   unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
                                   test_model_kwargs={"inpaint_image": z_inp.to(dev), "inpaint_mask": m.to(dev)}, conditioning_weights=w)
        cc = c.float().cpu()
        osample = O.plms_sample if which == "plms" else O.ddim_sample
        want = torch.cat([osample(model, 4, inp["x_T"][b:b + 1], cc[b:b + 1, eq[b]], narrow_sd["learnable_vector"].expand(1, len(eq[b]), -1), 5.0,
                                  z_inp[b:b + 1], m[b:b + 1], ac)[0] for b in range(2)])
    check(f"narrow {which.upper()} 4 steps, ragged weighted conditioning", z0, want, SAMPLER_OPT_TOL)


def test_sampler_refuses_bad_weights(dev, narrow, golden_dir):
    from ldm.models.diffusion.plms import PLMSSampler
    from pbe_amd.lib import PbeError
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    kw = dict(S=2, batch_size=2, shape=[4, 16, 16], conditioning=torch.randn(2, 3, 768).to(dev), verbose=False, unconditional_guidance_scale=5.0,
              unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
              test_model_kwargs={"inpaint_image": torch.from_numpy(gold["z_inpaint"]).to(dev), "inpaint_mask": torch.from_numpy(gold["mask_lat"]).to(dev)})
    for bad in ([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], [[1.0, -1.0, 1.0], [1.0, 1.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]):
        with pytest.raises(PbeError):
            PLMSSampler(narrow).sample(conditioning_weights=bad, **kw)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def _cli():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_w", os.path.join(root, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_inference_cli_reference_weight(dev, golden_dir, tmp_path):
    """Two references with --reference_weight 2 1 against the oracle pipeline fed [r0, r0, r1] (the limits of
    test_inference_cli_two_references), and --reference_weight 1 0 against the single-reference run."""
    import yaml
    from PIL import Image
    cli = _cli()
    d = os.path.join(golden_dir, "examples")
    img_p, msk_p = os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png")
    ref_p = [os.path.join(d, "reference_example_1.jpg"), os.path.join(d, "reference_example_2.jpg")]
    cfg, steps, seed = str(tmp_path / "narrow.yaml"), 2, 321
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)

    def run(tag, refs, extra):
        out, dump = str(tmp_path / tag), str(tmp_path / f"{tag}.npz")
        x = cli.main(["--plms", "--outdir", out, "--config", cfg, "--ddim_steps", str(steps), "--image_path", img_p, "--mask_path", msk_p,
                      "--reference_path", *refs, "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights", "--dump_tensors", dump] + extra)
        return x, np.load(dump), out
    out, t, outdir = run("w21", ref_p, ["--reference_weight", "2", "1"])
    assert t["c"].shape == (1, 2, 768) and t["reference_weight"].tolist() == [[2.0, 1.0]]
    img = np.asarray(Image.open(img_p).convert("RGB"))
    msk = np.asarray(Image.open(msk_p).convert("L"))
    model = build.narrow_model("cpu")
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    with torch.no_grad():
        cs = []
        for p in (ref_p[0], ref_p[0], ref_p[1]):
            oi, _, om, oref = O.preprocess_triple(img, msk, np.asarray(Image.open(p).convert("RGB").resize((224, 224))))
            cs.append(O.learned_conditioning(sd, oref, cases.CLIP_NARROW, cases.MAPPER_NARROW))
        c = torch.cat(cs, 1)
        z_inp = O.first_stage_encode(sd, oi * om, torch.from_numpy(t["post_eps"]), cases.VAE_NARROW, "first_stage_model.")
        m64 = O.resize_mask(om, z_inp.shape[-2:])
        usd = {k[len("model.diffusion_model."):]: v for k, v in sd.items() if k.startswith("model.diffusion_model.")}
        z0, info = O.plms_sample(lambda x9, tt, ctx: O.unet_forward(usd, x9, tt, ctx, cases.UNET_NARROW), steps, torch.from_numpy(t["x_T"]), c,
                                 sd["learnable_vector"].float().expand(1, 3, -1), 5.0, z_inp, m64, O.schedule_buffers()["alphas_cumprod"])
        image = torch.clamp((O.first_stage_decode(sd, z0, cases.VAE_NARROW, "first_stage_model.") + 1.0) / 2.0, 0.0, 1.0)
    assert info["calls"] == steps + 1
    check("CLI --reference_weight 2 1: conditioning c", torch.from_numpy(t["c"]), c[:, 1:], 4e-3)
    check("CLI --reference_weight 2 1: final latent (2 PLMS steps)", torch.from_numpy(t["latent"]), z0, 8e-3)
    png = np.asarray(Image.open(os.path.join(outdir, "results", f"image_example_1_{seed}.png"))).astype(np.float32)
    exp = (255.0 * image[0].permute(1, 2, 0).numpy()).astype(np.uint8).astype(np.float32)
    mad = float(np.abs(png - exp).mean())
    report("CLI --reference_weight 2 1: result PNG vs oracle, mean |d| in grey levels", mad, 0.55)
    assert png.shape == (512, 512, 3) and mad <= 0.55
    assert torch.equal(out, torch.from_numpy(t["image"]))


def test_inference_cli_reference_weight_zero_is_the_single_reference_run(dev, golden_dir, tmp_path):
    """--reference_weight 1 0 on two references against the run with the first reference alone (another kernel route: within the limits
    of test_inference_cli_two_references, not the same bits)."""
    import yaml
    from PIL import Image
    cli = _cli()
    d = os.path.join(golden_dir, "examples")
    img_p, msk_p = os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png")
    ref_p = [os.path.join(d, "reference_example_1.jpg"), os.path.join(d, "reference_example_2.jpg")]
    cfg, steps, seed = str(tmp_path / "narrow.yaml"), 2, 321
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)

    def run(tag, refs, extra):
        out, dump = str(tmp_path / tag), str(tmp_path / f"{tag}.npz")
        cli.main(["--plms", "--outdir", out, "--config", cfg, "--ddim_steps", str(steps), "--image_path", img_p, "--mask_path", msk_p,
                  "--reference_path", *refs, "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights", "--dump_tensors", dump] + extra)
        return None, np.load(dump), out
    _, t10, out10 = run("w10", ref_p, ["--reference_weight", "1", "0"])
    _, t1, out1 = run("single", ref_p[:1], [])
    assert t1["c"].shape == (1, 1, 768) and t1["reference_weight"].tolist() == [[1.0]]
    check("CLI --reference_weight 1 0 vs the single-reference run: final latent", torch.from_numpy(t10["latent"]), torch.from_numpy(t1["latent"]).float(), 8e-3)
    a = np.asarray(Image.open(os.path.join(out10, "results", f"image_example_1_{seed}.png"))).astype(np.float32)
    b = np.asarray(Image.open(os.path.join(out1, "results", f"image_example_1_{seed}.png"))).astype(np.float32)
    mad = float(np.abs(a - b).mean())
    report("CLI --reference_weight 1 0 vs the single-reference run: PNG mean |d| in grey levels", mad, 0.55)
    assert mad <= 0.55
