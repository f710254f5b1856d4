"""Regional exemplars on the GPU: pbe_ctx_attention_rw_f16 against the fp64 reference of tests/regionref.py (the gate of
tests/ctxref.py, unchanged), its bit identities with the plain and the weighted launch, its padding / bounds contract, and the block,
U-Net, sampler and CLI paths that take region maps against the CPU oracle - per token subset on the unmodified oracle where the regions
are binary, under regionref.regional_oracle where they are soft."""
import os

import numpy as np
import pytest
import torch

import cases
import ctxref
import guard
import modelbuild as build
import regionref as rr
from accgate import rel_l2
from oracle_loader import O
from test_ctx_attention_gpu import _device_operands, _st, check
from test_model_gpu import BLOCK_TOL, FWD_TOL, SAMPLER_OPT_TOL, report

pytestmark = pytest.mark.gpu


def _keys(fn):
    from pbe_amd import ops
    ops._TIMES = {}
    try:
        out = fn()
        return out, list(ops._TIMES)
    finally:
        ops._TIMES = None


def _gate(name, got, o, table):
    want, emu = rr.reference(o, table)[0], rr.emulate(o, table)
    ok, text = ctxref.verdict(got.cpu(), want, emu)
    report(f"ctx_attention rw {name}", rel_l2(got.cpu(), want), ctxref.REL_L2_FACTOR * rel_l2(emu, want))
    print(f"ctx_attention rw {name}: {text}")
    assert ok, f"{name}: {text}"
    import ctxgate                                                           # beside it: every element within its own bound (tests/ctxgate.py)
    from test_accuracy_gpu import report as accuracy_report
    v = ctxgate.verdict(got, o, table.float(), emu=emu)
    accuracy_report(f"{'ctx_attention rw ' + name:64s} err/bound={v.ratio:.3f} at {v.where} rel_l2={v.r_got:.3e} (emulation {v.r_emu:.3e})")
    assert v.ok, f"{name}: {v}"


def _rw(oc, table, dev):
    return oc.with_row_weights(table.float().to(dev).contiguous())


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rr.SHAPES, ids=rr.shape_id)
def test_rw_kernel_against_fp64_reference(dev, shape):
    from pbe_amd import ops
    B, N, C, H, Nk, parts, h, w = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts)
    case = rr.kernel_case(shape)
    x, oc, st = _device_operands(o, dev)
    (y, rs), keys = _keys(lambda: ops.ctx_attention(x, _rw(oc, case["table"], dev), st, ctxref.EPS, tokens=N))
    assert keys == [f"xar:{B * N}:{C}:{H}:{Nk}"], keys
    _gate(rr.shape_id(shape), y, o, case["table"])
    want = torch.stack([y.double().sum(1), (y.double() ** 2).sum(1)], 1).cpu()      # (limits of test_kernel_against_fp64_reference)
    assert rs.parts == 1 and torch.allclose(rs.buf[0].double().cpu(), want, rtol=2e-6, atol=1e-4)
    # the folded operands do not depend on the table: the same operands with another table, no re-folding
    other = rr.kernel_case(shape, seed=1)
    assert not torch.equal(other["table"], case["table"])
    y2, _ = ops.ctx_attention(x, _rw(oc, other["table"], dev), st, ctxref.EPS, tokens=N)
    _gate(rr.shape_id(shape) + " (second table)", y2, o, other["table"])
    y3, rs3 = ops.ctx_attention(x, _rw(oc, case["table"], dev), st, ctxref.EPS, tokens=N)
    assert torch.equal(y, y3) and torch.equal(rs.buf, rs3.buf)                      # run to run


@pytest.mark.parametrize("shape", rr.SHAPES, ids=rr.shape_id)
def test_rw_bit_identities(dev, shape):
    """A zeros table gives the bits of the plain launch, a row-constant table log2 w those of the weighted launch: Y and statistics."""
    from pbe_amd import ops
    import kbiasref as kr
    B, N, C, H, Nk, parts, h, w = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts)
    x, oc, st = _device_operands(o, dev)
    (plain, rs0), k0 = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N))
    (zeros, rs1), k1 = _keys(lambda: ops.ctx_attention(x, _rw(oc, torch.zeros(B, N, Nk), dev), st, ctxref.EPS, tokens=N))
    assert k0 == [f"xa:{B * N}:{C}:{H}:{Nk}"] and k1 == [f"xar:{B * N}:{C}:{H}:{Nk}"]
    assert torch.equal(plain, zeros) and torch.equal(rs0.buf, rs1.buf)
    lw = torch.log2(kr.ctx_weights(B, Nk, 11 + C)).float()
    oc.log2w = lw.to(dev)
    (wy, rs2), k2 = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N))
    (ry, rs3), k3 = _keys(lambda: ops.ctx_attention(x, _rw(oc, lw[:, None, :].expand(B, N, Nk), dev), st, ctxref.EPS, tokens=N))
    assert k2 == [f"xaw:{B * N}:{C}:{H}:{Nk}"] and k3 == [f"xar:{B * N}:{C}:{H}:{Nk}"]
    assert torch.equal(wy, ry) and torch.equal(rs2.buf, rs3.buf) and not torch.equal(wy, plain)


def test_rw_kernel_ignores_padding_and_stays_in_bounds(dev):
    """The table as a [B * N, Nk] view inside a NaN-poisoned arena (column and row padding), Y between sentinels, tokens = 72: fully
    written, nothing outside touched, the gate passes.  Positive control: a NaN at (b = 1, t = 5, j = 0) reaches exactly that row."""
    from pbe_amd import ops
    shape = rr.SHAPES[0]
    B, N, C, H, Nk, parts, h, w = shape
    assert N == 72
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=5)
    case = rr.kernel_case(shape, seed=2)
    x, oc, st = _device_operands(o, dev)
    flat, _ = guard.embed(case["table"].float().reshape(B * N, Nk), col_pad=3, row_pad=2, device=dev)
    table = flat.view(B, N, Nk)
    assert table.stride(1) > Nk and table.stride(2) == 1
    y, arena = guard.sentinel_out((B * N, C), col_pad=40, device=dev)
    ops.ctx_attention(x, oc.with_row_weights(table), st, ctxref.EPS, tokens=N, out=y, row_stats=False)
    torch.cuda.synchronize()
    guard.assert_fully_written(y, "rw ctx_attention Y")
    guard.assert_untouched(arena, y, "rw ctx_attention Y")
    _gate("poisoned padding", y.contiguous(), o, case["table"])
    # a launch over the first sample alone reads nothing of the second sample's table: poison it
    t1 = case["table"].float().clone()
    t1[1] = float("nan")
    y1, _ = ops.ctx_attention(x[:N], oc.rows(0, 1).with_row_weights(t1.to(dev)[:1]), st, ctxref.EPS, tokens=N, row_stats=False)
    assert torch.equal(y1, y[:N])
    bad = case["table"].float().clone()
    bad[1, 5, 0] = float("nan")
    yb, _ = ops.ctx_attention(x, _rw(oc, bad, dev), st, ctxref.EPS, tokens=N, row_stats=False)
    finite = torch.isfinite(yb.float()).all(1).cpu()
    want = torch.ones(B * N, dtype=torch.bool)
    want[N + 5] = False
    assert torch.equal(finite, want), torch.nonzero(~finite).flatten().tolist()
    assert not torch.isfinite(yb[N + 5].float()).any()


def test_rw_launch_refusals(dev):
    from ldm.modules.attention import prepare_context_regions
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    shape = rr.SHAPES[0]
    B, N, C, H, Nk, parts, h, w = shape
    x, oc, st = _device_operands(ctxref.random_operands(B, N, C, H, Nk, parts), dev)
    z = torch.zeros(B, N, Nk, device=dev)
    bads = [torch.zeros(B, N, Nk + 1, device=dev), torch.zeros(B, N + 1, Nk, device=dev), torch.zeros(B + 1, N, Nk, device=dev),
            torch.zeros(B * N, Nk, device=dev), z.half(), z.cpu(), torch.zeros(B, N, 2 * Nk, device=dev)[:, :, ::2],
            torch.zeros(B, Nk, N, device=dev).transpose(1, 2)]
    for bad in bads:
        with pytest.raises(PbeError):
            ops.ctx_attention(x, oc.with_row_weights(bad), st, ctxref.EPS, tokens=N)
    both = oc.with_row_weights(z)
    both.log2w = torch.zeros(B, Nk, device=dev)
    with pytest.raises(PbeError, match="log2rw replaces log2w"):
        ops.ctx_attention(x, both, st, ctxref.EPS, tokens=N)
    ops.ctx_attention(x, oc.with_row_weights(z), st, ctxref.EPS, tokens=N)
    # 20 tokens are beyond the fused kernel, the only per-row form
    sp, _ = _st(320, 8, dev, "st.")
    ctx = torch.randn(2, 20, 768).to(dev)
    with pytest.raises(PbeError, match="16"):
        sp(torch.randn(2, 320, 8, 12).to(dev), ctx, context_regions=torch.ones(2, 20, 8, 12))
    with pytest.raises(PbeError, match="8 x 12"):
        sp(torch.randn(2, 320, 8, 12).to(dev), ctx[:, :3].contiguous(), context_regions=torch.ones(2, 3, 12, 12))
    assert prepare_context_regions(ctx, None) is None


# ---- blocks against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 320, 1280])
def test_spatial_transformer_regions_against_oracle(dev, C):
    """Binary regions (left half / right half / rows 2-4, one uncovered cell) against the unmodified oracle run per token subset, and
    soft regions with weights (2, 1, 0.5) against the oracle with ln e added to its scores.  Every width takes the fused kernel."""
    H, h, w = 8, 8, 12
    st, sd = _st(C, H, dev, "st.")
    g = torch.Generator().manual_seed(C)
    x, ctx = torch.randn(2, C, h, w, generator=g), torch.randn(2, 3, 768, generator=g)
    r = rr.binary_regions(2, h, w)
    with torch.no_grad():
        want = rr.subset_composition(lambda b, c: O.spatial_transformer(sd, "st.", x[b:b + 1], c, H), ctx, rr.level_weights(r, None, h, w))
        plain = O.spatial_transformer(sd, "st.", x, ctx, H)
        got, keys = _keys(lambda: st(x.to(dev), ctx.to(dev), context_regions=r))
        got2 = st(x.to(dev), ctx.to(dev), context_regions=rr.binary_regions(2, h, w, up=2).float())
    check(f"SpatialTransformer C={C}, binary regions vs the per-subset oracle", got, want, BLOCK_TOL)
    report(f"SpatialTransformer C={C}: regional vs regionless oracle (must be far)", rel_l2(want, plain.double()), 1.0)
    assert rel_l2(want, plain.double()) > 10 * BLOCK_TOL
    assert torch.equal(got, got2)                                            # the same maps at twice the resolution: the same table
    assert any(k.startswith("xar:") for k in keys), keys
    assert not any(k.startswith(("xa:", "xaw:", "ab:", "a:2:8:96:3:")) for k in keys), keys
    rs, wt = rr.soft_regions(2, 3, h, w, seed=C, up=2), [[2.0, 1.0, 0.5]] * 2
    with torch.no_grad():
        with rr.regional_oracle(O, [rr.level_table(rs, wt, h, w)]):
            want = O.spatial_transformer(sd, "st.", x, ctx, H)
        got, keys = _keys(lambda: st(x.to(dev), ctx.to(dev), context_weights=torch.tensor(wt), context_regions=rs))
    check(f"SpatialTransformer C={C}, soft regions x weights vs the regional oracle", got, want, BLOCK_TOL)
    assert any(k.startswith("xar:") for k in keys) and not any(k.startswith(("xa:", "xaw:", "ab:", "a:2:8:96:3:")) for k in keys), keys


def test_block_takes_levelled_row_weights(dev):
    """BasicTransformerBlock.forward(context_row_weights=e [B, N, K]) is the SpatialTransformer's route without the level step."""
    from pbe_amd.lib import PbeError
    C, H, h, w = 64, 8, 8, 12
    st, _ = _st(C, H, dev, "st.")
    blk = st.transformer_blocks[0]
    g = torch.Generator().manual_seed(3)
    x, ctx = torch.randn(2, h * w, C, generator=g).to(dev), torch.randn(2, 3, 768, generator=g).to(dev)
    rs, wt = rr.soft_regions(2, 3, h, w, seed=4), torch.tensor([[2.0, 1.0, 0.5]] * 2)
    e = rr.level_weights(rs, wt, h, w)
    with torch.no_grad():
        a, keys = _keys(lambda: blk(x, ctx, context_row_weights=e))
        ones = blk(x, ctx, context_row_weights=torch.ones(2, h * w, 3))
        plain = blk(x, ctx)
        one_tok = blk(x, ctx[:, :1].contiguous(), context_row_weights=torch.ones(2, h * w, 1))
        one_plain = blk(x, ctx[:, :1].contiguous())
    assert any(k.startswith("xar:") for k in keys)
    assert torch.equal(ones, plain) and not torch.equal(a, plain) and torch.equal(one_tok, one_plain)
    for bad in (torch.ones(2, h * w, 2), torch.zeros(2, h * w, 3), -torch.ones(2, h * w, 3)):
        with pytest.raises(PbeError):
            blk(x, ctx, context_row_weights=bad)
    with pytest.raises(PbeError):
        blk(x, ctx, context_weights=wt, context_row_weights=e)


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


def _tables(r, wt):
    return [rr.level_table(r, wt, s, s) for s in (16, 8, 4, 2)]               # the narrow model's attention grids (2 x 2: the middle block)


@pytest.mark.parametrize("up", [1, 2], ids=["16x16", "32x32"])
def test_narrow_unet_forward_regions(dev, narrow, narrow_sd, up):
    """4 samples, 3 tokens, soft regions at the latent grid or twice it, sample 2 with all-ones regions; grids 16 / 8 / 4 / 2."""
    inp = cases.narrow_inputs()
    g = torch.Generator().manual_seed(404)
    ctx = torch.randn(4, 3, 768, generator=g)
    r = rr.soft_regions(4, 3, 16, 16, seed=40 + up, up=up)
    r[2] = 1.0
    sd = _unet_sd(narrow_sd)
    x, t = inp["unet_x"], inp["unet_t"]
    with torch.no_grad():
        with rr.regional_oracle(O, _tables(r, None)):
            want = O.unet_forward(sd, x, t, ctx, cases.UNET_NARROW)
        plain_want = O.unet_forward(sd, x, t, ctx, cases.UNET_NARROW)
        (got, keys) = _keys(lambda: narrow.apply_model(x.to(dev), t.to(dev), ctx.to(dev), context_regions=r))
        plain = narrow.apply_model(x.to(dev), t.to(dev), ctx.to(dev))
        ones = narrow.apply_model(x.to(dev), t.to(dev), ctx.to(dev), context_regions=torch.ones(4, 3, 16 * up, 16 * up))
    check(f"narrow UNetModel forward, regions at {16 * up}x{16 * up}", got, want, FWD_TOL)
    report("narrow UNetModel: regional vs regionless oracle (must be far)", rel_l2(want, plain_want.double()), 1.0)
    assert rel_l2(want, plain_want.double()) > 10 * FWD_TOL
    assert any(k.startswith("xar:") for k in keys) and not any(k.startswith(("xa:", "xaw:")) for k in keys), keys
    assert torch.equal(got[2], plain[2]) and not torch.equal(got[1], plain[1])      # the all-ones sample: the regionless run's bits
    assert torch.equal(ones, plain)


def test_context_cache_key_includes_the_regions(dev, narrow):
    inp = cases.narrow_inputs()
    g = torch.Generator().manual_seed(406)
    ctx = torch.randn(4, 3, 768, generator=g).to(dev)
    x, t = inp["unet_x"].to(dev), inp["unet_t"].to(dev)
    wt = torch.tensor([[1.0, 2.0, 0.5]] * 4)
    ra, rb = rr.soft_regions(4, 3, 16, 16, seed=1), rr.soft_regions(4, 3, 16, 16, seed=2)
    with torch.no_grad():
        a = narrow.apply_model(x, t, ctx, context_weights=wt, context_regions=ra)
        b = narrow.apply_model(x, t, ctx, context_weights=wt, context_regions=rb)
        a2 = narrow.apply_model(x, t, ctx, context_weights=wt, context_regions=ra)
        w_only = narrow.apply_model(x, t, ctx, context_weights=wt)
        keep = ra.clone()
        ra.copy_(rb)                                         # in place: another version of the same tensor
        a3 = narrow.apply_model(x, t, ctx, context_weights=wt, context_regions=ra)
        ra.copy_(keep)
        fa = build.narrow_model(dev).apply_model(x, t, ctx, context_weights=wt, context_regions=ra)
        fb = build.narrow_model(dev).apply_model(x, t, ctx, context_weights=wt, context_regions=rb)
    assert not torch.equal(a, b) and not torch.equal(a, w_only)
    assert torch.equal(a, fa) and torch.equal(b, fb) and torch.equal(a, a2) and torch.equal(a3, b)


def test_narrow_paired_prefix_is_bit_identical_with_regions(dev, narrow):
    from pbe_amd import ops
    g = torch.Generator().manual_seed(7)
    unet = narrow.model.diffusion_model
    B, K = 2, 3
    x = torch.randn(B, 4, 16, 16, generator=g).to(dev)
    z = torch.randn(B, 4, 16, 16, generator=g).to(dev)
    m = (torch.rand(B, 1, 16, 16, generator=g) > 0.3).float().to(dev)
    ctx = torch.randn(2 * B, K, 768, generator=g).to(dev)
    wt = torch.exp2(torch.randn(2 * B, K, generator=g, dtype=torch.float64))
    r = rr.soft_regions(2 * B, K, 16, 16, seed=9)
    t = torch.full((2 * B,), 621, dtype=torch.int64, device=dev)
    with torch.no_grad():
        a = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 2), t, ctx, context_weights=wt, context_regions=r)
        b = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 1), t, ctx, paired=True, context_weights=wt, context_regions=r)
        plain = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 2), t, ctx, context_weights=wt)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"
    assert not torch.equal(a, plain)


def _conditioning(narrow, dev):
    g = torch.Generator().manual_seed(8)
    refs = torch.randn(2, 3, 3, 224, 224, generator=g)
    return narrow.proj_out(narrow.get_learned_conditioning(refs.to(dev))), torch.tensor([[2.0, 1.0, 0.5], [1.0, 0.0, 3.0]]), \
        rr.soft_regions(2, 3, 16, 16, seed=12)


@pytest.mark.parametrize("which", ["plms", "ddim"])
def test_narrow_samplers_regions_against_oracle(dev, narrow, narrow_sd, golden_dir, which):
    """4 steps at scale 5 with regions and weights against the oracle sampler whose cross-attention adds ln e (the unconditional half of
    its 2B batch gets none); the graphed run gives the eager run's bits."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    z_inp, m = torch.from_numpy(gold["z_inpaint"]), torch.from_numpy(gold["mask_lat"])
    sd = _unet_sd(narrow_sd)
    ac = O.schedule_buffers()["alphas_cumprod"]
    model = lambda x9, t, ctx: O.unet_forward(sd, x9, t, ctx, cases.UNET_NARROW)      # noqa: E731
    cls = PLMSSampler if which == "plms" else DDIMSampler
    with torch.no_grad():
        c, wt, r = _conditioning(narrow, dev)
        kw = dict(S=4, batch_size=2, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                  unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
                  test_model_kwargs={"inpaint_image": z_inp.to(dev), "inpaint_mask": m.to(dev)}, conditioning_weights=wt)
        eager = cls(narrow)
        eager.use_graph = False
        z0, _ = eager.sample(conditioning_regions=r, **kw)
        zw, _ = eager.sample(**kw)
        graphed = cls(narrow)
        graphed.use_graph = True
        zg, _ = graphed.sample(conditioning_regions=r, **kw)
        osample = O.plms_sample if which == "plms" else O.ddim_sample
        with rr.regional_oracle(O, _tables(r, wt)):
            want = osample(model, 4, inp["x_T"], c.float().cpu(), narrow_sd["learnable_vector"].expand(2, 3, -1), 5.0, z_inp, m, ac)[0]
    check(f"narrow {which.upper()} 4 steps, regions x weights", z0, want, SAMPLER_OPT_TOL)
    assert not torch.equal(z0, zw)
    assert torch.equal(z0, zg)


def test_sampler_refuses_bad_regions(dev, narrow, golden_dir):
    from ldm.models.diffusion.plms import PLMSSampler
    from pbe_amd.lib import PbeError
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    kw = dict(S=2, batch_size=2, shape=[4, 16, 16], conditioning=torch.randn(2, 3, 768).to(dev), verbose=False, unconditional_guidance_scale=5.0,
              unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
              test_model_kwargs={"inpaint_image": torch.from_numpy(gold["z_inpaint"]).to(dev), "inpaint_mask": torch.from_numpy(gold["mask_lat"]).to(dev)})
    neg = torch.ones(2, 3, 16, 16)
    neg[1, 1, 2, 3] = -0.5
    for bad in (torch.ones(2, 3, 16), torch.ones(2, 2, 16, 16), neg, torch.ones(2, 3, 12, 16), torch.full((2, 3, 16, 16), float("nan"))):
        with pytest.raises(PbeError):
            PLMSSampler(narrow).sample(conditioning_regions=bad, **kw)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_inference_cli_reference_region(dev, golden_dir, tmp_path):
    """Two references, left-half / right-half region images: the CLI's result is the direct pipeline.inpaint(ref_regions=) run on the
    same tensors and differs from the run without --reference_region; a count mismatch is a parser error."""
    import importlib.util
    import yaml
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_r", os.path.join(root, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    d = os.path.join(golden_dir, "examples")
    img_p, msk_p = os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png")
    ref_p = [os.path.join(d, "reference_example_1.jpg"), os.path.join(d, "reference_example_2.jpg")]
    cfg, steps, seed = str(tmp_path / "narrow.yaml"), 2, 321
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)
    left = np.zeros((512, 512), dtype=np.uint8)
    left[:, :256] = 255
    reg_p = [str(tmp_path / "left.png"), str(tmp_path / "right.png")]
    Image.fromarray(left).save(reg_p[0])
    Image.fromarray(255 - left).save(reg_p[1])

    def run(tag, extra):
        out, dump = str(tmp_path / tag), str(tmp_path / f"{tag}.npz")
        x = cli.main(["--plms", "--outdir", out, "--config", cfg, "--ddim_steps", str(steps), "--image_path", img_p, "--mask_path", msk_p,
                      "--reference_path", *ref_p, "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights", "--skip_save",
                      "--dump_tensors", dump] + extra)
        return x, np.load(dump)
    out, t = run("regions", ["--reference_region", *reg_p, "--reference_weight", "2", "1"])
    _, t0 = run("plain", ["--reference_weight", "2", "1"])
    reg = torch.from_numpy(t["reference_region"])
    assert tuple(reg.shape) == (1, 2, 64, 64) and "reference_region" not in t0.files
    assert float(reg.min()) >= 0.0 and float(reg.max()) <= 1.0
    assert bool((reg[0, 0, :, :31] > 1 - 1e-6).all()) and bool((reg[0, 0, :, 33:] < 1e-6).all()) and torch.allclose(reg[0, 0] + reg[0, 1], torch.ones(64, 64, dtype=reg.dtype))
    trip = preprocess.load_triple_device(img_p, msk_p, ref_p[0], dev)
    ref = torch.stack([trip["ref"], preprocess.load_triple_device(img_p, msk_p, ref_p[1], dev)["ref"]], 1)
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint(model, trip["image"], trip["mask"], ref, steps=steps, scale=5.0, x_T=torch.from_numpy(t["x_T"]).to(dev),
                                  post_eps=torch.from_numpy(t["post_eps"]).to(dev), sampler="plms", ref_weights=torch.from_numpy(t["reference_weight"]),
                                  ref_regions=reg)
    assert torch.equal(direct["c"].float().cpu(), torch.from_numpy(t["c"]))
    assert torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
    assert torch.equal(direct["image"].float().cpu(), out)
    away = rel_l2(torch.from_numpy(t["latent"]), torch.from_numpy(t0["latent"]).double())
    report("CLI --reference_region vs the run without it: final latent rel-L2 (must be far)", away, 1.0)
    assert away > 10 * 8e-3                                                # 8e-3: the CLI tests' latent limit
    with pytest.raises(SystemExit):
        cli.parse(["--reference_path", *ref_p, "--reference_region", reg_p[0]])
