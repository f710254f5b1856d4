"""Exemplar attribution maps on the GPU: the map-emitting form of the fused cross-attention kernel (pbe_ctx_attention_map_f16) against
the fp64 reference and the verdict of tests/mapref.py, its bit identity with the launches without the map, its bounds and its
accumulate mode; the gather kernel (pbe_ctx_map_gather_f32) against numpy; and the collector (ldm.modules.attention.ContextMaps)
through the SpatialTransformer, the narrow U-Net, both samplers, the pipeline and the CLI - against the oracle's own softmax where a
reference exists, bit for bit between the paired / unpaired / graphed / eager routes."""
import io
import os

import numpy as np
import pytest
import torch

import cases
import ctxref
import guard
import kbiasref as kr
import mapref as mr
import modelbuild as build
import regionref as rr
from accgate import rel_l2
from oracle_loader import O
from test_ctx_attention_gpu import _device_operands, _st
from test_model_gpu import SAMPLER_OPT_TOL, report

pytestmark = pytest.mark.gpu

# rel-L2 of a SpatialTransformer's maps against the oracle's softmax (fp32, CPU).  Not derivable - it includes the block's fp16 drift
# ahead of the scores (GroupNorm, proj_in, attn1) - so, by the project's convention (a regression that triples an
# error fails), 3 x the largest value measured on an MI355X over the six cases of test_spatial_transformer_maps_against_oracle
# (profiles/ctx_maps_report.txt).
MAP_ORACLE_MEASURED = 1.937e-4      # C = 1280, no regions; the six cases measured 1.47e-4 .. 1.94e-4
MAP_ORACLE_TOL = 3 * MAP_ORACLE_MEASURED


def _keys(fn):
    from pbe_amd import ops
    ops._TIMES = {}
    try:
        out = fn()
        return out, list(ops._TIMES)
    finally:
        ops._TIMES = None


def _form(o, shape, form, dev, oc):
    """(operands for the launch, fp64 table [B, N, Nk] the verdict takes) of the plain / weighted / row-weight form."""
    B, N, C, H, Nk, parts = shape
    if form == "plain":
        return oc, mr.zeros_table(o)
    if form == "weights":
        w = kr.ctx_weights(B, Nk, 11 + C)
        oc.log2w = torch.log2(w).float().to(dev)
        return oc, mr.weights_table(o, w)
    case = mr.region_case(shape)
    return oc.with_row_weights(case["table"].float().to(dev).contiguous()), case["table"]


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "weights", "regions"])
@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_map_kernel_against_fp64_reference(dev, shape, form):
    """The map passes the verdict; Y and the row statistics are those of the entry point without the map, bit for bit."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts)
    x, oc, st = _device_operands(o, dev)
    oc, table = _form(o, shape, form, dev, oc)
    (y0, rs0), k0 = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N))
    amap = torch.full((B, N, Nk), float("nan"), device=dev)
    (y1, rs1), k1 = _keys(lambda: ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(amap, False)))
    tag = {"plain": "xa", "weights": "xaw", "regions": "xar"}[form]
    assert k0 == [f"{tag}:{B * N}:{C}:{H}:{Nk}"] and k1 == [f"{tag}m:{B * N}:{C}:{H}:{Nk}"], (k0, k1)
    assert torch.equal(y0, y1) and torch.equal(rs0.buf, rs1.buf)
    want, emu = mr.reference(o, table), mr.emulate(o, table)
    ok, text = mr.verdict(amap, want, emu, table)
    report(f"ctx_attention map {form} {mr.shape_id(shape)}: max|d| (bound 2^-11)", float((amap.double().cpu() - want).abs().max()), mr.ABS_BOUND)
    print(f"ctx_attention map {form} {mr.shape_id(shape)}: {text}")
    assert ok, text
    import ctxgate                                                           # beside it: Y and the map per element (tests/ctxgate.py)
    from test_accuracy_gpu import report as accuracy_report
    ref = ctxgate.reference(o, None if form == "plain" else table.float())
    v = ctxgate.verdict(y1, o, None if form == "plain" else table.float(), ref=ref)
    accuracy_report(f"{'ctx_attention ' + form + ' ' + mr.shape_id(shape):64s} err/bound={v.ratio:.3f} at {v.where} rel_l2={v.r_got:.3e} (emulation {v.r_emu:.3e})")
    assert v.ok, str(v)
    ok2, ratio, where, text2 = ctxgate.map_verdict(amap, o, None if form == "plain" else table.float(), ref=ref)
    accuracy_report(f"{'ctx_attention map ' + form + ' ' + mr.shape_id(shape):64s} err/bound={ratio:.3f} at {where}")
    assert ok2, text2
    # the operands may carry the target themselves (what the transformer blocks use); run to run: the same bits
    again = torch.zeros_like(amap)
    y2, _ = ops.ctx_attention(x, oc.with_map(again, False), st, ctxref.EPS, tokens=N)
    assert torch.equal(again, amap) and torch.equal(y2, y0)


@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_map_store_stays_in_bounds(dev, shape):
    """Store mode into a sentinel-filled buffer with am_rs = Nk + 3 and one guard row per sample: every (t < tokens, j < Nk) element is
    written, every guard element keeps the sentinel."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=3)
    x, oc, st = _device_operands(o, dev)
    bits = guard.SENTINEL_BITS[torch.float32]
    arena = torch.full((B + 1, N + 1, Nk + 3), bits, dtype=torch.int32, device=dev).view(torch.float32)      # (+ a whole guard sample behind)
    amap = arena[:B, :N, :Nk]
    assert amap.stride() == ((N + 1) * (Nk + 3), Nk + 3, 1)
    ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(amap, False), row_stats=False)
    torch.cuda.synchronize()
    ib = arena.view(torch.int32).cpu()
    inside = torch.zeros_like(ib, dtype=torch.bool)
    inside[:B, :N, :Nk] = True
    assert bool((ib[inside] != bits).all()), f"{int((ib[inside] == bits).sum())} map elements were not written"
    assert bool((ib[~inside] == bits).all()), f"{int((ib[~inside] != bits).sum())} guard elements were written"
    dense = torch.empty(B, N, Nk, device=dev)
    ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(dense, False), row_stats=False)
    assert torch.equal(amap, dense)                                            # the padded layout changes nothing


@pytest.mark.parametrize("shape", [mr.SHAPES[1], mr.SHAPES[2], mr.SHAPES[5]], ids=mr.shape_id)
def test_map_accumulate(dev, shape):
    """Two launches into zeros give exactly 2 x the stored map; one launch onto a random base gives base + stored bit for bit (one fp32
    add by the thread that owns the element)."""
    from pbe_amd import ops
    B, N, C, H, Nk, parts = shape
    o = ctxref.random_operands(B, N, C, H, Nk, parts, seed=2)
    x, oc, st = _device_operands(o, dev)
    oc = oc.with_row_weights(mr.region_case(shape)["table"].float().to(dev).contiguous())
    stored = torch.empty(B, N, Nk, device=dev)
    y0, _ = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(stored, False))
    twice = torch.zeros(B, N, Nk, device=dev)
    for _ in range(2):
        y1, _ = ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(twice, True))
    assert torch.equal(twice, 2 * stored) and torch.equal(y0, y1)
    base = torch.randn(B, N, Nk, generator=torch.Generator().manual_seed(9)).to(dev)
    acc = base.clone()
    ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(acc, True))
    assert torch.equal(acc, base + stored)


def test_map_launch_refusals(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    shape = mr.SHAPES[0]
    B, N, C, H, Nk, parts = shape
    x, oc, st = _device_operands(ctxref.random_operands(B, N, C, H, Nk, parts), dev)
    z = torch.zeros(B, N, Nk, device=dev)
    for bad in (torch.zeros(B, N, Nk + 1, device=dev), torch.zeros(B + 1, N, Nk, device=dev), z.half(), z.cpu(), torch.zeros(B, N, 2 * Nk, device=dev)[:, :, ::2]):
        with pytest.raises(PbeError, match="attn_map"):
            ops.ctx_attention(x, oc, st, ctxref.EPS, tokens=N, attn_map=(bad, True))
    with pytest.raises(PbeError, match="launch per range"):
        ops.ctx_attention(x, oc.with_map(z[:1], True, 1), st, ctxref.EPS, tokens=N)


def test_map_gather_against_numpy(dev):
    """A non-square level, 8 x 12 -> 16 x 24, store and accumulate: a multiply by a power of two and copies, so exact."""
    from pbe_amd import ops
    B, K, h, w = 2, 3, 8, 12
    g = torch.Generator().manual_seed(21)
    acc = torch.rand(B, h * w, K, generator=g)
    want = mr.gather_numpy(acc.numpy(), (h, w), (16, 24), 0.25)
    out = torch.full((B, K, 16, 24), float("nan"), device=dev)
    got = ops.ctx_map_gather(acc.to(dev), (h, w), 0.25, out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    base = torch.randn(B, K, 16, 24, generator=g)
    got = ops.ctx_map_gather(acc.to(dev), (h, w), 0.25, out=base.to(dev), accumulate=True)
    assert np.array_equal(got.cpu().numpy(), base.numpy() + want)
    own = ops.ctx_map_gather(acc.to(dev), (h, w))
    assert np.array_equal(own.cpu().numpy(), acc.numpy().reshape(B, h, w, K).transpose(0, 3, 1, 2))
    third = ops.ctx_map_gather((3 * torch.ones(B, h * w, K)).to(dev), (h, w), div=3.0)
    assert bool((third == 1.0).all())                                          # n launches of exactly 1, divided by n: exactly 1


# ---- blocks against the oracle's softmax -----------------------------------------------------------------------------------------------
def _level_map(cm, h, w):
    """[B, h*w, K] of the collector's h x w level."""
    m = cm.per_level()[(h, w)]
    return m.permute(0, 2, 3, 1).reshape(m.shape[0], h * w, m.shape[1]).cpu()


@pytest.mark.parametrize("C", [64, 320, 1280])
def test_spatial_transformer_maps_against_oracle(dev, C):
    """A depth-1 SpatialTransformer on an 8 x 12 grid, 3 tokens: soft regions x weights (2, 1, 0.5), and no regions, against the softmax
    the oracle itself forms (mapref.oracle_maps).  A path that ignored the regions could not pass: the two oracle maps lie far apart.
    With regions the output carries the bits of the run without a collector; without regions those of a block whose
    ctx_fused_max_width is 1280 (at C = 1280 the default route is the q / attention / to_out composition)."""
    from ldm.modules.attention import ContextMaps
    H, h, w = 8, 8, 12
    st, sd = _st(C, H, dev, "st.")
    g = torch.Generator().manual_seed(C)
    x, ctx = torch.randn(2, C, h, w, generator=g), torch.randn(2, 3, 768, generator=g)
    rs, wt = rr.soft_regions(2, 3, h, w, seed=C, up=2), torch.tensor([[2.0, 1.0, 0.5]] * 2)
    xd, cd = x.to(dev), ctx.to(dev)
    with torch.no_grad():
        with mr.oracle_maps(O, [rr.level_table(rs, wt, h, w)]) as rec_r:
            O.spatial_transformer(sd, "st.", x, ctx, H)
        with mr.oracle_maps(O) as rec_p:
            O.spatial_transformer(sd, "st.", x, ctx, H)
        cm_r, cm_p = ContextMaps(), ContextMaps()
        y_r, keys_r = _keys(lambda: st(xd, cd, context_weights=wt, context_regions=rs, context_maps=cm_r))
        y_r0 = st(xd, cd, context_weights=wt, context_regions=rs)
        y_p, keys_p = _keys(lambda: st(xd, cd, context_maps=cm_p))
        st.transformer_blocks[0].ctx_fused_max_width = 1280
        y_p0 = st(xd, cd)
    (n_r, want_r), (n_p, want_p) = rec_r[0], rec_p[0]
    assert len(rec_r) == len(rec_p) == 1 and n_r == n_p == h * w
    assert cm_r.counts() == {(h, w): 1} and cm_p.counts() == {(h, w): 1}
    got_r, got_p = _level_map(cm_r, h, w), _level_map(cm_p, h, w)
    for name, got, want in (("soft regions x weights", got_r, want_r), ("no regions", got_p, want_p)):
        v = rel_l2(got, want)
        report(f"SpatialTransformer C={C}, attribution map vs the oracle's softmax, {name}", v, MAP_ORACLE_TOL)
        assert bool(torch.isfinite(got).all()) and v <= MAP_ORACLE_TOL, f"{name}: rel-L2 {v:.3e} > {MAP_ORACLE_TOL:.1e}"
        assert float((got.double().sum(-1) - 1).abs().max()) <= mr.ROW_BOUND
    away = rel_l2(want_r, want_p)
    report(f"SpatialTransformer C={C}: regional vs regionless oracle map (must be far)", away, 1.0)
    assert away > 10 * MAP_ORACLE_TOL and rel_l2(got_r, want_p) > 10 * MAP_ORACLE_TOL
    assert torch.equal(y_r, y_r0) and torch.equal(y_p, y_p0)
    assert any(k.startswith("xarm:") for k in keys_r) and any(k.startswith("xam:") for k in keys_p)
    assert not any(k.startswith(("xa:", "xaw:", "xar:", "a:2:8:96:3:")) for k in keys_r + keys_p), (keys_r, keys_p)


def test_context_beyond_the_fused_kernel_is_refused_with_a_collector(dev):
    from ldm.modules.attention import ContextMaps
    from pbe_amd.lib import PbeError
    st, _ = _st(320, 8, dev, "st.")
    x = torch.randn(2, 320, 8, 12).to(dev)
    with pytest.raises(PbeError, match=r"attribution maps take at most 16 context tokens, got 20"):
        st(x, torch.randn(2, 20, 768).to(dev), context_maps=ContextMaps())
    st(x, torch.randn(2, 20, 768).to(dev))                                    # (without a collector: the composition, as before)
    wide, _ = _st(320, 16, dev, "st.")                                        # 16 heads x 9 tokens = 144 > 128
    with pytest.raises(PbeError, match="heads \\* tokens <= 128"):
        wide(x, torch.randn(2, 9, 768).to(dev), context_maps=ContextMaps())


# ---- the narrow model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


def test_binary_regions_give_exact_maps(dev, narrow):
    """Binary regions through a narrow U-Net forward: at every position of every level that exactly one token covers, that token's map
    is exactly 1.0 and the others' exactly 0.0 - a lone live key gives exp2(0) / 1 in every head and block, the counts and the division
    are exact.  The eps is that of the forward without a collector, bit for bit."""
    from ldm.modules.attention import ContextMaps
    inp = cases.narrow_inputs()
    g = torch.Generator().manual_seed(404)
    ctx = torch.randn(4, 3, 768, generator=g).to(dev)
    r = rr.binary_regions(4, 16, 16)
    x, t = inp["unet_x"].to(dev), inp["unet_t"].to(dev)
    cm = ContextMaps()
    with torch.no_grad():
        got = narrow.apply_model(x, t, ctx, context_regions=r, context_maps=cm)
        plain = narrow.apply_model(x, t, ctx, context_regions=r)
    assert torch.equal(got, plain)
    per = cm.per_level()
    assert sorted(per) == [(2, 2), (4, 4), (8, 8), (16, 16)] and all(n > 0 for n in cm.counts().values()), cm.counts()
    lone_rows = 0
    for (h, w), m in per.items():
        e = rr.level_weights(r, None, h, w)                                    # [B, h*w, K] fp64
        lone = (e > 0).sum(-1) == 1
        mm = m.permute(0, 2, 3, 1).reshape(4, h * w, 3).cpu()
        assert torch.equal(mm[lone], (e[lone] > 0).float()), f"level {h} x {w}"
        lone_rows += int(lone.sum())
        assert float((mm.double().sum(-1) - 1).abs().max()) <= mr.ROW_BOUND
    assert lone_rows > 4 * 100
    res = cm.result((16, 16))
    assert tuple(res.shape) == (4, 3, 16, 16) and float((res.double().sum(1) - 1).abs().max()) <= mr.ROW_BOUND


def _conditioning(narrow, dev):
    g = torch.Generator().manual_seed(8)
    refs = torch.randn(2, 3, 3, 224, 224, generator=g)
    return narrow.proj_out(narrow.get_learned_conditioning(refs.to(dev))), torch.tensor([[2.0, 1.0, 0.5], [1.0, 0.0, 3.0]]), \
        rr.soft_regions(2, 3, 16, 16, seed=12)


def _sampler_kw(narrow, dev, golden_dir, c):
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    return dict(S=4, batch_size=2, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
                test_model_kwargs={"inpaint_image": torch.from_numpy(gold["z_inpaint"]).to(dev), "inpaint_mask": torch.from_numpy(gold["mask_lat"]).to(dev)})


def _sampler(narrow, which, graph=False, paired=True):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    s = (PLMSSampler if which == "plms" else DDIMSampler)(narrow)
    s.use_graph, s.share_guidance_prefix = graph, paired
    return s


def _same_maps(a, b):
    pa, pb = a.per_level(), b.per_level()
    return a.counts() == b.counts() and sorted(pa) == sorted(pb) and all(torch.equal(pa[k], pb[k]) for k in pa) and \
        torch.equal(a.result((16, 16)), b.result((16, 16)))


@pytest.mark.parametrize("which", ["plms", "ddim"])
def test_narrow_samplers_collect_maps(dev, narrow, golden_dir, which):
    """4 steps at scale 5, regions x weights: the maps of the paired, the unpaired (one 2B batch, the conditional rows) and the graphed
    run are the same bits, from every U-Net call of the run (PLMS: the probe call too); the latent is that of the run without a
    collector.  Sample 1 has weight 0 on token 1: its map is exactly 0."""
    from ldm.modules.attention import ContextMaps
    with torch.no_grad():
        c, wt, r = _conditioning(narrow, dev)
        kw = dict(_sampler_kw(narrow, dev, golden_dir, c), conditioning_weights=wt, conditioning_regions=r)
        cms = [ContextMaps() for _ in range(3)]
        z_p, _ = _sampler(narrow, which).sample(conditioning_maps=cms[0], **kw)
        z_u, _ = _sampler(narrow, which, paired=False).sample(conditioning_maps=cms[1], **kw)
        z_g, _ = _sampler(narrow, which, graph=True).sample(conditioning_maps=cms[2], **kw)
        z_0, _ = _sampler(narrow, which).sample(**kw)
    calls = 5 if which == "plms" else 4
    counts = cms[0].counts()
    assert sorted(counts) == [(2, 2), (4, 4), (8, 8), (16, 16)] and all(n > 0 and n % calls == 0 for n in counts.values()), counts
    assert _same_maps(cms[0], cms[1]), "paired vs unpaired guidance"
    assert _same_maps(cms[0], cms[2]), "graphed vs eager"
    assert torch.equal(z_p, z_0) and torch.equal(z_u, z_0) and torch.equal(z_g, z_0)
    res = cms[0].result((16, 16))
    assert tuple(res.shape) == (2, 3, 16, 16) and bool(torch.isfinite(res).all())
    assert float((res.double().sum(1) - 1).abs().max()) <= mr.ROW_BOUND and bool((res[1, 1] == 0).all()) and float(res[0, 1].max()) > 0


@pytest.mark.parametrize("which", ["plms", "ddim"])
def test_narrow_samplers_maps_without_regions(dev, narrow, golden_dir, which):
    """No regions: with a collector every level takes the fused kernel, so the latent is that of a collector-less run whose blocks
    have ctx_fused_max_width = 1280, bit for bit, and within SAMPLER_OPT_TOL of the default collector-less run."""
    from ldm.modules.attention import BasicTransformerBlock, ContextMaps
    with torch.no_grad():
        c, wt, _ = _conditioning(narrow, dev)
        kw = dict(_sampler_kw(narrow, dev, golden_dir, c), conditioning_weights=wt)
        cm = ContextMaps()
        z_m, _ = _sampler(narrow, which).sample(conditioning_maps=cm, **kw)
        z_0, _ = _sampler(narrow, which).sample(**kw)
        wide = build.narrow_model(dev)
        for m in wide.modules():
            if isinstance(m, BasicTransformerBlock):
                m.ctx_fused_max_width = 1280
        z_w, _ = _sampler(wide, which).sample(**kw)
    v = rel_l2(z_m.float().cpu(), z_0.double().cpu())
    report(f"narrow {which.upper()} 4 steps: latent with a collector vs without (no regions)", v, SAMPLER_OPT_TOL)
    assert v <= SAMPLER_OPT_TOL and torch.equal(z_m, z_w)
    res = cm.result((16, 16))
    assert float((res.double().sum(1) - 1).abs().max()) <= mr.ROW_BOUND and bool((res[1, 1] == 0).all())


def test_one_token_context_launches_nothing_new(dev, narrow, golden_dir):
    """K = 1: the maps are ones, the launches are exactly those of the run without a collector, and so are the bits."""
    from ldm.modules.attention import ContextMaps
    with torch.no_grad():
        c, _, _ = _conditioning(narrow, dev)
        kw = _sampler_kw(narrow, dev, golden_dir, c[:, :1].contiguous())
        cm = ContextMaps()
        (z_m, _), keys_m = _keys(lambda: _sampler(narrow, "plms").sample(conditioning_maps=cm, **kw))
        (z_0, _), keys_0 = _keys(lambda: _sampler(narrow, "plms").sample(**kw))
    assert keys_m == keys_0 and not any(k.startswith("xa") for k in keys_m), sorted(set(keys_m) ^ set(keys_0))
    assert torch.equal(z_m, z_0)
    assert torch.equal(cm.result((16, 16)), torch.ones(2, 1, 16, 16, device=dev))
    assert sorted(cm.per_level()) == [(2, 2), (4, 4), (8, 8), (16, 16)] and all(bool((v == 1).all()) for v in cm.per_level().values())


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_inference_cli_save_reference_maps(dev, golden_dir, tmp_path):
    """Two references with regions and --save_reference_maps: one PNG per reference at the picture size, byte-identical to
    pipeline.inpaint(return_ref_maps=True) quantised the same way; the dump carries ref_maps; the picture is the one without the flag."""
    import importlib.util
    import yaml
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_m", os.path.join(root, "scripts", "inference.py"))
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
                      "--dump_tensors", dump, "--reference_region", *reg_p, "--reference_weight", "2", "1"] + extra)
        return x, np.load(dump), out
    x_m, t, out = run("maps", ["--save_reference_maps"])
    x_0, t0, out0 = run("plain", [])
    assert torch.equal(x_m, x_0) and "ref_maps" in t.files and "ref_maps" not in t0.files
    assert not os.path.exists(os.path.join(out0, "reference_maps"))
    files = [os.path.join(out, "reference_maps", f"image_example_1_{seed}_ref{j}.png") for j in range(2)]
    assert sorted(os.listdir(os.path.join(out, "reference_maps"))) == [os.path.basename(f) for f in files]
    trip = preprocess.load_triple_device(img_p, msk_p, ref_p[0], dev)
    ref = torch.stack([trip["ref"], preprocess.load_triple_device(img_p, msk_p, ref_p[1], dev)["ref"]], 1)
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint(model, trip["image"], trip["mask"], ref, steps=steps, scale=5.0, x_T=torch.from_numpy(t["x_T"]).to(dev),
                                  post_eps=torch.from_numpy(t["post_eps"]).to(dev), sampler="plms", ref_weights=torch.from_numpy(t["reference_weight"]),
                                  ref_regions=torch.from_numpy(t["reference_region"]), return_ref_maps=True)
        u8 = pipeline.ref_maps_u8(direct["ref_maps"], (512, 512)).cpu().numpy()
    maps = direct["ref_maps"]
    assert tuple(maps.shape) == (1, 2, 64, 64) and torch.equal(maps.cpu(), torch.from_numpy(t["ref_maps"]))
    assert torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
    for j, path in enumerate(files):
        im = Image.open(path)
        assert im.mode == "L" and im.size == (512, 512)
        assert np.array_equal(np.array(im), u8[0, j])
        buf = io.BytesIO()
        Image.fromarray(u8[0, j], mode="L").save(buf, format="PNG")
        with open(path, "rb") as f:
            assert f.read() == buf.getvalue()
    # the regions took: the left reference holds the left half of the picture, the right one the right half
    m = maps.cpu()
    # (columns 24 .. 39 share a cell of the coarsest level with the resized boundary: left out)
    assert float(m[0, 0, :, :24].min()) > 0.99 and float(m[0, 0, :, 40:].max()) < 0.01 and float(m[0, 1, :, 40:].min()) > 0.99
    assert int(u8[0, 0, :, :180].min()) == 255 and int(u8[0, 0, :, 332:].max()) == 0
