"""Regional exemplars without a GPU: tests/regionref.py on itself (its reference and emulation against ctxref / kbiasref, the gate against
the table mutations), the level rule of ldm.modules.attention.prepare_context_regions, the oracle wrapper against plain algebra, and the
samplers' / pipeline's / CLI's host-side pieces."""
import importlib.util
import math
import os

import pytest
import torch

import ctxref as cr
import kbiasref as kr
import regionref as rr
from accgate import rel_l2
from oracle_loader import O
from pbe_amd.lib import PbeError

INF = math.inf


# ---- regionref on itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rr.SHAPES, ids=rr.shape_id)
def test_row_constant_table_is_the_weighted_reference(shape):
    B, N, C, H, Nk, parts, h, w = shape
    o = cr.random_operands(B, N, C, H, Nk, parts)
    wt = kr.ctx_weights(B, Nk, 3 + C)
    table = torch.log2(wt)[:, None, :].expand(B, N, Nk)
    want, term = rr.reference(o, table)
    want_w, term_w = cr.reference(kr.fold_log2w(o, wt))
    assert rel_l2(want, want_w) <= 1e-14 and rel_l2(term, term_w) <= 1e-13
    assert torch.equal(rr.emulate(o, table), cr.emulate(kr.fold_log2w(o, wt, through_fp32=True)))
    assert torch.equal(rr.emulate(o, torch.zeros(B, N, Nk)), cr.emulate(o))


@pytest.mark.parametrize("shape", rr.SHAPES, ids=rr.shape_id)
def test_gate_accepts_the_emulation_and_rejects_the_mutations(shape):
    B, N, C, H, Nk, parts, h, w = shape
    o = cr.random_operands(B, N, C, H, Nk, parts)
    case = rr.kernel_case(shape)
    table = case["table"]
    absent = float(torch.isinf(table).double().mean())
    assert 0.03 <= absent <= 0.3, absent                                       # a fair share of (row, token) pairs is absent
    assert all(bool(torch.isinf(case["bare_absent"][b, t]).all()) for b, t in enumerate(case["cells"]))
    assert bool(torch.isfinite(table.max(-1).values).all())                    # every row keeps a token
    want = rr.reference(o, table)[0]
    emu = rr.emulate(o, table)
    ok, text = cr.verdict(emu, want, emu)
    print(f"{rr.shape_id(shape)}: emulation {text}; {100 * absent:.1f} % of the table is -inf")
    assert ok, text
    for kind in rr.MUTATIONS:
        bad = rr.emulate(o, rr.mutate(case, kind, h, w))
        ok, text = cr.verdict(bad, want, emu)
        assert not ok, f"{kind} passed the gate: {text}"
    ok, text = cr.verdict(rr.emulate(o, rr.mutate(case, "bare_absent", h, w)), want, emu)
    assert not ok and text == "non-finite result", text


# ---- level_table / prepare_context_regions ---------------------------------------------------------------------------------------------
def test_area_average_hand_computed():
    """One sample, two tokens, a 4 x 4 map onto a 2 x 2 grid, weights (2, 0.5)."""
    r = torch.zeros(1, 2, 4, 4)
    r[0, 0, :2, :2] = torch.tensor([[1.0, 1.0], [0.0, 0.0]])                  # cell (0, 0): 1/2
    r[0, 0, 2:, 2:] = 1.0                                                      # cell (1, 1): 1
    r[0, 1, :2, 2:] = torch.tensor([[1.0, 0.0], [0.0, 0.0]])                  # cell (0, 1): 1/4
    r[0, 1, 2:, 2:] = 0.5                                                      # cell (1, 1): 1/2
    e = rr.level_weights(r, [[2.0, 0.5]], 2, 2)
    want = torch.tensor([[[1.0, 0.0], [0.0, 0.125], [2.0, 0.5], [2.0, 0.25]]], dtype=torch.float64)    # cell (1, 0): uncovered -> w
    assert torch.equal(e, want)
    from ldm.modules.attention import ContextRegions, prepare_context_regions
    cr_ = prepare_context_regions(torch.zeros(1, 2, 8), r, [[2.0, 0.5]])
    assert isinstance(cr_, ContextRegions) and prepare_context_regions(torch.zeros(1, 2, 8), cr_) is cr_
    assert prepare_context_regions(torch.zeros(1, 2, 8), None) is None
    assert torch.equal(cr_.level_weights(2, 2), want)
    t = cr_.level(2, 2)
    assert t.dtype == torch.float32 and tuple(t.shape) == (1, 4, 2) and t is cr_.level(2, 2)
    assert torch.equal(t, torch.log2(want).float()) and t[0, 0, 1] == -INF
    assert torch.equal(cr_.level(1, 1), torch.log2(torch.tensor([[[2.0 * 6 / 16, 0.5 * 3 / 16]]], dtype=torch.float64)).float())


@pytest.mark.parametrize("shape", rr.SHAPES[:3], ids=rr.shape_id)
def test_prepare_context_regions_is_the_level_rule(shape):
    from ldm.modules.attention import prepare_context_regions
    B, N, C, H, Nk, parts, h, w = shape
    case = rr.kernel_case(shape)
    ctx = torch.zeros(B, Nk, 8)
    got = prepare_context_regions(ctx, case["regions"], case["weights"]).level(h, w)
    assert torch.equal(got, case["table"].float())
    for b, t in enumerate(case["cells"]):                                    # fallback rows equal log2 w
        assert torch.equal(got[b, t], torch.log2(case["weights"][b]).float())
    # weight 0 removes a token everywhere, fallback rows included
    wz = case["weights"].clone()
    wz[:, 1] = 0.0
    tz = prepare_context_regions(ctx, case["regions"], wz).level(h, w)
    assert bool(torch.isinf(tz[:, :, 1]).all()) and bool(torch.isfinite(tz.max(-1).values).all())
    assert torch.equal(tz, rr.level_table(case["regions"], wz, h, w).float())
    # all-ones regions: log2 w on every row, at any resolution; without weights: zeros
    ones = torch.ones(B, Nk, 2 * h, 3 * w)
    assert torch.equal(prepare_context_regions(ctx, ones, case["weights"]).level(h, w), torch.log2(case["weights"]).float()[:, None, :].expand(B, N, Nk))
    assert torch.equal(prepare_context_regions(ctx, ones).level(h, w), torch.zeros(B, N, Nk))


def test_prepare_context_regions_refuses():
    from ldm.modules.attention import prepare_context_regions
    ctx = torch.zeros(2, 3, 8)
    good = torch.ones(2, 3, 8, 12)
    bad = [torch.ones(2, 3, 8), torch.ones(3, 3, 8, 12), torch.ones(2, 2, 8, 12), -good]
    for v in (float("nan"), INF):
        t = good.clone()
        t[1, 2, 3, 4] = v
        bad.append(t)
    for t in bad:
        with pytest.raises(PbeError):
            prepare_context_regions(ctx, t)
    with pytest.raises(PbeError):                                            # the weights are checked by prepare_context_weights
        prepare_context_regions(ctx, good, [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    cr_ = prepare_context_regions(ctx, good)
    cr_.level(4, 6), cr_.level(8, 12), cr_.level(1, 1)
    for h, w in ((3, 12), (8, 5), (16, 12)):
        with pytest.raises(PbeError, match=f"{h} x {w}"):
            cr_.level(h, w)
    # K = 1: validated all the same
    with pytest.raises(PbeError):
        prepare_context_regions(torch.zeros(2, 1, 8), -torch.ones(2, 1, 4, 4))


# ---- the oracle wrapper against plain algebra ------------------------------------------------------------------------------------------
def _st_sd(C, H, tag):
    """The state dict test_ctx_attention_gpu._st builds, on the host."""
    from ldm.modules.attention import SpatialTransformer
    from pbe_amd.weights import fill_module_
    st = SpatialTransformer(C, H, C // H, depth=1, context_dim=768)
    fill_module_(st, prefix=tag)
    torch.nn.init.normal_(st.proj_out.weight, std=0.05)
    return {tag + k: v.detach().float() for k, v in st.state_dict().items()}


def test_regional_oracle_is_the_per_subset_composition():
    C, H, h, w = 64, 8, 8, 12
    torch.manual_seed(0)
    sd = _st_sd(C, H, "st.")
    g = torch.Generator().manual_seed(C)
    x, ctx = torch.randn(2, C, h, w, generator=g), torch.randn(2, 3, 768, generator=g)
    r = rr.binary_regions(2, h, w)
    e = rr.level_weights(r, None, h, w)
    assert bool((e[0, 6 * w + 7] == 1).all()) and bool((e[1, 6 * w + 8] == 1).all())           # the uncovered cells fall back to all tokens
    assert len({tuple(v) for v in e[0].tolist()}) >= 4
    with torch.no_grad():
        plain = O.spatial_transformer(sd, "st.", x, ctx, H)
        with rr.regional_oracle(O, [rr.level_table(r, None, h, w)]):
            got = O.spatial_transformer(sd, "st.", x, ctx, H)
        again = O.spatial_transformer(sd, "st.", x, ctx, H)
        want = rr.subset_composition(lambda b, c: O.spatial_transformer(sd, "st.", x[b:b + 1], c, H), ctx, e)
    assert torch.equal(plain, again)                                         # the original is restored
    v, away = rel_l2(got, want.double()), rel_l2(got, plain.double())
    print(f"regional oracle vs per-subset composition: rel-L2 {v:.3e}; vs the regionless oracle {away:.3e}")
    assert v <= 1e-5, v
    from test_model_gpu import BLOCK_TOL
    assert away > 10 * BLOCK_TOL, away                                        # a path that drops the regions cannot pass BLOCK_TOL


def test_regional_oracle_guidance_pair_and_level_choice():
    C, H = 64, 8
    torch.manual_seed(0)
    sd = _st_sd(C, H, "st.")
    g = torch.Generator().manual_seed(5)
    x, ctx = torch.randn(1, C, 4, 6, generator=g), torch.randn(1, 3, 768, generator=g)
    r = rr.soft_regions(1, 3, 4, 6, seed=1, up=2)
    tables = [rr.level_table(r, [[2.0, 1.0, 0.5]], 4, 6), rr.level_table(r, [[2.0, 1.0, 0.5]], 2, 3)]
    with torch.no_grad():
        plain = O.spatial_transformer(sd, "st.", x, ctx, H)
        with rr.regional_oracle(O, tables):
            one = O.spatial_transformer(sd, "st.", x, ctx, H)
            pair = O.spatial_transformer(sd, "st.", torch.cat([x, x]), torch.cat([ctx, ctx]), H)
    assert torch.allclose(pair[:1], plain, atol=1e-5) and torch.allclose(pair[1:], one, atol=1e-5) and not torch.allclose(one, plain, atol=1e-3)


# ---- samplers, pipeline, CLI: the host side --------------------------------------------------------------------------------------------
def test_guidance_regions_of_the_samplers():
    from ldm.models.diffusion.plms import guidance_regions
    cond = torch.zeros(2, 3, 8)
    r = torch.rand(2, 3, 4, 6)
    assert guidance_regions(None, cond, 2, True) is None and guidance_regions(None, cond, 2, False) is None
    gr = guidance_regions(r, cond, 2, True)
    assert gr.dtype == torch.float64 and gr.device.type == "cpu" and tuple(gr.shape) == (4, 3, 4, 6)
    assert torch.equal(gr[:2], torch.ones(2, 3, 4, 6, dtype=torch.float64)) and torch.equal(gr[2:], r.double())
    assert torch.equal(guidance_regions(r, cond, 2, False), r.double())
    for bad in (torch.rand(2, 3, 4), torch.rand(2, 2, 4, 6), torch.rand(3, 3, 4, 6)):
        with pytest.raises(PbeError):
            guidance_regions(bad, cond, 2, True)


def test_pad_regions():
    from pbe_amd.pipeline import pad_regions
    a, b = torch.rand(2, 4, 6), torch.rand(3, 4, 6)
    out = pad_regions([a, b], 3)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, 3, 4, 6)
    assert torch.equal(out[0, :2], a.double()) and torch.equal(out[1], b.double()) and bool((out[0, 2] == 0).all())
    for bad in ([], [a, torch.rand(3, 4, 5)], [torch.rand(4, 4, 6)], [torch.rand(4, 6)]):
        with pytest.raises(PbeError):
            pad_regions(bad, 3)


def test_cli_reference_region_arguments():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_regions_cpu", os.path.join(root, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse(["--reference_path", "a.jpg", "b.jpg", "--reference_region", "a.png", "b.png", "--reference_weight", "2", "1"])
    assert opt.reference_region == ["a.png", "b.png"]
    assert cli.parse(["--reference_path", "a.jpg"]).reference_region is None
    for argv in (["--reference_path", "a.jpg", "b.jpg", "--reference_region", "a.png"],
                 ["--reference_path", "a.jpg", "--reference_region", "a.png", "b.png"]):
        with pytest.raises(SystemExit):
            cli.parse(argv)


def test_symbols_launch_key_and_route_limits():
    from ldm.modules.attention import BasicTransformerBlock
    from pbe_amd import lib, ops
    assert "pbe_ctx_attention_rw_f16" in lib.SYMBOLS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pbe_hip.h")).read()
    assert "int pbe_ctx_attention_rw_f16(const pbe_ctx_attn_desc* d, const float* log2rw, int64_t rw_bs, int64_t rw_rs, pbe_stream_t stream);" in hdr
    assert "log2rw" in ops.CtxOperands.__slots__
    blk = BasicTransformerBlock(1280, 8, 160, context_dim=768)
    assert not blk._ctx_fused(4)                                               # the speed bound still holds without regions
    blk._ctx_regional(4), blk._ctx_regional(16)                                # .. and does not apply with them
    with pytest.raises(PbeError, match="16"):
        blk._ctx_regional(20)
    with pytest.raises(PbeError, match="128"):
        BasicTransformerBlock(1280, 20, 64, context_dim=768)._ctx_regional(8)
