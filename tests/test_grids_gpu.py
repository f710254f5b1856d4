"""Feature maps with H != W on the GPU: the 3x3 conv tiles on non-square maps against fp64 (tests/tilecheck.py: launch rule, sampling and
rounding model; tests/test_edges_gpu.py: poisoned operands and sentinel arenas), and the narrow model on a 24x16 latent grid (levels
24x16, 12x8, 6x4, 3x2) against the CPU oracle (oracle/pbe_oracle.py) at the tolerances of the same model at 16x16.

A halo-resident tile (10 .. 14) holds whole rows of one image or a whole number of images (tests/test_halo_plan_cpu.py states the
kernel's geometry): part (a) runs such tiles where an image holds 3, 6, 24 or 48 of them and where a tile holds 2 or 4 whole images of
H != W; part (b) runs maps a 128- or 256-pixel tile would split (12x8, 6x8, 3x8, 12x16, 24x8) and asserts the launch took a tile that
can express them."""
import pytest
import torch

import cases
import guard
import modelbuild as build
import tilecheck as tc
from oracle_loader import O
from test_edges_gpu import U32, _conv_check, _conv_operands, _same_bits
from test_halo_plan_cpu import HALO, geometry, tile_faults
from test_model_gpu import FWD_TOL, SAMPLER_OPT_TOL, report      # the project's tolerances and its parity report

pytestmark = pytest.mark.gpu
GROUPS = tc.GROUPS


# =====================================================================================================================================
# conv tiles
# =====================================================================================================================================
def _key(shape):
    return "c:" + ":".join(map(str, shape)) + ":1:1:0"


def _case(shape, request):
    """tilecheck.Case of the stride-1 conv (bias + row vector + residual + group statistics) with the (tile, split-K) the library plans
    for it under tile_cfg = request (-1: the heuristic)."""
    probe = tc.Case(_key(shape), 0)
    p = tc.plan(probe, tile_cfg=request)
    case = tc.Case(_key(shape), p[0] | (max(1, p[1]) << 8))
    case.bm, case.bn = p[2], p[3]
    return case


def _launch(case, dev, request):
    """run_case with `request` forced (pbe_tune key 1) -> (tensors, BM); the launch ran exactly the planned (tile, split-K)."""
    from pbe_amd import ops
    try:
        ops.tune(1, request)
        ops._PLANS = []
        t = tc.run_case(case, dev)
        plans = ops._PLANS
    finally:
        ops.tune(1, -1)
        ops._PLANS = None
    assert len(plans) == 1 and plans[0][0] == case.key, (case.describe(), plans)
    _, cfg, splits, bm, _, _ = plans[0]
    assert (cfg, max(1, splits)) == (case.tile, case.splits), f"{case.describe()}: launch ran tile {cfg} split-K {splits}"
    return t, bm


def _group_stats_ok(case, y):
    """The statistics the copy-out emitted (if any) against fp64 sums of the stored output: the limits of test_tuned_entry_against_fp64."""
    st = getattr(y, "_pbe_gstats", None)
    if st is None:
        return 0
    tot = st.view().double().sum(1)
    yg = y.double().view(case.B, case.Ho * case.Wo, st.groups, case.Cout // st.groups)
    ref = torch.stack([yg.sum((1, 3)), (yg ** 2).sum((1, 3))], -1)
    assert torch.allclose(tot, ref, rtol=2e-6, atol=1e-3), f"{case.id}: group statistics off by {(tot - ref).abs().max().item():.3e}"
    print(f"{case.describe()}: group statistics in {st.blocks} row block(s) per sample, off by {(tot - ref).abs().max().item():.3e}")
    return st.blocks


def _gate(case, t, bm):
    got, want, bound, labels = tc.sampled(case, t, bm)
    rep = tc.check(got, want, bound, case.describe(), labels)
    print(rep)
    return rep


HALO_GRIDS = [  # tile, (B, H, W, C1, C2, Cout), tiles per image (< 1: images per tile)
    (10, (2, 24, 32, 64, 0, 160), 3),
    (11, (2, 24, 16, 64, 64, 160), 3),           # two sources
    (11, (8, 4, 8, 128, 0, 160), 1 / 4),         # 4 whole 4x8 images per tile
    (12, (2, 12, 32, 128, 0, 320), 3),
    (13, (1, 96, 64, 64, 0, 128), 24),
    (13, (4, 8, 16, 64, 0, 128), 1 / 2),         # 2 whole 8x16 images per tile
    (14, (1, 6, 128, 64, 0, 128), 6),            # one 128-pixel row per tile
]


@pytest.mark.parametrize("tile,shape,per_image", HALO_GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_halo_tiles_on_non_square_maps(dev, tile, shape, per_image):
    """Each halo tile forced at split 1 on an H != W map: sampled elements within the fp64 bound, the bits of gather tile 9 at split 1,
    group statistics equal to fp64 sums of the stored output; then the same launch on NaN-poisoned operands with Y and the statistics in
    sentinel arenas (bit-identical to the contiguous launch, nothing outside written, everything inside written)."""
    from pbe_amd import ops
    B, H, W, C1, C2, Co = shape
    request = tile | (1 << 8)
    case = _case(shape, request)
    assert (case.tile, case.splits) == (tile, 1), case.describe()
    _, _, nsub, tiles_per_img = geometry(H, W, case.bm)
    assert (tiles_per_img if nsub == 1 else 1 / nsub) == per_image and tile_faults(B, H, W, case.bm) == ""
    with torch.no_grad():
        t, bm = _launch(case, dev, request)
        _gate(case, t, bm)
        y = t["out"]
        blocks = _group_stats_ok(case, y)
        assert blocks in (0, (H * W) // bm) and (blocks == 0 or (H * W) % bm == 0), (case.describe(), blocks)      # a row block is one tile
        try:
            ops.tune(1, 9 | (1 << 8))
            ops._PLANS = []
            y9 = ops.conv3x3(t["x1"], t["wpacked"], t["bias"], x2=t["x2"], **t["kw"])
            p9 = ops._PLANS[0]
        finally:
            ops.tune(1, -1)
            ops._PLANS = None
        assert (p9[1], max(1, p9[2])) == (9, 1), p9
        assert torch.equal(y, y9), f"{case.id}: halo tile {tile} and gather tile 9 differ in {int((y != y9).sum())} elements"
    # borders, poison and arenas (tests/test_edges_gpu.py)
    G = GROUPS if H * W >= 64 else 0
    e = _conv_operands(B, H, W, C1, C2, Co, 1, 1, 0, True, seed=H + W + Co + tile)
    what = f"halo conv {B}x{H}x{W}x({C1}+{C2})->{Co} tile {tile}"
    yy, gs0, gs1, _ = _conv_check(e, dev, what, cfg=request, groups=G)
    if not G:
        return
    (buf, arena, nblk), nblk0 = gs1, gs0[2]
    assert nblk == nblk0 == blocks
    used = B * nblk * G * 2
    guard.assert_untouched(arena, buf[:used], what + " [statistics]")
    if nblk == 0:
        return
    guard.assert_fully_written(buf[:used], what + " [statistics]")
    _same_bits(buf[:used], gs0[0][:used], what + " [statistics]")
    st = buf[:used].view(B, nblk, G, 2).double().cpu()
    yg = yy.double().cpu().view(B, nblk, (H * W) // nblk, G, Co // G)
    n = (H * W) // nblk * (Co // G)                  # a sum of n fp32 terms in any order is within n 2^-24 sum|term|
    for i, pw in ((0, 1), (1, 2)):
        want, mag = (yg ** pw).sum((2, 4)), (yg.abs() ** pw).sum((2, 4))
        assert ((st[..., i] - want).abs() <= n * U32 * mag + 1e-30).all(), (what, i, (st[..., i] - want).abs().max())


@pytest.mark.parametrize("shape,tile", [((4, 24, 16, 640, 0, 640), 12), ((4, 48, 32, 320, 0, 320), 10), ((2, 96, 64, 320, 0, 320), 11)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_heuristic_keeps_halo_tiles_on_whole_row_maps(dev, shape, tile):
    """Maps whose images hold 3, 6 and 48 tiles: the heuristic still plans a halo tile, and the result is within the bound."""
    case = _case(shape, -1)
    assert case.tile in HALO and case.tile == tile and tile_faults(*shape[:3], case.bm) == "", case.describe()
    with torch.no_grad():
        t, bm = _launch(case, dev, -1)
        _gate(case, t, bm)
        _group_stats_ok(case, t["out"])


SPLIT_IMAGE = [(4, 12, 8, 256, 0, 256), (8, 12, 8, 128, 0, 160), (4, 12, 16, 128, 0, 128), (4, 24, 8, 128, 0, 128), (8, 6, 8, 256, 0, 256),
               (16, 3, 8, 256, 0, 256), (4, 12, 8, 1280, 1280, 1280)]      # the last: the skip-concat ResBlock of a 512x768 run at batch 2 with guidance


@pytest.mark.parametrize("shape", SPLIT_IMAGE, ids=lambda s: "x".join(map(str, s)))
def test_maps_a_halo_tile_would_split(dev, shape):
    """Under the heuristic and with each halo tile requested (row vector, residual, group statistics): the launch takes no tile that
    fails the planner / kernel contract, and every sampled element is within its bound.  A request that resolves to a (tile, split-K)
    already gated on the same seeded operands is gated through its bits."""
    gated = {}
    for request in [-1] + [h | (1 << 8) for h in HALO]:
        case = _case(shape, request)
        if case.tile in HALO:
            assert tile_faults(*shape[:3], case.bm) == "", f"{case.describe()}: {tile_faults(*shape[:3], case.bm)}"
        with torch.no_grad():
            t, bm = _launch(case, dev, request)
            _group_stats_ok(case, t["out"])
            seen = gated.get((case.tile, case.splits))
            if seen is not None and torch.equal(seen, t["out"]):
                continue
            _gate(case, t, bm)
            gated[(case.tile, case.splits)] = t["out"]
    assert gated


def test_gate_rejects_rows_of_the_neighbouring_image(dev):
    """Positive control: what a 128-pixel tile over 96-pixel images would store - pixels 96 .. 127 (the first four rows of image 1) hold
    the rows of the image the tile staged - put into a host copy of a correct output: the gate, sampling for BM = 128, rejects it."""
    shape = (4, 12, 8, 256, 0, 256)
    case = _case(shape, -1)
    with torch.no_grad():
        t, _ = _launch(case, dev, -1)
        _gate(case, t, 128)
        bad = t["out"].cpu().clone()
        flat = bad.view(-1, case.Cout)
        flat[96:128] = flat[0:32]
        t["out"] = bad
        got, want, bound, labels = tc.sampled(case, t, 128)
    rep = tc.compare(got, want, bound, case.describe(), labels)
    assert rep.ratio > 1.0, f"rows of the neighbouring image not detected: {rep}"


# =====================================================================================================================================
# the narrow model on a 24x16 latent grid against the oracle
# =====================================================================================================================================
LH, LW = 24, 16


def check(name, got, ref, tol):
    got = got.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    v = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
    report(name, v, tol)
    assert v <= tol, f"{name}: rel-L2 {v:.3e} > {tol:.1e}"


@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def narrow_sd(narrow):
    return {k: v.detach().float().cpu() for k, v in narrow.state_dict().items()}


def _unet_sd(narrow_sd):
    return {k[len("model.diffusion_model."):]: v for k, v in narrow_sd.items() if k.startswith("model.diffusion_model.")}


@pytest.mark.parametrize("tokens", [1, 3])
def test_narrow_unet_forward_24x16(dev, narrow, narrow_sd, tokens):
    """B = 4: the 12x8 level is the shape class a 128-pixel halo tile would split.  3 tokens: the attention levels hold 384, 96, 24 and 6
    tokens (ragged key tiles, N % 64 != 0)."""
    g = torch.Generator().manual_seed(2416 + tokens)
    x, ctx = torch.randn(4, 9, LH, LW, generator=g), torch.randn(4, tokens, 768, generator=g)
    t = torch.full((4,), 981, dtype=torch.int64)
    with torch.no_grad():
        want = O.unet_forward(_unet_sd(narrow_sd), x, t, ctx, cases.UNET_NARROW)
        got = narrow.apply_model(x.to(dev), t.to(dev), ctx.to(dev))
    assert got.dtype == torch.float16 and got.shape == (4, 4, LH, LW)
    check(f"narrow UNetModel forward 24x16, {tokens}-token context", got, want, FWD_TOL)


def test_narrow_paired_prefix_is_bit_identical_24x16(dev, narrow):
    """forward_nhwc(paired=True) against the duplicated 2B evaluation (test_narrow_paired_prefix_is_bit_identical_multi_token) at 24x16."""
    from pbe_amd import ops
    g = torch.Generator().manual_seed(7)
    unet = narrow.model.diffusion_model
    for B, K in ((2, 1), (2, 3), (1, 3)):
        x = torch.randn(B, 4, LH, LW, generator=g).to(dev)
        z = torch.randn(B, 4, LH, LW, generator=g).to(dev)
        m = (torch.rand(B, 1, LH, LW, generator=g) > 0.3).float().to(dev)
        ctx = torch.randn(2 * B, K, 768, generator=g).to(dev)
        t = torch.full((2 * B,), 621, dtype=torch.int64, device=dev)
        with torch.no_grad():
            a = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 2), t, ctx)
            b = unet.forward_nhwc(ops.plms_pack_input(x, z, m, 1), t, ctx, paired=True)
        assert torch.equal(a, b), f"B={B} K={K}: {int((a != b).sum())} of {a.numel()} elements differ"
        assert not torch.equal(b[:B], b[B:])


def test_narrow_plms_24x16_against_oracle(dev, narrow, narrow_sd):
    """4 PLMS steps at scale 5 on 24x16 latents with a seeded z_inpaint and a seeded binary mask (5 U-Net calls on a guidance pair)."""
    from ldm.models.diffusion.plms import PLMSSampler
    g = torch.Generator().manual_seed(2417)
    x_T, z_inp = torch.randn(2, 4, LH, LW, generator=g), torch.randn(2, 4, LH, LW, generator=g) * 0.8
    m = (torch.rand(2, 1, LH, LW, generator=g) > 0.3).float()
    c = torch.randn(2, 1, 768, generator=g)
    with torch.no_grad():
        z0, _ = PLMSSampler(narrow).sample(S=4, batch_size=2, shape=[4, LH, LW], conditioning=c.to(dev), verbose=False, unconditional_guidance_scale=5.0,
                                           unconditional_conditioning=narrow.learnable_vector.repeat(2, 1, 1), eta=0.0, x_T=x_T.to(dev),
                                           test_model_kwargs={"inpaint_image": z_inp.to(dev), "inpaint_mask": m.to(dev)})
        sd = _unet_sd(narrow_sd)
        uc = narrow_sd["learnable_vector"].expand(2, 1, -1)
        want, info = O.plms_sample(lambda x9, t, ctx: O.unet_forward(sd, x9, t, ctx, cases.UNET_NARROW), 4, x_T, c, uc, 5.0, z_inp, m,
                                   O.schedule_buffers()["alphas_cumprod"])
    assert info["calls"] == 5 and z0.shape == (2, 4, LH, LW)
    check("narrow PLMS 4 steps, 24x16 latents", z0, want, SAMPLER_OPT_TOL)


def test_narrow_vae_12x8_latent(dev, narrow, narrow_sd):
    """first_stage_decode of a 12x8 latent (96x64 image) and first_stage_encode of a 96x64 image with injected eps (test_narrow_vae)."""
    g = torch.Generator().manual_seed(2418)
    z = torch.randn(2, 4, 12, 8, generator=g)
    img, eps = torch.rand(2, 3, 96, 64, generator=g) * 2 - 1, torch.randn(2, 4, 12, 8, generator=g)
    with torch.no_grad():
        dec = narrow.decode_first_stage(z.to(dev).clone())
        enc = narrow.get_first_stage_encoding(narrow.encode_first_stage(img.to(dev)), noise=eps)
        want_dec = O.first_stage_decode(narrow_sd, z, cases.VAE_NARROW, "first_stage_model.")
        want_enc = O.first_stage_encode(narrow_sd, img, eps, cases.VAE_NARROW, "first_stage_model.")
    assert dec.shape == (2, 3, 96, 64) and enc.shape == (2, 4, 12, 8)
    check("narrow decode_first_stage, 12x8 latent", dec, want_dec, FWD_TOL)
    check("narrow encode_first_stage+sample (injected eps), 96x64 image", enc, want_enc, FWD_TOL)
