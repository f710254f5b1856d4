"""Tone matching of a pasted window on the GPU: pbe_tone_stats_i64 (pbe_amd/csrc/tone.hip) against the integer table of
tests/toneref.py element for element (inputs between poison, the table in a sentinel arena, the workspace poisoned: tests/guard.py),
pbe_paste_window_tone_u8 against fp64 under toneref's gate and against the plain paste at tone (1, 0), a planted tone recovered
through the real kernels, pbe_amd.window.tone_selection against numpy, pipeline.inpaint_window / inpaint_holes with `tone` on the narrow
model against the same steps made by hand, and scripts/inference.py --match_tone.

No test here judges picture quality: the weights are name-seeded noise."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import cases
import guard
import maskref as mr
import modelbuild as build
import toneref as tr
import windowref as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, R = (128, 128), 8


def _embed(a, dev, poison=None):
    """A contiguous array between poison (NaN for floats): (view in the array's shape, arena)."""
    view, arena = guard.embed(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), device=dev, poison=poison)
    return view.view(a.shape), arena


def _stats_out(B, dev):
    """An int64 [B, 3, 6] table inside a sentinel arena of int32 halves (guard has no 64-bit pattern; the halves of a written element are
    a small count's, never the sentinel): (table, arena, the flat int32 view)."""
    flat, arena = guard.sentinel_out((B * 36,), dtype=torch.int32, device=dev)
    return flat.view(torch.int64).view(B, 3, 6), arena, flat


def _poison_workspace(dev, byte):
    from pbe_amd import ops
    ops._ws[(torch.device(dev).index or 0, "tone")] = torch.full((1 << 20,), byte, dtype=torch.uint8, device=dev)


# ---- 1. tone_stats ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mode", tr.STATS_CASES, ids=[f"{'x'.join(map(str, s))}_{m}" for s, m in tr.STATS_CASES])
def test_tone_stats_is_the_integer_reference(dev, shape, mode):
    from pbe_amd import ops
    image, result, sel = tr.stats_inputs(shape, mode)
    want = tr.stats_ref(image, result, sel)
    (iv, _), (rv, _), (sv, _) = _embed(image, dev), _embed(result, dev), _embed(sel, dev, poison=1.0)       # a sel read from outside would count
    _poison_workspace(iv.device, 0xA5)
    stats, arena, flat = _stats_out(shape[0], dev)
    back = ops.tone_stats(iv, rv, sv, out=stats)
    assert back.data_ptr() == stats.data_ptr()
    guard.assert_untouched(arena, flat, f"tone_stats {shape} {mode}")
    guard.assert_fully_written(flat, f"tone_stats {shape} {mode}")
    got = stats.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want), f"tone_stats {shape} {mode}: {int((got != want).sum())} of {want.size} elements differ:\n{got}\n{want}"
    # the workspace poisoned differently, the table allocated by the wrapper: the same table
    _poison_workspace(iv.device, 0x3C)
    again = ops.tone_stats(iv, rv, sv)
    assert again.dtype == torch.int64 and tuple(again.shape) == (shape[0], 3, 6) and np.array_equal(again.cpu().numpy(), want)
    if mode == "zeros":
        assert not got.any()
    if shape == (3, 64, 96):                                         # the same planes one float off 16-byte alignment: the scalar path
        def shifted(a):
            buf = torch.full((a.size + 1,), float("nan"), dtype=torch.float32, device=dev)
            buf[1:].copy_(torch.from_numpy(a).reshape(-1))
            return buf[1:].view(a.shape)
        assert shifted(image).data_ptr() % 16 == 4
        assert np.array_equal(ops.tone_stats(shifted(image), shifted(result), shifted(sel)).cpu().numpy(), want)


def test_tone_ops_refuse_bad_arguments(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    image, result, sel = (torch.zeros(s, device=dev) for s in ((2, 3, 8, 8), (2, 3, 8, 8), (2, 1, 8, 8)))
    assert not ops.tone_stats(image, result, sel).any()
    with pytest.raises(PbeError, match="dtype"):
        ops.tone_stats(image.half(), result, sel)
    with pytest.raises(PbeError, match="dtype"):
        ops.tone_stats(image, result, sel.double())
    for bad in ((image[:, :2], result, sel), (image, result[:1], sel), (image, result, sel.expand(2, 3, 8, 8)), (image[0], result[0], sel[0])):
        with pytest.raises(PbeError, match="tone_stats"):
            ops.tone_stats(*bad)
    with pytest.raises(PbeError, match="contiguous"):
        ops.tone_stats(torch.zeros(2, 3, 8, 16, device=dev)[:, :, :, ::2], result, sel)
    with pytest.raises(PbeError, match="GPU|device"):
        ops.tone_stats(image, result.cpu(), sel)
    with pytest.raises(PbeError, match="out"):
        ops.tone_stats(image, result, sel, out=torch.zeros(2, 3, 6, dtype=torch.int32, device=dev))
    pic = torch.zeros(20, 30, 3, dtype=torch.uint8, device=dev)
    for tone in ((1.0, 0.0), ((1, 1, 1), (0, 0, float("nan"))), ((1, 1), (0, 0))):
        with pytest.raises(PbeError, match="tone"):
            ops.paste_window(torch.zeros(3, 8, 8, device=dev), torch.ones(10, 10, device=dev), pic, (0, 0, 10, 10), tone=tone)
    assert not pic.any()


# ---- 2. paste_window(tone=...) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.PASTE_CASES, ids=[c[0] for c in wr.PASTE_CASES])
def test_paste_window_tone_against_fp64(dev, case):
    from pbe_amd import ops
    name, shape, win, size = case
    pic, result, alpha = wr.paste_inputs(shape, win, size, 21)
    rv, _ = _embed(result, dev)
    av, _ = _embed(alpha, dev)
    for gain, offset in tr.TONES:
        pv, arena = _embed(pic, dev)
        back = ops.paste_window(rv, av, pv, win, tone=(gain, offset))
        assert back.data_ptr() == pv.data_ptr()
        guard.assert_untouched(arena, pv.view(-1), f"paste_window tone {name}", pattern=guard.POISON_BITS[torch.uint8])
        got = pv.cpu().numpy()
        changed, near, live = tr.gate_paste_tone(got, pic, result, alpha, win, gain, offset, f"paste_window tone {name} {gain}")
        emu = tr.paste_tone32(pic, result, alpha, win, gain, offset)
        print(f"paste_window tone {name} {gain}: {changed} of {live} bytes differ from the fp64 reference ({near} at a tie), {int((got != emu).sum())} from the fp32 emulation")
        assert (got != pic).any() and (got != wr.paste32(pic, result, alpha, win)).any()
    # tone (1, 0) is the plain entry, byte for byte
    plain, _ = _embed(pic, dev)
    unit, _ = _embed(pic, dev)
    ops.paste_window(rv, av, plain, win)
    ops.paste_window(rv, av, unit, win, tone=((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    assert torch.equal(plain, unit) and not torch.equal(plain.cpu(), torch.from_numpy(pic))


# ---- 3. a planted tone is recovered through the kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("g0,b0", tr.RECOVERY)
def test_a_planted_tone_is_recovered_on_the_device(dev, g0, b0):
    from pbe_amd import ops
    from pbe_amd.window import fit_tone, tone_selection
    pic, mask, result = tr.recovery_case(g0, b0)
    win = tr.RECOVERY_WINDOW
    size = win[2:]
    dp, dm, dr = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(result).to(dev)
    image = ops.window_image(dp, win, size)
    sel = tone_selection(dm, win, size, tr.RECOVERY_MARGIN)
    assert np.array_equal(sel.cpu().numpy(), wr.mask_ref(mr.grow_ref(mask, tr.RECOVERY_MARGIN), win, size))
    stats = ops.tone_stats(image[None], dr[None], sel[None])
    assert np.array_equal(stats.cpu().numpy(), tr.stats_ref(wr.image32(pic, win, size)[None], result[None], sel.cpu().numpy()[None]))
    fit = fit_tone(stats.cpu())[0]
    alpha = ops.feather_alpha(dm, win, tr.RECOVERY_FEATHER)
    fixed = ops.paste_window(dr, alpha, dp.clone(), win, tone=(fit["gain"], fit["offset"])).cpu().numpy()
    plain = ops.paste_window(dr, alpha, dp.clone(), win).cpu().numpy()
    off_fixed, off_plain = np.abs(fixed.astype(int) - pic).max(), np.abs(plain.astype(int) - pic).max()
    print(f"planted ({g0}, {b0}): fitted gain {fit['gain']}, offset {fit['offset']}; largest byte difference {off_fixed} with the map, {off_plain} without")
    assert off_fixed <= 1 and off_plain >= 10
    assert torch.equal(dp.cpu(), torch.from_numpy(pic))


# ---- 4. tone_selection -----------------------------------------------------------------------------------------------------------------
def _two_pictures(dev):
    pics = [wr.random_picture((200, 300), 31), wr.random_picture((160, 144), 32)]
    masks = [np.zeros((200, 300), dtype=np.uint8), np.zeros((160, 144), dtype=np.uint8)]
    masks[0][70:130, 110:190] = 255          # the window is 160 x 160 -> scale 1.25 to 128 x 128
    masks[0][75, 120] = 130
    masks[1][70:90, 60:80] = 200             # a small hole: the window is the working size, scale 1
    to = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return pics, masks, [to(p) for p in pics], [to(m) for m in masks]


def _sel_ref(mask, win, size, margin):
    r = max(-((-margin * win[2]) // size[0]), -((-margin * win[3]) // size[1]))
    return wr.mask_ref(mr.grow_ref(mask, r) if r > 0 else mask, win, size), r


def test_tone_selection_is_grow_then_window_mask(dev):
    from pbe_amd.window import tone_selection
    _, masks, _, dm = _two_pictures(dev)
    for i, (win, radii) in enumerate((((20, 70, 160, 160), {8: 10, 0: 0, 3: 4}), ((16, 6, 128, 128), {8: 8, 0: 0, 1: 1}))):
        for margin, r_want in radii.items():
            want, r = _sel_ref(masks[i], win, SIZE, margin)
            got = tone_selection(dm[i], win, SIZE, margin)
            assert r == r_want and got.dtype == torch.float32 and tuple(got.shape) == (1, *SIZE)
            assert np.array_equal(got.cpu().numpy(), want), f"picture {i}, margin {margin}: {int((got.cpu().numpy() != want).sum())} working pixels differ"
            assert 0 < want.mean() < 1
        assert torch.equal(dm[i].cpu(), torch.from_numpy(masks[i]))
    # an anisotropic window: the larger of the two axes' radii
    want, r = _sel_ref(masks[0], (10, 60, 180, 140), (64, 96), 8)
    assert r == 23 and np.array_equal(tone_selection(dm[0], (10, 60, 180, 140), (64, 96), 8).cpu().numpy(), want)


# ---- 5. the pipeline -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def inp(dev):
    return {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}


def _same_fits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x == y, (x, y)


def test_inpaint_window_with_tone_equals_the_steps_by_hand(dev, narrow, inp):
    from pbe_amd import ops, pipeline
    from pbe_amd.window import fit_tone, tone_selection
    pics, masks, dp, dm = _two_pictures(dev)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, tone="affine", **kw)
    base = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, **kw)
    assert "tone" not in base and "tone_stats" not in base
    assert torch.equal(out["latent"], base["latent"]) and torch.equal(out["image"], base["image"]), "tone changed the working-size result"
    wins = out["windows"]
    assert wins == base["windows"] == [(20, 70, 160, 160), (16, 6, 128, 128)]
    result = base["image"].float().contiguous()
    want = tr.stats_ref(out["inputs"]["image"].cpu().numpy(), result.cpu().numpy(), np.stack([_sel_ref(masks[i], wins[i], SIZE, 8)[0] for i in range(2)]))
    assert out["tone_stats"].dtype == torch.int64 and np.array_equal(out["tone_stats"].cpu().numpy(), want)
    sel = torch.stack([tone_selection(dm[i], wins[i], SIZE, 8) for i in range(2)])
    stats = ops.tone_stats(base["inputs"]["image"], result, sel)
    assert torch.equal(out["tone_stats"], stats)
    fits = fit_tone(stats.cpu(), "affine", 1.25)
    _same_fits(out["tone"], fits)
    _same_fits(out["tone"], tr.fit_ref(want))
    for i in range(2):
        f = fits[i]
        print(f"window {i}: n {f['n']}, gain {f['gain']}, offset {f['offset']}, clamped {f['clamped']}, rms {f['rms_before']} -> {f['rms_after']}")
        assert f["n"] >= 64 and not f["identity"]
        hand = ops.paste_window(result[i], base["alphas"][i], dp[i].clone(), wins[i], tone=(f["gain"], f["offset"]))
        assert torch.equal(out["pictures"][i], hand) and not torch.equal(out["pictures"][i], base["pictures"][i])
        assert torch.equal(dp[i].cpu(), torch.from_numpy(pics[i])), "the caller's picture was changed"
        tr.gate_paste_tone(hand.cpu().numpy(), pics[i], result[i].cpu().numpy(), base["alphas"][i].cpu().numpy(), wins[i], f["gain"], f["offset"],
                           f"inpaint_window tone picture {i}")
    # the other arguments reach the fit
    other = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, tone="affine", tone_margin=2, tone_gain_limit=1.0, **kw)
    assert all(f["gain"] == [1.0] * 3 for f in other["tone"]) and other["tone"][0]["n"] > fits[0]["n"]
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError, match="tone"):
        pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, tone="median", **kw)


def test_inpaint_holes_with_tone_pastes_each_window_through_its_own_map(dev, narrow, inp):
    from pbe_amd import ops, pipeline
    from pbe_amd.window import fit_tone, tone_selection
    pic = wr.random_picture((300, 400), 51)
    mask = np.zeros((300, 400), dtype=np.uint8)
    mask[30:50, 40:70] = 255
    mask[35, 50] = 10
    mask[60:90, 106:126] = 129                                 # another group at feather 8, yet inside the first hole's window
    mask[90, 126] = 128
    dp, dm = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"][:1], size=SIZE, feather=R, tone="mean", **kw)
    wins = [h["window"] for h in out["holes"]]
    assert wins == [(0, 0, 128, 128), (11, 52, 128, 128)] and len(out["tone"]) == 2 and tuple(out["tone_stats"].shape) == (2, 3, 6)
    labels = ops.mask_components(dm)
    own = [ops.select_components(labels, list(h["labels"])) for h in out["holes"]]
    result = out["image"].float().contiguous()
    # each window's selection comes from its OWN mask: the other group's hole is a known pixel there and counts
    sel = torch.stack([tone_selection(own[n], wins[n], SIZE, 8) for n in range(2)])
    whole = torch.stack([tone_selection(dm, wins[n], SIZE, 8) for n in range(2)])
    assert not torch.equal(sel[0], whole[0]) and not torch.equal(sel[1], whole[1])
    stats = ops.tone_stats(out["inputs"]["image"], result, sel)
    assert torch.equal(out["tone_stats"], stats)
    assert np.array_equal(stats.cpu().numpy(), tr.stats_ref(out["inputs"]["image"].cpu().numpy(), result.cpu().numpy(), sel.cpu().numpy()))
    fits = fit_tone(stats.cpu(), "mean")
    _same_fits(out["tone"], fits)
    assert all(f["gain"] == [1.0] * 3 for f in fits) and fits[0]["offset"] != fits[1]["offset"]
    p = dp.clone()
    for n in (1, 0):
        ops.paste_window(result[n], out["alphas"][n], p, wins[n], tone=(fits[n]["gain"], fits[n]["offset"]))
    assert torch.equal(out["pictures"][0], p)
    swapped = dp.clone()
    for n in (0, 1):
        ops.paste_window(result[n], out["alphas"][n], swapped, wins[n], tone=(fits[1 - n]["gain"], fits[1 - n]["offset"]))
    assert not torch.equal(out["pictures"][0], swapped), "the windows were not pasted each through its own map"
    assert torch.equal(dp.cpu(), torch.from_numpy(pic))


# ---- 6. the CLI ------------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_tone", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_inference_cli_match_tone(dev, golden_dir, tmp_path):
    """scripts/inference.py --paste_back --match_tone affine: pasted/*.png is inpaint_window(tone="affine")'s picture byte for byte and the
    .tone.json its 'tone'; --match_tone without --paste_back is refused with a message that says so."""
    import yaml
    from PIL import Image
    from pbe_amd import ops, pipeline, preprocess
    cli = _cli()
    d = os.path.join(golden_dir, "examples")
    ref_path = os.path.join(d, "reference_example_1.jpg")
    u8 = preprocess.load_triple_u8(os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png"), ref_path)
    canvas, cmask = wr.random_picture((600, 680), 41), np.zeros((600, 680), dtype=np.uint8)
    canvas[40:552, 90:602], cmask[40:552, 90:602] = u8["image"], u8["mask"]
    context, feather, seed, steps = 0.0, 8, 321, 4
    Image.fromarray(canvas).save(str(tmp_path / "picture.png"))
    Image.fromarray(cmask, mode="L").save(str(tmp_path / "mask.png"))
    cfg = str(tmp_path / "narrow.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)
    common = ["--config", cfg, "--ddim_steps", str(steps), "--image_path", str(tmp_path / "picture.png"), "--mask_path", str(tmp_path / "mask.png"),
              "--reference_path", ref_path, "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights"]
    with pytest.raises(SystemExit, match="need --paste_back"):
        cli.parse(common + ["--outdir", str(tmp_path / "no"), "--match_tone", "affine"])
    with pytest.raises(SystemExit, match="need --paste_back"):
        cli.parse(common + ["--outdir", str(tmp_path / "no"), "--tone_margin", "4"])
    out, dump = str(tmp_path / "out"), str(tmp_path / "dump.npz")
    cli.main(common + ["--outdir", out, "--dump_tensors", dump, "--paste_back", "--context", str(context), "--feather", str(feather), "--match_tone", "affine"])
    t = np.load(dump)
    ref = torch.from_numpy(u8["ref"]).to(dev)[None]
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint_window(model, [torch.from_numpy(canvas).to(dev)], [torch.from_numpy(cmask).to(dev)],
                                         ops.u8_to_planes(ref, preprocess.CLIP_MEAN, preprocess.CLIP_STD), size=(512, 512), context=context, feather=feather,
                                         steps=steps, scale=5.0, x_T=torch.from_numpy(t["x_T"]).to(dev), post_eps=torch.from_numpy(t["post_eps"]).to(dev), sampler="ddim",
                                         tone="affine")
    assert torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
    pasted = np.asarray(Image.open(os.path.join(out, "pasted", f"picture_{seed}.png")))
    assert pasted.shape == (600, 680, 3) and np.array_equal(pasted, direct["pictures"][0].cpu().numpy())
    with open(os.path.join(out, "pasted", f"picture_{seed}.tone.json")) as f:
        fits = json.load(f)
    _same_fits(fits, direct["tone"])
    assert len(fits) == 1 and fits[0]["n"] >= 64
    changed = (pasted != canvas).any(2)
    assert changed.any() and not changed[~wr.chebyshev_within(cmask, 2 * feather)].any()
    # --per_hole takes the same flags: one fit per window, in the mean mode every gain is 1
    out_h = str(tmp_path / "out_holes")
    cli.main(common + ["--outdir", out_h, "--paste_back", "--per_hole", "--context", str(context), "--feather", str(feather), "--match_tone", "mean",
                       "--tone_margin", "4"])
    with open(os.path.join(out_h, "pasted", f"picture_{seed}.tone.json")) as f:
        fits_h = json.load(f)
    n_windows = len([n for n in os.listdir(os.path.join(out_h, "results")) if n.endswith(".png")])
    assert len(fits_h) == n_windows >= 1 and all(f["gain"] == [1.0] * 3 and not f["identity"] for f in fits_h)
    pasted_h = np.asarray(Image.open(os.path.join(out_h, "pasted", f"picture_{seed}.png")))
    assert pasted_h.shape == (600, 680, 3) and not (pasted_h != canvas).any(2)[~wr.chebyshev_within(cmask, 2 * feather)].any()
