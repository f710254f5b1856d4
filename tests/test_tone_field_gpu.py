"""The tone field on the GPU: pbe_tone_cells_i32 (pbe_amd/csrc/tone_field.hip) against the integer table of tests/fieldref.py by equality
(inputs between poison, the table in a sentinel arena: tests/guard.py), pbe_tone_field_f32 against fp64 within the derived tolerance
with the workspace poisoned two ways, pbe_paste_window_field_u8 against fp64 under fieldref's gate and against the two other pastes
byte for byte, a planted ramp followed through the real kernels, pipeline.inpaint_window / inpaint_holes with tone="field" on the narrow
model against the same steps made by hand, and scripts/inference.py --match_tone field.

No test here judges picture quality: the weights are name-seeded noise."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import cases
import fieldref as fr
import guard
import maskref as mr
import modelbuild as build
import toneref as tr
import windowref as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, R = (128, 128), 8
F = np.float32


def _embed(a, dev, poison=None):
    """A contiguous array between poison (NaN for floats): (view in the array's shape, arena)."""
    view, arena = guard.embed(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), device=dev, poison=poison)
    return view.view(a.shape), arena


def _poison_workspace(dev, byte):
    from pbe_amd import ops
    ops._ws[(torch.device(dev).index or 0, "tone_field")] = torch.full((1 << 20,), byte, dtype=torch.uint8, device=dev)


# ---- 1. tone_cells ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fr.CELL_CASES, ids=fr.cell_case_id)
def test_tone_cells_is_the_integer_reference(dev, case):
    from pbe_amd import ops
    shape, mode, cell = case
    image, result, sel = tr.stats_inputs(shape, mode)
    want = fr.cells_ref(image, result, sel, cell)
    (iv, _), (rv, _), (sv, _) = _embed(image, dev), _embed(result, dev), _embed(sel, dev, poison=1.0)       # a sel read from outside would count
    flat, arena = guard.sentinel_out((want.size,), dtype=torch.int32, device=dev)
    table = flat.view(want.shape)
    back = ops.tone_cells(iv, rv, sv, cell, out=table)
    assert back.data_ptr() == table.data_ptr()
    guard.assert_untouched(arena, flat, f"tone_cells {case}")
    guard.assert_fully_written(flat, f"tone_cells {case}")
    got = table.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), f"tone_cells {case}: {int((got != want).sum())} of {want.size} elements differ"
    again = ops.tone_cells(iv, rv, sv, cell)                         # the table allocated by the wrapper: the same table
    assert again.dtype == torch.int32 and tuple(again.shape) == want.shape and np.array_equal(again.cpu().numpy(), want)
    if mode == "zeros":
        assert not got.any()
    if shape == (1, 64, 96) and mode == "mixed":                     # the same planes one float off 16-byte alignment: narrower loads
        def shifted(a, by):
            buf = torch.full((a.size + by,), float("nan"), dtype=torch.float32, device=dev)
            buf[by:].copy_(torch.from_numpy(a).reshape(-1))
            return buf[by:].view(a.shape)
        for by, rest in ((1, 4), (2, 8)):
            assert shifted(image, by).data_ptr() % 16 == rest
            assert np.array_equal(ops.tone_cells(shifted(image, by), shifted(result, by), shifted(sel, by), cell).cpu().numpy(), want)


def test_tone_field_ops_refuse_bad_arguments(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    image, result, sel = (torch.zeros(s, device=dev) for s in ((2, 3, 8, 8), (2, 3, 8, 8), (2, 1, 8, 8)))
    assert not ops.tone_cells(image, result, sel).any()
    with pytest.raises(PbeError, match="dtype"):
        ops.tone_cells(image.half(), result, sel)
    for bad in ((image[:, :2], result, sel), (image, result[:1], sel), (image, result, sel.expand(2, 3, 8, 8)), (image[0], result[0], sel[0])):
        with pytest.raises(PbeError, match="tone_cells"):
            ops.tone_cells(*bad)
    with pytest.raises(PbeError, match="contiguous"):
        ops.tone_cells(torch.zeros(2, 3, 8, 16, device=dev)[:, :, :, ::2], result, sel)
    for cell in (0, 3, 12, 128, True):
        with pytest.raises(PbeError, match="cell"):
            ops.tone_cells(image, result, sel, cell)
    with pytest.raises(PbeError, match="out"):
        ops.tone_cells(image, result, sel, out=torch.zeros(2, 4, 1, 1, dtype=torch.int64, device=dev))
    cells = torch.zeros(1, 4, 3, 2, dtype=torch.int32, device=dev)
    assert not ops.tone_field(cells).any()
    with pytest.raises(PbeError, match="dtype"):
        ops.tone_field(cells.long())
    with pytest.raises(PbeError, match="cells"):
        ops.tone_field(cells[:, :3])
    with pytest.raises(PbeError, match="2\\^20"):
        ops.tone_field(torch.zeros(1, 4, 1025, 1024, dtype=torch.int32, device=dev))
    for kw in (dict(limit=0.0), dict(limit=float("nan")), dict(limit=float("inf")), dict(limit=1e-60), dict(min_pixels=-1), dict(cell=5)):
        with pytest.raises(PbeError, match="tone_field"):
            ops.tone_field(cells, **kw)
    pic = torch.zeros(20, 30, 3, dtype=torch.uint8, device=dev)
    res, alpha, field = torch.zeros(3, 8, 8, device=dev), torch.ones(10, 10, device=dev), torch.zeros(3, 1, 1, device=dev)
    with pytest.raises(PbeError, match="field and tone"):
        ops.paste_window(res, alpha, pic, (0, 0, 10, 10), tone=((1, 1, 1), (0, 0, 0)), field=field)
    for bad, cell in ((torch.zeros(3, 2, 1, device=dev), 8), (field, 4), (field.half(), 8), (field, 7)):
        with pytest.raises(PbeError, match="field|cell"):
            ops.paste_window(res, alpha, pic, (0, 0, 10, 10), field=bad, cell=cell)
    assert not pic.any()


# ---- 2. tone_field ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", fr.FIELD_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_tone_field_against_fp64(dev, grid):
    from pbe_amd import ops
    tables = np.stack([fr.random_table(grid), fr.constant_table(grid, 7), fr.random_table(grid, seed=5, empty=0.6)])
    want = np.stack([fr.field64(t) for t in tables])
    tv, _ = _embed(tables, dev, poison=0x7F7F7F00)                   # a count read from outside the table would be huge
    tol = fr.field_tol(fr.levels_of(grid))
    got = []
    for byte in (0xA5, 0x7F):                                        # 0x7F7F7F7F is a huge float and a huge count
        _poison_workspace(tv.device, byte)
        flat, arena = guard.sentinel_out((want.size,), dtype=torch.float32, device=dev)
        out = flat.view(want.shape)
        back = ops.tone_field(tv, out=out)
        assert back.data_ptr() == out.data_ptr()
        guard.assert_untouched(arena, flat, f"tone_field {grid}")
        guard.assert_fully_written(flat, f"tone_field {grid}")
        got.append(out.cpu().numpy())
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32)), "the field depends on what the workspace held"
    err = float(np.abs(got[0].astype(np.float64) - want).max())
    emu = np.stack([fr.field32(t) for t in tables])
    print(f"tone_field {grid}: |got - fp64| <= {err:.3g} (tolerance {tol:.3g}), {int((got[0].view(np.int32) != emu.view(np.int32)).sum())} elements differ from the fp32 emulation")
    assert np.isfinite(got[0]).all() and err <= tol
    # the constant case gives equal bits: (float)(7 / 255) in every element
    assert np.array_equal(got[0][1].view(np.int32), np.full(want[1].shape, F(7 / 255.0), dtype=F).view(np.int32))
    # too little evidence: zeros, and every element written
    assert not ops.tone_field(tv, min_pixels=1 << 30).any()
    other = ops.tone_field(tv, limit=0.03).cpu().numpy()
    assert np.abs(other).max() <= 0.03 + fr.field_tol(fr.levels_of(grid), 0.03) and np.abs(other.astype(np.float64) - np.stack([fr.field64(t, limit=0.03) for t in tables])).max() <= fr.field_tol(fr.levels_of(grid), 0.03)


# ---- 3. paste_window(field=...) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fr.PASTE_CASES, ids=[c[0] for c in fr.PASTE_CASES])
def test_paste_window_field_against_fp64(dev, case):
    from pbe_amd import ops
    name, shape, win, size, cell = case
    pic, result, alpha, field = fr.paste_field_inputs(case)
    (rv, _), (av, _), (fv, _) = _embed(result, dev), _embed(alpha, dev), _embed(field, dev)
    pv, arena = _embed(pic, dev)
    back = ops.paste_window(rv, av, pv, win, field=fv, cell=cell)
    assert back.data_ptr() == pv.data_ptr()
    guard.assert_untouched(arena, pv.view(-1), f"paste_window field {name}", pattern=guard.POISON_BITS[torch.uint8])
    got = pv.cpu().numpy()
    changed, near, live = fr.gate_paste_field(got, pic, result, alpha, win, field, cell, what=f"paste_window field {name}")
    emu = fr.paste_field32(pic, result, alpha, win, field, cell)
    print(f"paste_window field {name}: {changed} of {live} bytes differ from the fp64 reference ({near} at a tie), {int((got != emu).sum())} from the fp32 emulation")
    assert (got != pic).any() and (got != wr.paste32(pic, result, alpha, win)).any()
    # a zero field is the plain entry and a constant field b the tone entry at gain 1, offset b: byte for byte
    plain, zero, tone, const = (_embed(pic, dev)[0] for _ in range(4))
    b = 0.0625
    ops.paste_window(rv, av, plain, win)
    ops.paste_window(rv, av, zero, win, field=torch.zeros_like(fv), cell=cell)
    ops.paste_window(rv, av, tone, win, tone=((1.0,) * 3, (b,) * 3))
    ops.paste_window(rv, av, const, win, field=torch.full_like(fv, b), cell=cell)
    assert torch.equal(plain, zero) and torch.equal(tone, const) and not torch.equal(plain, tone)


# ---- 4. a planted ramp through the kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fr.RAMP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_planted_ramp_is_followed_on_the_device(dev, shape):
    from pbe_amd import ops
    from pbe_amd.window import fit_tone, tone_field, tone_selection
    pic, mask, result, planted = fr.ramp_case(shape)
    win = (0, 0) + shape
    dp, dm, dr = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(result).to(dev)
    image = ops.window_image(dp, win, shape)
    sel = tone_selection(dm, win, shape, fr.RAMP_MARGIN)
    field, cells, summary = tone_field(image[None], dr[None], sel[None])
    want_cells = fr.cells_ref(wr.image32(pic, win, shape)[None], result[None], wr.mask_ref(mr.grow_ref(mask, fr.RAMP_MARGIN), win, shape)[None])
    assert np.array_equal(cells.cpu().numpy(), want_cells)
    levels = fr.levels_of(want_cells.shape[2:])
    assert np.abs(field.cpu().numpy()[0].astype(np.float64) - fr.field64(want_cells[0])).max() <= fr.field_tol(levels)
    s = summary[0]
    mean = fit_tone(ops.tone_stats(image[None], dr[None], sel[None]).cpu(), "mean")[0]
    assert s["mode"] == "field" and s["n"] == mean["n"] == int(want_cells[0, 0].sum()) and s["offset"] == mean["offset"], "the top of the pyramid is not mean-mode's offset"
    assert s["cell"] == 8 and s["grid"] == list(want_cells.shape[2:]) and s["levels"] == levels and not s["identity"]
    f = field.cpu().numpy()[0]
    assert np.allclose(s["field_min"], 255.0 * f.min(axis=(1, 2))) and np.allclose(s["field_max"], 255.0 * f.max(axis=(1, 2)))
    alpha = ops.feather_alpha(dm, win, fr.RAMP_FEATHER)
    zone = ((alpha > 0) & (alpha < 1)).cpu().numpy()
    ef, em = fr.ramp_errors(f, s["offset"], planted, zone)
    print(f"{shape}: rms error over the blend zone, grey levels: field {ef.round(3).tolist()}, one offset {em.round(3).tolist()}")
    assert (ef[:2] <= 0.25 * em[:2]).all()
    # and in the picture: the known pixels of the blend zone come back nearer to the original with the field than with one offset
    with_field = ops.paste_window(dr, alpha, dp.clone(), win, field=field[0]).cpu().numpy().astype(int)
    with_mean = ops.paste_window(dr, alpha, dp.clone(), win, tone=(mean["gain"], mean["offset"])).cpu().numpy().astype(int)
    known = zone & (mask < 128)
    rms = lambda a: float(np.sqrt(((a - pic.astype(int))[known][:, :2] ** 2).mean()))      # noqa: E731
    print(f"{shape}: rms byte difference on the known pixels of the blend zone: {rms(with_field):.3f} with the field, {rms(with_mean):.3f} with one offset")
    assert rms(with_field) < rms(with_mean)
    assert torch.equal(dp.cpu(), torch.from_numpy(pic))


# ---- 5. the pipeline -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def inp(dev):
    return {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}


def _two_pictures(dev):
    pics = [wr.random_picture((200, 300), 31), wr.random_picture((160, 144), 32)]
    masks = [np.zeros((200, 300), dtype=np.uint8), np.zeros((160, 144), dtype=np.uint8)]
    masks[0][70:130, 110:190] = 255          # the window is 160 x 160 -> scale 1.25 to 128 x 128
    masks[1][70:90, 60:80] = 200             # a small hole: the window is the working size, scale 1
    to = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return pics, masks, [to(p) for p in pics], [to(m) for m in masks]


def test_inpaint_window_with_field_equals_the_steps_by_hand(dev, narrow, inp):
    from pbe_amd import ops, pipeline
    from pbe_amd.lib import PbeError
    from pbe_amd.window import tone_field, tone_selection
    pics, masks, dp, dm = _two_pictures(dev)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, tone="field", **kw)
    base = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, **kw)
    assert "tone_stats" not in out and not {"tone", "tone_field", "tone_cells"} & set(base)
    assert torch.equal(out["latent"], base["latent"]) and torch.equal(out["image"], base["image"]), "tone changed the working-size result"
    wins = out["windows"]
    assert wins == base["windows"]
    result = base["image"].float().contiguous()
    sel = torch.stack([tone_selection(dm[i], wins[i], SIZE, 8) for i in range(2)])
    field, cells, summary = tone_field(base["inputs"]["image"], result, sel)
    assert torch.equal(out["tone_cells"], cells) and torch.equal(out["tone_field"], field) and out["tone"] == summary
    assert tuple(field.shape) == (2, 3, 16, 16) and tuple(cells.shape) == (2, 4, 16, 16)
    want_cells = fr.cells_ref(base["inputs"]["image"].cpu().numpy(), result.cpu().numpy(), sel.cpu().numpy())
    assert np.array_equal(cells.cpu().numpy(), want_cells)
    for i in range(2):
        s = summary[i]
        print(f"window {i}: n {s['n']}, offset {s['offset']}, field {s['field_min']} .. {s['field_max']} grey levels")
        assert s["n"] >= 64 and not s["identity"] and s["grid"] == [16, 16] and s["levels"] == 5
        assert np.abs(field[i].cpu().numpy().astype(np.float64) - fr.field64(want_cells[i])).max() <= fr.field_tol(5)
        hand = ops.paste_window(result[i], base["alphas"][i], dp[i].clone(), wins[i], field=field[i])
        assert torch.equal(out["pictures"][i], hand) and not torch.equal(out["pictures"][i], base["pictures"][i])
        assert torch.equal(dp[i].cpu(), torch.from_numpy(pics[i])), "the caller's picture was changed"
        fr.gate_paste_field(hand.cpu().numpy(), pics[i], result[i].cpu().numpy(), base["alphas"][i].cpu().numpy(), wins[i], field[i].cpu().numpy(),
                            what=f"inpaint_window field picture {i}")
    # the other arguments reach the field; tone_gain_limit is ignored
    other = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, tone="field", tone_margin=2, tone_cell=16, tone_field_limit=0.01,
                                    tone_gain_limit=1.0, **kw)
    assert tuple(other["tone_field"].shape) == (2, 3, 8, 8) and float(other["tone_field"].abs().max()) <= 0.01 + fr.field_tol(4, 0.01)
    assert other["tone"][0]["n"] > summary[0]["n"] and other["tone"][0]["cell"] == 16
    with pytest.raises(PbeError, match="tone_field|cell"):
        pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, tone="field", tone_cell=5, **kw)


def test_inpaint_holes_with_field_pastes_each_window_with_its_own_field(dev, narrow, inp):
    from pbe_amd import ops, pipeline
    from pbe_amd.window import tone_field, tone_selection
    pic = wr.random_picture((300, 400), 51)
    mask = np.zeros((300, 400), dtype=np.uint8)
    mask[30:50, 40:70] = 255
    mask[60:90, 106:126] = 129                                 # another group at feather 8, yet inside the first hole's window
    dp, dm = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"][:1], size=SIZE, feather=R, tone="field", batch=1, **kw)
    wins = [h["window"] for h in out["holes"]]
    assert len(wins) == 2 and len(out["tone"]) == 2 and tuple(out["tone_field"].shape) == (2, 3, 16, 16) and tuple(out["tone_cells"].shape) == (2, 4, 16, 16)
    assert "tone_stats" not in out
    labels = ops.mask_components(dm)
    own = [ops.select_components(labels, list(h["labels"])) for h in out["holes"]]
    result = out["image"].float().contiguous()
    sel = torch.stack([tone_selection(own[n], wins[n], SIZE, 8) for n in range(2)])      # each window's OWN mask
    field, cells, summary = tone_field(out["inputs"]["image"], result, sel)
    assert torch.equal(out["tone_cells"], cells) and torch.equal(out["tone_field"], field) and out["tone"] == summary
    assert not torch.equal(field[0], field[1])
    p = dp.clone()
    for n in (1, 0):
        ops.paste_window(result[n], out["alphas"][n], p, wins[n], field=field[n])
    assert torch.equal(out["pictures"][0], p)
    swapped = dp.clone()
    for n in (0, 1):
        ops.paste_window(result[n], out["alphas"][n], swapped, wins[n], field=field[1 - n])
    assert not torch.equal(out["pictures"][0], swapped), "the windows were not pasted each with its own field"
    assert torch.equal(dp.cpu(), torch.from_numpy(pic))


# ---- 6. the CLI ------------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_tone_field", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_inference_cli_match_tone_field(dev, golden_dir, tmp_path, capsys):
    """scripts/inference.py --paste_back --match_tone field: pasted/*.png is inpaint_window(tone="field")'s picture byte for byte and the
    .tone.json its summary; --tone_cell without --match_tone field is refused with a message that says so."""
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
    with pytest.raises(SystemExit, match="need --match_tone field"):
        cli.parse(common + ["--outdir", str(tmp_path / "no"), "--paste_back", "--match_tone", "mean", "--tone_cell", "16"])
    with pytest.raises(SystemExit, match="need --paste_back"):
        cli.parse(common + ["--outdir", str(tmp_path / "no"), "--match_tone", "field"])
    out, dump = str(tmp_path / "out"), str(tmp_path / "dump.npz")
    cli.main(common + ["--outdir", out, "--dump_tensors", dump, "--paste_back", "--context", str(context), "--feather", str(feather), "--match_tone", "field",
                       "--tone_cell", "16", "--tone_field_limit", "0.1"])
    printed = capsys.readouterr().out
    assert "tone of window 0: field over n = " in printed and "grid 32 x 32 cells of 16" in printed
    t = np.load(dump)
    ref = torch.from_numpy(u8["ref"]).to(dev)[None]
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint_window(model, [torch.from_numpy(canvas).to(dev)], [torch.from_numpy(cmask).to(dev)],
                                         ops.u8_to_planes(ref, preprocess.CLIP_MEAN, preprocess.CLIP_STD), size=(512, 512), context=context, feather=feather,
                                         steps=steps, scale=5.0, x_T=torch.from_numpy(t["x_T"]).to(dev), post_eps=torch.from_numpy(t["post_eps"]).to(dev), sampler="ddim",
                                         tone="field", tone_cell=16, tone_field_limit=0.1)
    assert torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
    pasted = np.asarray(Image.open(os.path.join(out, "pasted", f"picture_{seed}.png")))
    assert pasted.shape == (600, 680, 3) and np.array_equal(pasted, direct["pictures"][0].cpu().numpy())
    with open(os.path.join(out, "pasted", f"picture_{seed}.tone.json")) as f:
        fits = json.load(f)
    assert fits == direct["tone"] and len(fits) == 1 and fits[0]["mode"] == "field" and fits[0]["n"] >= 64 and fits[0]["grid"] == [32, 32]
    changed = (pasted != canvas).any(2)
    assert changed.any() and not changed[~wr.chebyshev_within(cmask, 2 * feather)].any()
    # --per_hole takes the same flags: one summary per window
    out_h = str(tmp_path / "out_holes")
    cli.main(common + ["--outdir", out_h, "--paste_back", "--per_hole", "--context", str(context), "--feather", str(feather), "--match_tone", "field"])
    with open(os.path.join(out_h, "pasted", f"picture_{seed}.tone.json")) as f:
        fits_h = json.load(f)
    n_windows = len([n for n in os.listdir(os.path.join(out_h, "results")) if n.endswith(".png")])
    assert len(fits_h) == n_windows >= 1 and all(f["mode"] == "field" and f["cell"] == 8 and f["grid"] == [64, 64] and not f["identity"] for f in fits_h)
    pasted_h = np.asarray(Image.open(os.path.join(out_h, "pasted", f"picture_{seed}.png")))
    assert pasted_h.shape == (600, 680, 3) and not (pasted_h != canvas).any(2)[~wr.chebyshev_within(cmask, 2 * feather)].any()
