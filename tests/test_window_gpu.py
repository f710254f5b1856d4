"""Windowed inpainting on the GPU: the four kernels of pbe_amd/csrc/window.hip against the restatements and gates of tests/windowref.py
(pictures and masks between poison bytes, outputs in sentinel arenas: tests/guard.py), pipeline.inpaint_window on the narrow model
against the same steps made by hand and against the plain path, and scripts/inference.py --paste_back.

No test here judges picture quality: the weights are name-seeded noise."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cases
import guard
import modelbuild as build
import windowref as wr
from test_model_gpu import report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = ((0.5,) * 3, (0.5,) * 3)
CLIP = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
MASK_POISON = 0xFF           # a byte read from outside the mask would be a hole


def _embed_u8(a, dev, poison=None):
    """A contiguous uint8 picture / mask between poison bytes: (view in the array's shape, arena)."""
    view, arena = guard.embed(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), device=dev, poison=poison)
    return view.view(a.shape), arena


def _out(shape, dev):
    view, arena = guard.sentinel_out((int(np.prod(shape)),), dtype=torch.float32, device=dev)
    return view.view(shape), arena, view


def _written(out, arena, flat, what):
    guard.assert_untouched(arena, flat, what)
    guard.assert_fully_written(flat, what)
    return out.cpu().numpy()


# ---- 5. window_image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.IMAGE_CASES, ids=[c[0] for c in wr.IMAGE_CASES])
def test_window_image_against_fp64(dev, case):
    from pbe_amd import ops
    name, shape, win, size = case
    pic = wr.random_picture(shape, 5)
    pv, _ = _embed_u8(pic, dev)
    for tag, (mean, std) in (("half", HALF), ("clip", CLIP)):
        out, arena, flat = _out((3, *size), dev)
        ops.window_image(pv, win, size, mean, std, out=out)
        got = _written(out, arena, flat, f"window_image {name}")
        emu = wr.image32(pic, win, size, mean, std)
        print(f"window_image {name} {tag}: {int((got != emu).sum())} of {got.size} elements differ from the fp32 emulation")
        worst = wr.gate_image(got, pic, win, size, mean, std, f"window_image {name} {tag}")
        report(f"window_image {name} {tag} |err|/bound", worst, 1.0)
        if name == "identity":
            crop = torch.from_numpy(np.ascontiguousarray(wr.crop(pic, win))).to(dev)[None]
            assert torch.equal(out, ops.u8_to_planes(crop, mean, std)[0]), "the identity window is not u8_to_planes of the cropped bytes"


# ---- 6. window_mask --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.IMAGE_CASES, ids=[c[0] for c in wr.IMAGE_CASES])
def test_window_mask_is_the_integer_reference(dev, case):
    from pbe_amd import ops
    name, shape, win, size = case
    for seed in (4, 5):
        mask = wr.random_mask(shape, seed, blobs=3 if seed == 4 else 0)          # seed 5: a thin line and single pixels only
        y0, x0, wh, ww = win
        mask[y0 + wh // 2, x0 + ww // 3] = 128                                       # a single hole pixel inside, one in the window's last corner
        mask[y0 + wh - 1, x0 + ww - 1] = 255
        if y0 > 0:
            mask[y0 - 1, x0:x0 + ww] = 255                                           # ... and hole rows just outside it, which must not be seen
        if y0 + wh < shape[0]:
            mask[y0 + wh, x0:x0 + ww] = 255
        mv, _ = _embed_u8(mask, dev, MASK_POISON)
        out, arena, flat = _out((1, *size), dev)
        ops.window_mask(mv, win, size, out=out)
        got = _written(out, arena, flat, f"window_mask {name}")
        ref = wr.mask_ref(mask, win, size)
        assert np.array_equal(got, ref), f"window_mask {name}: {int((got != ref).sum())} working pixels differ"
        assert 0 < ref.mean() < 1
        if name == "identity":
            crop = torch.from_numpy(np.ascontiguousarray(wr.crop(mask, win))).to(dev)[None]
            assert torch.equal(out[None], ops.u8_to_planes(crop, mask_mode=1))


# ---- 7. feather_alpha ------------------------------------------------------------------------------------------------------------------
ALPHA_WINDOWS = [("whole", (0, 0, 90, 130)), ("flush_top_left", (0, 0, 60, 80)), ("flush_bottom_right", (41, 63, 49, 67)), ("interior", (20, 30, 40, 50)),
                 ("tiny", (40, 50, 10, 12)), ("one_pixel", (89, 129, 1, 1))]


@pytest.mark.parametrize("r", [0, 1, 3, 16, 40])
def test_feather_alpha_is_the_integer_reference(dev, r):
    """A hole in every picture corner, windows flush with the borders, r larger than the window ("tiny", "one_pixel": r = 16, 40)."""
    from pbe_amd import ops
    mask = wr.random_mask((90, 130), 7)
    mask[0, 0] = mask[-1, -1] = mask[0, -1] = mask[-1, 0] = 255
    mv, marena = _embed_u8(mask, dev, MASK_POISON)
    for name, win in ALPHA_WINDOWS:
        out, arena, flat = _out((win[2], win[3]), dev)
        ops.feather_alpha(mv, win, r, out=out)
        got = _written(out, arena, flat, f"feather_alpha {name} r={r}")
        ref = wr.alpha_ref(mask, win, r)
        assert np.array_equal(got, ref), f"feather_alpha {name} r={r}: {int((got != ref).sum())} of {ref.size} differ, max |diff| {np.abs(got - ref).max()}"
        assert np.all(got[wr.crop(mask, win) >= 128] == 1.0)
    assert torch.equal(mv.cpu(), torch.from_numpy(mask))
    # a few hole pixels in a larger picture: for the smaller radii most of the window is exactly 0
    big = np.zeros((300, 400), dtype=np.uint8)
    big[0, 399] = 200
    big[150:153, 200] = 128
    bv, _ = _embed_u8(big, dev, MASK_POISON)
    for win in ((100, 150, 110, 120), (0, 300, 60, 100)):
        got, ref = ops.feather_alpha(bv, win, r).cpu().numpy(), wr.alpha_ref(big, win, r)
        assert np.array_equal(got, ref) and (got == 1).any() and ((got == 0).any() or r == 40)        # at r = 40 every window pixel lies within 2r


# ---- 8. paste_window -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.PASTE_CASES, ids=[c[0] for c in wr.PASTE_CASES])
def test_paste_window_against_fp64(dev, case):
    from pbe_amd import ops
    name, shape, win, size = case
    pic, result, alpha = wr.paste_inputs(shape, win, size, 21)
    pv, arena = _embed_u8(pic, dev)
    flat = pv.view(-1)
    rv, _ = guard.embed(torch.from_numpy(result).reshape(-1), device=dev)
    av, _ = guard.embed(torch.from_numpy(alpha).reshape(-1), device=dev)
    back = ops.paste_window(rv.view(result.shape), av.view(alpha.shape), pv, win)
    assert back.data_ptr() == pv.data_ptr()
    guard.assert_untouched(arena, flat, f"paste_window {name}", pattern=guard.POISON_BITS[torch.uint8])
    got = pv.cpu().numpy()
    changed, near, live = wr.gate_paste(got, pic, result, alpha, win, f"paste_window {name}")
    emu = wr.paste32(pic, result, alpha, win)
    print(f"paste_window {name}: {changed} of {live} bytes differ from the fp64 reference ({near} at a tie), {int((got != emu).sum())} from the fp32 emulation")
    assert (got != pic).any()
    if name == "identity":                                  # alpha == 1 at scale 1: rint(255 result) exactly
        pv2, _ = _embed_u8(pic, dev)
        ops.paste_window(rv.view(result.shape), torch.ones_like(av).view(alpha.shape), pv2, win)
        want = np.rint(np.float32(255) * result).astype(np.uint8).transpose(1, 2, 0)
        assert np.array_equal(wr.crop(pv2.cpu().numpy(), win), want)
        # alpha == 0 everywhere: nothing is written at all
        pv3, arena3 = _embed_u8(pic, dev)
        ops.paste_window(rv.view(result.shape), torch.zeros_like(av).view(alpha.shape), pv3, win)
        assert torch.equal(pv3.cpu(), torch.from_numpy(pic))


def test_window_ops_refuse_bad_arguments(dev):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    pic, mask = torch.zeros(20, 30, 3, dtype=torch.uint8, device=dev), torch.zeros(20, 30, dtype=torch.uint8, device=dev)
    for win in ((0, 0, 21, 10), (-1, 0, 10, 10), (0, 25, 10, 6), (0, 0, 0, 5)):
        with pytest.raises(PbeError, match="not inside"):
            ops.window_image(pic, win, (8, 8))
        with pytest.raises(PbeError, match="not inside"):
            ops.window_mask(mask, win, (8, 8))
        with pytest.raises(PbeError, match="not inside"):
            ops.feather_alpha(mask, win, 2)
    with pytest.raises(PbeError, match="contiguous"):
        ops.window_image(torch.zeros(20, 60, 3, dtype=torch.uint8, device=dev)[:, ::2], (0, 0, 10, 10), (8, 8))
    with pytest.raises(PbeError, match="dtype"):
        ops.window_image(pic.float(), (0, 0, 10, 10), (8, 8))
    with pytest.raises(PbeError, match="dtype"):
        ops.paste_window(torch.zeros(3, 8, 8, device=dev).half(), torch.zeros(10, 10, device=dev), pic, (0, 0, 10, 10))
    with pytest.raises(PbeError, match="alpha"):
        ops.paste_window(torch.zeros(3, 8, 8, device=dev), torch.zeros(10, 11, device=dev), pic, (0, 0, 10, 10))
    with pytest.raises(PbeError, match="feather"):
        ops.feather_alpha(mask, (0, 0, 10, 10), -1)


# ---- 9. inpaint_window -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


def _two_pictures(dev):
    pics = [wr.random_picture((200, 300), 31), wr.random_picture((160, 144), 32)]
    masks = [np.zeros((200, 300), dtype=np.uint8), np.zeros((160, 144), dtype=np.uint8)]
    masks[0][70:130, 110:190] = 255          # 60 x 80: needs 120 x 160, so the window is 160 x 160 -> scale 1.25 to 128 x 128
    masks[0][75, 120] = 130
    masks[1][70:90, 60:80] = 200             # a small hole: the window is the working size, scale 1
    to = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return pics, masks, [to(p) for p in pics], [to(m) for m in masks]


def test_inpaint_window_equals_the_steps_by_hand(dev, narrow):
    from pbe_amd import ops, pipeline
    from pbe_amd.window import plan_window
    inp = {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}
    pics, masks, dp, dm = _two_pictures(dev)
    size, r = (128, 128), 8
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=size, feather=r, **kw)
    wins = [plan_window(m, size, 0.5, r) for m in masks]
    assert out["windows"] == wins == [(20, 70, 160, 160), (16, 6, 128, 128)]
    image = torch.stack([ops.window_image(dp[i], wins[i], size) for i in range(2)])
    mask = torch.stack([ops.window_mask(dm[i], wins[i], size) for i in range(2)])
    assert torch.equal(out["inputs"]["image"], image) and torch.equal(out["inputs"]["mask"], mask)
    assert torch.equal(out["inputs"]["inpaint"], ops.mul_planes(image, mask))
    hand = pipeline.inpaint(narrow, image, mask, inp["ref"], **kw)
    assert torch.equal(out["image"], hand["image"]) and torch.equal(out["latent"], hand["latent"])
    for i in range(2):
        alpha = ops.feather_alpha(dm[i], wins[i], r)
        assert torch.equal(out["alphas"][i], alpha)
        pasted = ops.paste_window(hand["image"][i].contiguous(), alpha, dp[i].clone(), wins[i])
        got = out["pictures"][i]
        assert got.dtype == torch.uint8 and got.shape == dp[i].shape and torch.equal(got, pasted)
        assert torch.equal(dp[i].cpu(), torch.from_numpy(pics[i])), "the caller's picture was changed"
        a_full = np.zeros(pics[i].shape[:2], dtype=np.float32)
        y0, x0, wh, ww = wins[i]
        a_full[y0:y0 + wh, x0:x0 + ww] = alpha.cpu().numpy()
        g = got.cpu().numpy()
        assert np.array_equal(g[a_full == 0], pics[i][a_full == 0]) and (g[a_full > 0] != pics[i][a_full > 0]).any()
        assert (a_full == 0).mean() > 0.2
        wr.gate_paste(g, pics[i], hand["image"][i].cpu().numpy(), alpha.cpu().numpy(), wins[i], f"inpaint_window picture {i}")
    # a caller's own windows pass through, validated
    own = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=size, feather=r, windows=[(20, 40, 150, 200), wins[1]], **kw)
    assert own["windows"][0] == (20, 40, 150, 200) and not torch.equal(own["inputs"]["image"][0], image[0]) and torch.equal(own["inputs"]["image"][1], image[1])
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError):
        pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=size, windows=[(0, 0, 201, 10), wins[1]], **kw)


def test_inpaint_window_at_the_working_size_is_the_plain_path(dev, narrow, tmp_path):
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    inp = {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}
    pic = wr.random_picture((128, 128), 33)
    mask = np.zeros((128, 128), dtype=np.uint8)
    mask[30:70, 50:100] = 255
    mask[5, 5] = 127
    paths = [str(tmp_path / n) for n in ("image.png", "mask.png", "ref.png")]
    Image.fromarray(pic).save(paths[0]); Image.fromarray(mask, mode="L").save(paths[1])
    Image.fromarray(wr.random_picture((224, 224), 34)).save(paths[2])
    trip = preprocess.load_triple_device(*paths, dev)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"][:1], post_eps=inp["post_eps"][:1])
    plain = pipeline.inpaint(narrow, trip["image"], trip["mask"], trip["ref"], **kw)
    out = pipeline.inpaint_window(narrow, [torch.from_numpy(pic).to(dev)], [torch.from_numpy(mask).to(dev)], trip["ref"], size=(128, 128), **kw)
    assert out["windows"] == [(0, 0, 128, 128)]
    assert torch.equal(out["inputs"]["image"], trip["image"]) and torch.equal(out["inputs"]["mask"], trip["mask"])
    assert torch.equal(out["inputs"]["inpaint"], trip["inpaint"])
    assert torch.equal(out["latent"], plain["latent"]) and torch.equal(out["image"], plain["image"])


def test_inpaint_window_passes_sampler_and_weights_through(dev, narrow):
    from pbe_amd import pipeline
    inp = {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}
    _, _, dp, dm = _two_pictures(dev)
    ref2 = torch.stack([inp["ref"], inp["ref"].flip(0)], 1)                     # [B, 2, 3, 224, 224]
    w = torch.tensor([[1.0, 0.25], [0.0, 2.0]], dtype=torch.float64)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"], sampler="dpm", ref_weights=w)
    out = pipeline.inpaint_window(narrow, dp, dm, ref2, size=(128, 128), **kw)
    hand = pipeline.inpaint(narrow, out["inputs"]["image"], out["inputs"]["mask"], ref2, **kw)
    other = pipeline.inpaint(narrow, out["inputs"]["image"], out["inputs"]["mask"], ref2, **{**kw, "sampler": "plms"})
    unweighted = pipeline.inpaint(narrow, out["inputs"]["image"], out["inputs"]["mask"], ref2, **{**kw, "ref_weights": None})
    assert torch.equal(out["latent"], hand["latent"]) and torch.equal(out["image"], hand["image"])
    assert not torch.equal(out["latent"], other["latent"]) and not torch.equal(out["latent"], unweighted["latent"])


# ---- 10. the CLI -----------------------------------------------------------------------------------------------------------------------
def test_inference_cli_paste_back(dev, golden_dir, tmp_path):
    """scripts/inference.py --paste_back on a bundled triple padded to a larger canvas: pasted/*.png is inpaint_window's picture byte for
    byte, and the H x W tree is that of a run without the flag on the cropped window."""
    import yaml
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    from pbe_amd.window import plan_window
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_window", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    d = os.path.join(golden_dir, "examples")
    u8 = preprocess.load_triple_u8(os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png"), os.path.join(d, "reference_example_1.jpg"))
    ref_path = os.path.join(d, "reference_example_1.jpg")
    canvas, cmask = wr.random_picture((600, 680), 41), np.zeros((600, 680), dtype=np.uint8)
    canvas[40:552, 90:602], cmask[40:552, 90:602] = u8["image"], u8["mask"]
    context, feather, seed, steps = 0.0, 8, 321, 4
    win = plan_window(cmask, (512, 512), context, feather)
    assert win[2:] == (512, 512) and win[:2] != (40, 90)                          # the working size, but not the embedded triple's rectangle
    for sub, (a, m) in (("canvas", (canvas, cmask)), ("crop", (wr.crop(canvas, win), wr.crop(cmask, win)))):
        os.makedirs(tmp_path / sub)
        Image.fromarray(np.ascontiguousarray(a)).save(str(tmp_path / sub / "picture.png"))
        Image.fromarray(np.ascontiguousarray(m), mode="L").save(str(tmp_path / sub / "mask.png"))
    cfg = str(tmp_path / "narrow.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)

    def run(sub, extra):
        out, dump = str(tmp_path / f"out_{sub}"), str(tmp_path / f"{sub}.npz")
        cli.main(extra + ["--outdir", out, "--config", cfg, "--ddim_steps", str(steps), "--image_path", str(tmp_path / sub / "picture.png"),
                          "--mask_path", str(tmp_path / sub / "mask.png"), "--reference_path", ref_path, "--seed", str(seed), "--scale", "5",
                          "--fixed_code", "--random_weights", "--dump_tensors", dump])
        return out, np.load(dump)
    out_c, t = run("canvas", ["--paste_back", "--context", str(context), "--feather", str(feather)])
    out_p, t0 = run("crop", [])
    assert tuple(t["window"]) == win and "window" not in t0.files and np.array_equal(t["latent"], t0["latent"])
    names = sorted(os.path.join(s, n) for s in ("source", "results", "grid") for n in os.listdir(os.path.join(out_p, s)))
    assert len(names) == 6 and not os.path.exists(os.path.join(out_p, "pasted"))
    for n in names:
        with open(os.path.join(out_c, n), "rb") as fa, open(os.path.join(out_p, n), "rb") as fb:
            assert fa.read() == fb.read(), n
    ref = torch.from_numpy(u8["ref"]).to(dev)[None]
    from pbe_amd import ops
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint_window(model, [torch.from_numpy(canvas).to(dev)], [torch.from_numpy(cmask).to(dev)],
                                         ops.u8_to_planes(ref, preprocess.CLIP_MEAN, preprocess.CLIP_STD), size=(512, 512), context=context, feather=feather,
                                         steps=steps, scale=5.0, x_T=torch.from_numpy(t["x_T"]).to(dev), post_eps=torch.from_numpy(t["post_eps"]).to(dev), sampler="ddim")
    assert torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
    pasted = np.asarray(Image.open(os.path.join(out_c, "pasted", f"picture_{seed}.png")))
    assert pasted.shape == (600, 680, 3) and np.array_equal(pasted, direct["pictures"][0].cpu().numpy())
    changed = (pasted != canvas).any(2)
    assert changed.any() and not changed[cmask_far(cmask, 2 * feather)].any()


def cmask_far(mask, d):
    """True where no hole pixel lies within Chebyshev distance d."""
    return ~wr.chebyshev_within(mask, d)
