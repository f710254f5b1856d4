"""One window per hole on the GPU: the three entry points of pbe_amd/csrc/holes.hip against the numpy restatement of tests/holesref.py,
by equality (masks between 0xFF poison bytes, which would read as hole pixels; outputs in sentinel arenas: tests/guard.py),
pipeline.inpaint_holes on the narrow model against inpaint_window and against the same steps made by hand, and
scripts/inference.py --per_hole.

No test here judges picture quality: the weights are name-seeded noise."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cases
import guard
import holesref as hr
import modelbuild as build
import windowref as wr
from test_model_gpu import report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_POISON = 0xFF           # a byte read from outside the mask would be a hole pixel


def _embed(a, dev, poison=None):
    view, arena = guard.embed(torch.from_numpy(np.array(a)).reshape(-1), device=dev, poison=poison)           # (a copy: the cases are read-only)
    return view.view(a.shape), arena


def _out(shape, dtype, dev):
    flat, arena = guard.sentinel_out((int(np.prod(shape)),), dtype=dtype, device=dev)
    return flat.view(shape), arena, flat


def _written(out, arena, flat, what):
    guard.assert_untouched(arena, flat, what)
    guard.assert_fully_written(flat, what)
    return out.cpu().numpy()


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", hr.PATTERNS)
def test_components_boxes_and_select_equal_the_reference(dev, pattern):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    for shape in hr.SHAPES:
        mask = hr.case_mask(pattern, shape)
        mv, _ = _embed(mask, dev, MASK_POISON)
        for conn in (8, 4):
            what = f"{pattern} {shape} at {conn}"
            ref = hr.case_labels(pattern, shape, conn)
            out, arena, flat = _out(shape, torch.int32, dev)
            back = ops.mask_components(mv, conn, out=out)
            assert back.data_ptr() == out.data_ptr()
            got = _written(out, arena, flat, f"mask_components {what}")
            assert np.array_equal(got, ref), f"mask_components {what}: {int((got != ref).sum())} of {ref.size} labels differ"
            want = hr.boxes_ref(ref)
            if want.shape[0] > 4096:
                with pytest.raises(PbeError, match=rf"{want.shape[0]} components.*capacity = 4096.*`capacity`"):
                    ops.component_boxes(out)
                count, table = ops.component_boxes(out, capacity=want.shape[0])                   # exactly enough
            else:
                count, table = ops.component_boxes(out)
            assert count == want.shape[0] and table.dtype == np.int64 and np.array_equal(table, want), f"component_boxes {what}"
            report(f"holes {what}: components", float(count), float(want.shape[0]))
            labels = want[:, 0].tolist()
            for tag, wanted in (("none", []), ("all", labels[:4096]), ("every second", labels[:8192:2])):
                sel, sarena, sflat = _out(shape, torch.uint8, dev)
                ops.select_components(out, wanted[::-1], out=sel)                                   # any order: the wrapper sorts
                got_sel = _written(sel, sarena, sflat, f"select_components {what} {tag}")
                assert np.array_equal(got_sel, hr.select_ref(ref, wanted)), f"select_components {what} {tag}"
            assert torch.equal(out.cpu(), torch.from_numpy(ref.astype(np.int32))), "component_boxes / select_components changed the labels"
        assert np.array_equal(mv.cpu().numpy(), mask), "the mask was changed"


def test_component_boxes_writes_its_rows_and_nothing_else(dev):
    """The entry point itself: rows from count on and everything around the table and the count keep the sentinel, also when the count
    exceeds the capacity (the table is then unspecified, the count true)."""
    from pbe_amd import lib, ops
    handle = lib.load()
    shape = (90, 130)
    stream = torch.cuda.current_stream().cuda_stream
    for pattern, conn, cap in (("diagonal", 8, 7), ("noise41", 8, 4096), ("checkerboard", 4, 4096), ("no_hole", 8, 5), ("wide_u", 4, 2), ("wide_u", 4, 1)):
        ref = hr.case_labels(pattern, shape, conn)
        want = hr.boxes_ref(ref)
        lv, _ = _embed(ref.astype(np.int32), dev, 7)                                                # a label read from outside the plane would be counted
        table, tarena, tflat = _out((cap, 6), torch.int32, dev)
        cnt, carena, cflat = _out((1,), torch.int32, dev)
        ws = torch.empty(handle.pbe_component_boxes_workspace_bytes(*shape, cap), dtype=torch.uint8, device=dev)
        lib.check(handle.pbe_component_boxes_i32(lv.data_ptr(), table.data_ptr(), cnt.data_ptr(), *shape, cap, ws.data_ptr(), ws.numel(), stream), "boxes")
        guard.assert_untouched(tarena, tflat, f"component_boxes table {pattern}")
        guard.assert_untouched(carena, cflat, f"component_boxes count {pattern}")
        n = int(cnt.cpu()[0])
        assert n == want.shape[0], (pattern, n)
        if n <= cap:
            got = table.cpu().numpy().astype(np.int64)
            assert np.array_equal(got[np.argsort(got[:n, 0])] if n else got[:0], want)
            assert (guard.bits(table[n:]) == guard.SENTINEL_BITS[torch.int32]).all(), "rows from count on were written"
    with pytest.raises(lib.PbeError, match="connectivity"):
        ops.mask_components(torch.zeros(4, 4, dtype=torch.uint8, device=dev), 6)
    with pytest.raises(lib.PbeError, match="dtype"):
        ops.mask_components(torch.zeros(4, 4, dtype=torch.int32, device=dev))
    with pytest.raises(lib.PbeError, match="contiguous"):
        ops.select_components(torch.zeros(4, 8, dtype=torch.int32, device=dev)[:, ::2], [0])
    with pytest.raises(lib.PbeError, match="4096"):
        ops.select_components(torch.zeros(4, 4, dtype=torch.int32, device=dev), list(range(4097)))
    with pytest.raises(lib.PbeError, match="capacity"):
        ops.component_boxes(torch.zeros(4, 4, dtype=torch.int32, device=dev), capacity=0)
    m4, l4, w4 = torch.zeros(4, 4, dtype=torch.uint8, device=dev), torch.zeros(4, 4, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    assert handle.pbe_mask_components_u8_i32(m4.data_ptr(), l4.data_ptr(), 4, 4, 6, w4.data_ptr(), 64, stream) != 0        # the entry point refuses it too


# ---- 2. inpaint_holes ------------------------------------------------------------------------------------------------------------------
SIZE, R = (128, 128), 8      # the smallest working size the window tests use


@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def inp(dev):
    return {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}


def _two_holes(dev):
    pic = wr.random_picture((300, 400), 51)
    mask = np.zeros((300, 400), dtype=np.uint8)
    mask[30:50, 40:70] = 255
    mask[35, 50] = 10                                          # a keep pixel inside the first hole
    mask[60:90, 106:126] = 129                                 # 37 columns to the right: another group at feather 8 (2 m = 34), yet inside
    mask[90, 126] = 128                                        # the first hole's window; this pixel joins it diagonally
    return pic, mask, torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev)


def test_one_group_is_inpaint_window(dev, narrow, inp):
    from pbe_amd import pipeline
    pics = [wr.random_picture((200, 300), 31), wr.random_picture((160, 144), 32)]
    masks = [np.zeros((200, 300), dtype=np.uint8), np.zeros((160, 144), dtype=np.uint8)]
    masks[0][70:130, 110:190] = 255
    masks[0][60:64, 100:104] = 200                             # a second component 7 rows above: the same group at feather 8
    masks[1][70:90, 60:80] = 200
    dp, dm = [torch.from_numpy(p).to(dev) for p in pics], [torch.from_numpy(m).to(dev) for m in masks]
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    one = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, **kw)
    out = pipeline.inpaint_holes(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, **kw)
    assert [h["window"] for h in out["holes"]] == one["windows"] and [h["sample"] for h in out["holes"]] == [0, 1]
    assert out["holes"][0]["labels"] == (60 * 300 + 100, 70 * 300 + 110) and out["holes"][0]["area"] == 60 * 80 + 16
    assert torch.equal(out["latent"], one["latent"]) and torch.equal(out["image"], one["image"])
    for i in range(2):
        assert torch.equal(out["inputs"]["mask"][i], one["inputs"]["mask"][i]) and torch.equal(out["alphas"][i], one["alphas"][i])
        assert torch.equal(out["pictures"][i], one["pictures"][i]) and not torch.equal(out["pictures"][i], dp[i])
        assert torch.equal(dp[i].cpu(), torch.from_numpy(pics[i])) and torch.equal(dm[i].cpu(), torch.from_numpy(masks[i]))
    # at feather 1 the two components of picture 0 are two holes: three windows now, and the leading sizes must follow
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError, match="x_T has leading size 2, expected 3"):
        pipeline.inpaint_holes(narrow, dp, dm, inp["ref"], size=SIZE, feather=1, **kw)
    with pytest.raises(PbeError, match="2 separate holes.*max_holes = 1"):
        pipeline.inpaint_holes(narrow, dp, dm, inp["ref"], size=SIZE, feather=1, max_holes=1, **kw)
    with pytest.raises(PbeError, match="no hole"):
        pipeline.inpaint_holes(narrow, dp[:1], [torch.zeros_like(dm[0])], inp["ref"][:1], size=SIZE, feather=R)


def test_two_far_holes_equal_the_steps_by_hand(dev, narrow, inp):
    from pbe_amd import ops, pipeline
    from pbe_amd.lib import PbeError
    from pbe_amd.window import plan_window_box
    pic, mask, dp, dm = _two_holes(dev)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"][:1], size=SIZE, feather=R, **kw)
    # by hand
    labels = ops.mask_components(dm)
    count, table = ops.component_boxes(labels)
    assert count == 2 and table[:, 0].tolist() == [30 * 400 + 40, 60 * 400 + 106] and table[:, 5].tolist() == [599, 601]
    own = [ops.select_components(labels, [int(l)]) for l in table[:, 0]]
    wins = [plan_window_box(tuple(int(v) for v in row[1:5]), mask.shape, SIZE, 0.5, R) for row in table]
    assert [h["window"] for h in out["holes"]] == wins and [h["box"] for h in out["holes"]] == [(30, 49, 40, 69), (60, 90, 106, 126)]
    assert [h["area"] for h in out["holes"]] == [599, 601] and [h["sample"] for h in out["holes"]] == [0, 0]
    report("inpaint_holes two far holes: windows", float(len(out["holes"])), 2.0)
    hand_in = pipeline.window_inputs([dp, dp], own, wins, SIZE)
    for k in ("image", "mask", "inpaint"):
        assert torch.equal(out["inputs"][k], hand_in[k]), k
    assert wins == [(0, 0, 128, 128), (11, 52, 128, 128)]                                           # each window holds (part of) the other hole,
    both = pipeline.window_inputs([dp, dp], [dm, dm], wins, SIZE)                                   # which the whole mask would show the model:
    assert not torch.equal(both["mask"][0], hand_in["mask"][0]) and not torch.equal(both["mask"][1], hand_in["mask"][1])
    ref2 = inp["ref"][[0, 0]]
    hand = pipeline.inpaint(narrow, hand_in["image"], hand_in["mask"], ref2, **kw)
    assert torch.equal(out["image"], hand["image"]) and torch.equal(out["latent"], hand["latent"]) and torch.equal(out["c"], hand["c"])
    alphas = [ops.feather_alpha(own[i], wins[i], R) for i in range(2)]
    result = hand["image"].float().contiguous()
    for order in ((0, 1), (1, 0)):
        p = dp.clone()
        for i in order:
            ops.paste_window(result[i], alphas[i], p, wins[i])
        assert torch.equal(out["pictures"][0], p), f"pasting in order {order} gives another picture"
    for i in range(2):
        assert torch.equal(out["alphas"][i], alphas[i])
    got = out["pictures"][0].cpu().numpy()
    far = ~wr.chebyshev_within(mask, 2 * R)
    changed = (got != pic).any(2)
    assert not changed[far].any() and far.mean() > 0.5, "a byte farther than 2 x feather from every hole changed"
    assert changed[30:50, 40:70].any() and changed[60:90, 106:126].any()                            # both holes were edited
    assert torch.equal(dp.cpu(), torch.from_numpy(pic)) and torch.equal(dm.cpu(), torch.from_numpy(mask))

    # batch = 1: two single-window inpaint calls
    single = pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"][:1], size=SIZE, feather=R, batch=1, **kw)
    for i in range(2):
        one = pipeline.inpaint(narrow, hand_in["image"][i:i + 1], hand_in["mask"][i:i + 1], inp["ref"][:1], steps=4, scale=5.0, x_T=inp["x_T"][i:i + 1],
                               post_eps=inp["post_eps"][i:i + 1])
        assert torch.equal(single["image"][i:i + 1], one["image"]) and torch.equal(single["latent"][i:i + 1], one["latent"])
    assert single["image"].shape == out["image"].shape and [h["window"] for h in single["holes"]] == wins

    # ref of leading size N: exemplar i goes to hole i
    routed = pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"], size=SIZE, feather=R, **kw)
    direct = pipeline.inpaint(narrow, hand_in["image"], hand_in["mask"], inp["ref"], **kw)
    assert torch.equal(routed["c"], direct["c"]) and not torch.equal(routed["c"][0], routed["c"][1])
    assert torch.equal(routed["c"][0], out["c"][0]) and torch.equal(out["c"][0], out["c"][1]) and not torch.equal(routed["c"][1], out["c"][1])
    assert torch.equal(routed["image"], direct["image"])
    with pytest.raises(PbeError, match="leading size 3.*1 .one per sample. or 2 .one per hole."):
        pipeline.inpaint_holes(narrow, [dp], [dm], torch.cat([inp["ref"], inp["ref"][:1]]), size=SIZE, feather=R, **kw)


# ---- 3. the CLI ------------------------------------------------------------------------------------------------------------------------
def test_inference_cli_per_hole(dev, golden_dir, tmp_path):
    """scripts/inference.py --paste_back --per_hole --reference_per_hole on a bundled triple set into a wider canvas beside a second hole:
    one set of files per hole, and pasted/*.png is inpaint_holes' picture byte for byte."""
    import yaml
    from PIL import Image
    from pbe_amd import ops, pipeline, preprocess
    from pbe_amd.window import plan_holes
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_holes_gpu", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    d = os.path.join(golden_dir, "examples")
    u8 = preprocess.load_triple_u8(os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png"), os.path.join(d, "reference_example_1.jpg"))
    canvas, cmask = wr.random_picture((600, 1400), 43), np.zeros((600, 1400), dtype=np.uint8)
    canvas[40:552, 90:602], cmask[40:552, 90:602] = u8["image"], u8["mask"]
    cmask[200:260, 1150:1230] = 255                                                              # the second hole, far to the right
    feather, seed, steps, size = 8, 321, 4, (512, 512)
    dm = torch.from_numpy(cmask).to(dev)
    plan = plan_holes(ops.component_boxes(ops.mask_components(dm))[1], cmask.shape, size, 0.5, feather)
    assert len(plan) == 2 and plan[1][1] == (200, 259, 1150, 1229), [p[1] for p in plan]
    Image.fromarray(canvas).save(str(tmp_path / "picture.png"))
    Image.fromarray(cmask, mode="L").save(str(tmp_path / "mask.png"))
    cfg = str(tmp_path / "narrow.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)
    refs = [os.path.join(d, "reference_example_1.jpg"), os.path.join(d, "reference_example_2.jpg")]
    base = ["--config", cfg, "--ddim_steps", str(steps), "--image_path", str(tmp_path / "picture.png"), "--mask_path", str(tmp_path / "mask.png"),
            "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights", "--paste_back", "--per_hole", "--feather", str(feather)]
    with pytest.raises(SystemExit, match="3 --reference_path images for 2 holes"):
        cli.main(base + ["--outdir", str(tmp_path / "bad"), "--reference_per_hole", "--reference_path", *refs, refs[0]])
    out = str(tmp_path / "out")
    x = cli.main(base + ["--outdir", out, "--reference_per_hole", "--reference_path", *refs])
    assert tuple(x.shape) == (2, 3, 512, 512)
    want = sorted([os.path.join("pasted", f"picture_{seed}.png")]
                  + [os.path.join(s, n.format(f"picture_hole{i}_{seed}")) for i in range(2)
                     for s, n in (("results", "{}.png"), ("grid", "grid-{}.png"), ("source", "{}_mask.png"), ("source", "{}_GT.png"), ("source", "{}_inpaint.png"),
                                  ("source", "{}_ref.png"))])
    have = sorted(os.path.join(s, n) for s in os.listdir(out) for n in os.listdir(os.path.join(out, s)))
    assert have == want
    ref = torch.stack([ops.u8_to_planes(torch.from_numpy(np.array(Image.open(r).convert("RGB").resize((224, 224)), dtype=np.uint8)).to(dev)[None],
                                        preprocess.CLIP_MEAN, preprocess.CLIP_STD)[0] for r in refs])
    shape = (2, 4, 64, 64)
    x_T = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    post_eps = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint_holes(model, [torch.from_numpy(canvas).to(dev)], [dm], ref, size=size, context=0.5, feather=feather, steps=steps, scale=5.0,
                                        x_T=x_T, post_eps=post_eps, sampler="ddim")
    assert torch.equal(direct["image"].cpu(), x)
    pasted = np.asarray(Image.open(os.path.join(out, "pasted", f"picture_{seed}.png")))
    assert pasted.shape == canvas.shape and np.array_equal(pasted, direct["pictures"][0].cpu().numpy())
    changed = (pasted != canvas).any(2)
    assert changed[:, :700].any() and changed[:, 1100:].any() and not changed[~wr.chebyshev_within(cmask, 2 * feather)].any()
    for i in range(2):
        res = np.asarray(Image.open(os.path.join(out, "results", f"picture_hole{i}_{seed}.png")))
        assert np.array_equal(res, (255.0 * direct["image"][i].float().cpu().permute(1, 2, 0).numpy()).astype(np.uint8))
