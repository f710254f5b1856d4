"""The shape of a mask on the GPU: the entry points of pbe_amd/csrc/maskshape.hip against the numpy restatement of tests/maskref.py, by
equality.  Masks lie between poison bytes that would join the set the distance is taken to (0xFF for the hole, 0x00 for the rest), outputs
in sentinel arenas (tests/guard.py).  Then pbe_amd.window.shape_mask, pipeline.inpaint_window / inpaint_holes with `mask_shape` on the
narrow model against the same calls on a mask shaped by hand, and scripts/inference.py --mask_grow / --mask_box.

No test here judges picture quality: the weights are name-seeded noise."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cases
import guard
import holesref as hr
import maskref as mr
import modelbuild as build
import windowref as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poison(to_hole):
    return 0xFF if to_hole else 0x00         # a byte read from outside the mask would join the set


def _embed(a, dev, poison):
    view, arena = guard.embed(torch.from_numpy(np.array(a)).reshape(-1), device=dev, poison=poison)           # (a copy: the cases are read-only)
    return view.view(a.shape), arena


def _out(shape, dtype, dev):
    flat, arena = guard.sentinel_out((int(np.prod(shape)),), dtype=dtype, device=dev)
    return flat.view(shape), arena, flat


def _written(out, arena, flat, what):
    guard.assert_untouched(arena, flat, what)
    guard.assert_fully_written(flat, what)
    return out.cpu().numpy()


# ---- 1. the distance map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", hr.PATTERNS)
def test_mask_dist2_equals_the_reference(dev, pattern):
    from pbe_amd import ops
    n = 0
    for shape in mr.SHAPES:
        mask = mr.case_mask(pattern, shape)
        for to_hole in (True, False):
            mv, _ = _embed(mask, dev, _poison(to_hole))
            for rmax in [r for p, s, r in mr.DIST2_CASES if p == pattern and s == shape]:
                what = f"mask_dist2 {pattern} {shape} to_hole={to_hole} rmax={rmax}"
                ref = mr.case_dist2(pattern, shape, to_hole, rmax)
                out, arena, flat = _out(shape, torch.int32, dev)
                back = ops.mask_dist2(mv, to_hole, rmax, out=out)
                assert back.data_ptr() == out.data_ptr()
                got = _written(out, arena, flat, what)
                bad = got != ref
                print(f"{what}: {int(bad.sum())} of {ref.size} differ, max {int(got.max())} (saturation {rmax * rmax + 1})")
                assert not bad.any(), f"{what}: {int(bad.sum())} of {ref.size} values differ, first at {tuple(np.argwhere(bad)[0])}"
                n += 1
            assert np.array_equal(mv.cpu().numpy(), mask), "the mask was changed"
    assert n == 2 * sum(1 for c in mr.DIST2_CASES if c[0] == pattern) == 2 * 27


def test_mask_dist2_saturates_at_rmax_squared_plus_one_and_allocates_its_result(dev):
    from pbe_amd import ops
    mask = mr.case_mask("last_corner", (90, 130))                                                  # true distances up to 156: far beyond rmax
    mv = torch.from_numpy(np.array(mask)).to(dev)
    for rmax in (0, 1, 7, 33):
        got = ops.mask_dist2(mv, True, rmax).cpu().numpy()
        assert got.dtype == np.int32 and got[0, 0] == rmax * rmax + 1 == got.max() and got[89, 129] == 0
        if rmax:
            assert got[89, 129 - rmax] == rmax * rmax and got[89 - rmax, 129] == rmax * rmax and got[89, 128 - rmax] == rmax * rmax + 1
    empty = ops.mask_dist2(torch.zeros((67, 1031), dtype=torch.uint8, device=dev), rmax=33)         # no hole pixel at all
    assert bool((empty == 33 * 33 + 1).all())
    full = ops.mask_dist2(torch.full((3, 2000), 200, dtype=torch.uint8, device=dev), to_hole=False)   # the default rmax = 2047
    assert bool((full == 2047 * 2047 + 1).all())
    one = torch.zeros((5, 4200), dtype=torch.uint8, device=dev)
    one[2, 0] = 255                                                                                # taps up to 2047 columns away, through 17 segments
    far = ops.mask_dist2(one).cpu().numpy()
    xs = np.arange(4200, dtype=np.int64)
    assert np.array_equal(far, np.minimum((np.arange(5)[:, None] - 2) ** 2 + xs[None] ** 2, 2047 * 2047 + 1))


# ---- 2. grow, close, open --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", mr.GROW_PATTERNS)
def test_grow_close_open_equal_the_reference(dev, pattern):
    from pbe_amd import ops
    for shape in mr.GROW_SHAPES:
        mask = mr.case_mask(pattern, shape)
        views = {t: _embed(mask, dev, _poison(t))[0] for t in (True, False)}
        for r in mr.GROW_R:
            for name, fn, ref_fn, first_to_hole in (("mask_grow", ops.mask_grow, mr.grow_ref, r >= 0), ("mask_close", ops.mask_close, mr.close_ref, True),
                                                    ("mask_open", ops.mask_open, mr.open_ref, False)):
                rr = r if name == "mask_grow" else abs(r)
                what = f"{name} {pattern} {shape} r={rr}"
                out, arena, flat = _out(shape, torch.uint8, dev)
                back = fn(views[first_to_hole], rr, out=out)
                assert back.data_ptr() == out.data_ptr()
                got, ref = _written(out, arena, flat, what), ref_fn(mask, rr)
                assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.size} bytes differ"
        for v in views.values():
            assert np.array_equal(v.cpu().numpy(), mask), "the mask was changed"


def test_grow_of_single_pixels_and_an_unaligned_result(dev):
    from pbe_amd import ops
    one = torch.zeros((41, 43), dtype=torch.uint8, device=dev)
    one[20, 20] = 128
    one[0, 42] = 127                                                                               # not a hole pixel
    for r, n in ((0, 1), (1, 5), (1.5, 9), (2, 13), (3, 29)):
        assert int((ops.mask_grow(one, r) == 255).sum()) == n, r
    assert not bool(ops.mask_grow(one, -1).any())
    # a result that starts on an odd byte takes the kernel's byte-by-byte path
    mask = mr.case_mask("blobs", (129, 257))
    mv = torch.from_numpy(np.array(mask)).to(dev)
    arena = torch.full((mask.size + 64,), 0xA5, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        arena.fill_(0xA5)
        out = arena[off:off + mask.size].view(mask.shape)
        ops.mask_grow(mv, 2.5, out=out)
        assert np.array_equal(out.cpu().numpy(), mr.grow_ref(mask, 2.5))
        assert bool((arena[:off] == 0xA5).all()) and bool((arena[off + mask.size:] == 0xA5).all())


# ---- 3. boxes --------------------------------------------------------------------------------------------------------------------------
def test_fill_boxes_equals_the_reference(dev):
    from pbe_amd import lib, ops
    rs = np.random.RandomState(5)
    for shape in ((90, 130), (129, 257), (1, 300), (300, 1)):
        Hs, Ws = shape
        ya, xa = rs.randint(0, Hs, size=4096), rs.randint(0, Ws, size=4096)
        many = np.stack([ya, np.minimum(ya + rs.randint(0, 3, size=4096), Hs - 1), xa, np.minimum(xa + rs.randint(0, 4, size=4096), Ws - 1)], 1)
        sets = {"none": np.zeros((0, 4), dtype=np.int64),
                "corners": np.array([[0, 0, 0, 0], [0, 0, Ws - 1, Ws - 1], [Hs - 1, Hs - 1, 0, 0], [Hs - 1, Hs - 1, Ws - 1, Ws - 1]]),
                "whole": np.array([[0, Hs - 1, 0, Ws - 1]]),
                "nested": np.array([[Hs // 4, Hs // 2, Ws // 4, Ws // 2], [Hs // 3, 3 * Hs // 4, Ws // 3, 3 * Ws // 4], [Hs // 3, Hs // 3, Ws // 3, Ws // 3],
                                    [0, Hs - 1, Ws // 2, Ws // 2], [Hs // 2, Hs // 2, 0, Ws - 1]]),
                "4096": many, "77": many[:77]}
        for tag, boxes in sets.items():
            ref = mr.fill_boxes_ref(boxes, shape)
            for where in ("host", "device"):
                what = f"fill_boxes {shape} {tag} boxes on the {where}"
                arg = boxes.tolist() if where == "host" and tag != "none" else torch.from_numpy(boxes).to(dev if where == "device" else "cpu")
                out, arena, flat = _out(shape, torch.uint8, dev)
                back = ops.fill_boxes(arg, shape, out=out)
                assert back.data_ptr() == out.data_ptr()
                got = _written(out, arena, flat, what)
                assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.size} bytes differ"
    fresh = ops.fill_boxes(torch.tensor([[2, 3, 4, 5]], device=dev), (8, 9))                        # no out: on the boxes' device
    assert fresh.device == dev and fresh.dtype == torch.uint8 and int(fresh.sum()) == 255 * 4
    assert int(ops.fill_boxes([[2, 3, 4, 5]], (8, 9), device=dev).sum()) == 255 * 4
    # a refused box: at the wrapper, and at the entry point itself, which then writes nothing
    for bad in ([[0, 8, 0, 1]], [[3, 2, 0, 1]], [[0, 1, 5, 4]], [[0, 1, 0, 9]], [[-1, 1, 0, 1]]):
        with pytest.raises(lib.PbeError, match="box 0"):
            ops.fill_boxes(bad, (8, 9), device=dev)
        with pytest.raises(lib.PbeError, match="box 1"):
            ops.fill_boxes(torch.tensor([[0, 0, 0, 0]] + bad, device=dev), (8, 9))
        handle, stream = lib.load(), torch.cuda.current_stream().cuda_stream
        rows = torch.tensor([[0, 0, 0, 0]] + bad, dtype=torch.int32, device=dev)
        out, arena, flat = _out((8, 9), torch.uint8, dev)
        assert handle.pbe_fill_boxes_u8(rows.data_ptr(), 2, out.data_ptr(), 8, 9, stream) != 0
        assert b"box 1" in handle.pbe_last_error()
        torch.cuda.synchronize()
        assert bool((guard.bits(arena) == guard.SENTINEL_BITS[torch.uint8]).all()), "a refused call wrote something"
    assert handle.pbe_fill_boxes_u8(rows.data_ptr(), 4097, out.data_ptr(), 8, 9, stream) != 0
    assert handle.pbe_fill_boxes_u8(rows.data_ptr(), 1, out.data_ptr(), 8, 9, stream) == 0          # row 0 alone is a box
    torch.cuda.synchronize()
    assert int(out.sum()) == 255


# ---- 4. shape_mask ---------------------------------------------------------------------------------------------------------------------
def _fragments():
    """Two halves of one object 2 pixels apart, a second object, a speck, and a tight silhouette (a disc)."""
    m = np.zeros((129, 257), dtype=np.uint8)
    m[20:50, 20:40] = 255
    m[20:50, 42:60] = 200                                      # the gap: columns 40, 41
    yy, xx = np.mgrid[0:129, 0:257]
    m[(yy - 90) ** 2 + (xx - 180) ** 2 <= 15 ** 2] = 129
    m[5, 250] = 128                                            # the speck
    m[6, 250] = 127
    return m


def test_shape_mask_equals_the_reference(dev):
    from pbe_amd import ops
    from pbe_amd.window import shape_mask
    chains = [{}, {"open": 1.5}, {"close": 2}, {"grow": 6}, {"grow": -2.5}, {"box": True}, {"box": True, "connectivity": 4},
              {"open": 1, "close": 1.5, "grow": 4, "box": True}, {"open": 1, "close": 2, "grow": -1}, {"grow": 6, "box": True}]
    for name, mask in (("fragments", _fragments()), ("blobs", mr.case_mask("blobs", (90, 130))), ("threshold4", mr.case_mask("threshold4", (90, 130)))):
        mv = torch.from_numpy(np.array(mask)).to(dev)
        for kw in chains:
            if name == "threshold4" and kw.get("box") and "open" not in kw:
                continue                                                                           # thousands of components: more boxes than fill_boxes takes
            got = shape_mask(mv, **kw)
            assert got.dtype == torch.uint8 and got.data_ptr() != mv.data_ptr()
            ref = mr.shape_mask_ref(mask, **kw)
            assert np.array_equal(got.cpu().numpy(), ref), f"shape_mask {name} {kw}: {int((got.cpu().numpy() != ref).sum())} bytes differ"
        assert np.array_equal(mv.cpu().numpy(), mask), "shape_mask changed its input"
    mv = torch.from_numpy(_fragments()).to(dev)
    count = lambda m: ops.component_boxes(ops.mask_components(m))[0]                               # noqa: E731
    assert count(mv) == 4
    closed = shape_mask(mv, close=1.5)
    assert count(closed) == 3 and bool((closed[20:50, 40:42] == 255).all())                        # the two halves are one hole now
    opened = shape_mask(mv, open=1)
    assert count(opened) == 3 and int(opened[5, 250]) == 0 and int(opened[30, 30]) == 255          # the speck is gone
    boxed = shape_mask(mv, open=1, close=1.5, box=True)
    assert count(boxed) == 2 and ops.component_boxes(ops.mask_components(boxed))[1][:, 1:5].tolist() == [[20, 49, 20, 59], [75, 105, 165, 195]]
    assert int((boxed == 255).sum()) == 30 * 40 + 31 * 31
    assert not bool(shape_mask(mv, open=40).any())                                                 # nothing survives: not an error here


def test_the_wrappers_refuse_before_any_launch(dev):
    from pbe_amd import lib, ops
    from pbe_amd.window import shape_mask
    m = torch.zeros((8, 16), dtype=torch.uint8, device=dev)
    calls = {"mask_dist2": lambda x: ops.mask_dist2(x), "mask_grow": lambda x: ops.mask_grow(x, 2), "mask_close": lambda x: ops.mask_close(x, 2),
             "mask_open": lambda x: ops.mask_open(x, 2), "shape_mask": lambda x: shape_mask(x, grow=2), "shape_mask box": lambda x: shape_mask(x, box=True)}
    for name, call in calls.items():
        with pytest.raises(lib.PbeError, match="dtype"):
            call(m.to(torch.int32))
        with pytest.raises(lib.PbeError, match="contiguous"):
            call(m[:, ::2])
        with pytest.raises(lib.PbeError, match="16384"):
            call(torch.zeros((1, 16385), dtype=torch.uint8, device=dev))
    for call in (lambda: ops.mask_grow(m, 2048), lambda: ops.mask_grow(m, -2047.5), lambda: ops.mask_close(m, 2048), lambda: ops.mask_open(m, 2048),
                 lambda: ops.mask_close(m, -1), lambda: ops.mask_open(m, -0.5), lambda: ops.mask_dist2(m, rmax=2048), lambda: ops.mask_dist2(m, rmax=1.5),
                 lambda: ops.mask_dist2(m, rmax=-1), lambda: ops.mask_grow(m, float("nan")), lambda: shape_mask(m, grow=2048), lambda: shape_mask(m, close=-1)):
        with pytest.raises(lib.PbeError, match="2047"):
            call()
    with pytest.raises(lib.PbeError, match="connectivity"):
        shape_mask(m, box=True, connectivity=6)
    board = torch.from_numpy(np.array(mr.case_mask("checkerboard", (90, 130)))).to(dev)                # 5850 components at connectivity 4
    with pytest.raises(lib.PbeError, match=r"shape_mask: the box stage found more than 4096 components.*open="):
        shape_mask(board, box=True, connectivity=4)
    assert int((shape_mask(board, box=True) == 255).sum()) == 90 * 130                             # one component at 8: its box is the picture
    with pytest.raises(lib.PbeError, match="out must be"):
        ops.mask_grow(m, 1, out=torch.zeros((8, 15), dtype=torch.uint8, device=dev))
    with pytest.raises(lib.PbeError, match="dtype"):
        ops.mask_dist2(m, out=torch.zeros((8, 16), dtype=torch.int64, device=dev))
    # the entry points themselves
    handle, stream = lib.load(), torch.cuda.current_stream().cuda_stream
    d2, ws = torch.zeros((8, 16), dtype=torch.int32, device=dev), torch.zeros(4096, dtype=torch.uint8, device=dev)
    assert handle.pbe_mask_dist2_u8_i32(m.data_ptr(), d2.data_ptr(), 8, 16, 1, 2048, ws.data_ptr(), ws.numel(), stream) != 0
    assert handle.pbe_mask_dist2_u8_i32(m.data_ptr(), d2.data_ptr(), 8, 16, 2, 3, ws.data_ptr(), ws.numel(), stream) != 0
    assert handle.pbe_mask_dist2_u8_i32(m.data_ptr(), d2.data_ptr(), 8, 16, 1, 3, ws.data_ptr(), 255, stream) != 0
    assert handle.pbe_mask_dist2_u8_i32(m.data_ptr(), d2.data_ptr(), 8, 16385, 1, 3, ws.data_ptr(), ws.numel(), stream) != 0
    assert handle.pbe_mask_from_dist2_u8(d2.data_ptr(), m.data_ptr(), 8, 16, -1, 0, stream) != 0
    assert handle.pbe_mask_from_dist2_u8(d2.data_ptr(), m.data_ptr(), 8, 16, 4, 2, stream) != 0
    assert handle.pbe_mask_dist2_u8_i32(m.data_ptr(), d2.data_ptr(), 8, 16, 1, 3, ws.data_ptr(), 256, stream) == 0        # exactly enough
    torch.cuda.synchronize()
    assert bool((d2 == 10).all())


# ---- 5. the pipeline on the narrow model -----------------------------------------------------------------------------------------------
SIZE, R, STEPS = (128, 128), 8, 2      # the smallest working size the window tests use


@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def inp(dev):
    return {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("ref", "x_T", "post_eps")}


def _silhouettes(dev):
    pics = [wr.random_picture((200, 300), 61), wr.random_picture((160, 144), 62)]
    masks = [np.zeros((200, 300), dtype=np.uint8), np.zeros((160, 144), dtype=np.uint8)]
    yy, xx = np.mgrid[0:200, 0:300]
    masks[0][(yy - 100) ** 2 + (xx - 150) ** 2 <= 20 ** 2] = 255                                   # a tight outline
    masks[0][20, 20] = 255                                                                         # and a speck far from it
    masks[1][70:90, 60:70] = 200
    masks[1][70:90, 72:80] = 130                                                                   # two halves, a 2-pixel gap
    to = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return pics, masks, [to(p) for p in pics], [to(m) for m in masks]


def test_inpaint_window_with_mask_shape_is_inpaint_window_of_the_shaped_mask(dev, narrow, inp):
    from pbe_amd import pipeline
    from pbe_amd.window import shape_mask
    pics, masks, dp, dm = _silhouettes(dev)
    S = {"open": 1, "close": 1.5, "grow": 6, "box": True}
    kw = dict(steps=STEPS, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    out = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, mask_shape=S, **kw)
    shaped = [shape_mask(m, **S) for m in dm]
    hand = pipeline.inpaint_window(narrow, dp, shaped, inp["ref"], size=SIZE, feather=R, **kw)
    raw = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, mask_shape=None, **kw)
    again = pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, **kw)
    assert out["windows"] == hand["windows"] != raw["windows"]
    assert torch.equal(out["latent"], hand["latent"]) and torch.equal(out["image"], hand["image"]) and not torch.equal(out["latent"], raw["latent"])
    assert sorted(out) == sorted(list(hand) + ["masks"]) and sorted(raw) == sorted(again) == sorted(hand)
    for i in range(2):
        ref = mr.shape_mask_ref(masks[i], **S)
        assert np.array_equal(out["masks"][i].cpu().numpy(), ref) and torch.equal(out["masks"][i], shaped[i])
        assert torch.equal(out["pictures"][i], hand["pictures"][i]) and torch.equal(out["alphas"][i], hand["alphas"][i])
        assert torch.equal(out["inputs"]["mask"][i], hand["inputs"]["mask"][i])
        assert torch.equal(dm[i].cpu(), torch.from_numpy(masks[i])), "the caller's mask was changed"
        # None: the parent's keys and bits
        assert torch.equal(raw["pictures"][i], again["pictures"][i]) and torch.equal(raw["alphas"][i], again["alphas"][i])
    assert torch.equal(raw["latent"], again["latent"]) and torch.equal(raw["image"], again["image"]) and "masks" not in raw
    ya, yb, xa, xb = 74, 126, 124, 176                                                             # the disc's box grown by 6: the speck is gone
    assert int((out["masks"][0] == 255).sum()) == (yb - ya + 1) * (xb - xa + 1) and bool((out["masks"][0][ya:yb + 1, xa:xb + 1] == 255).all())
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError, match="unknown key"):
        pipeline.inpaint_window(narrow, dp, dm, inp["ref"], size=SIZE, feather=R, mask_shape={"dilate": 3}, **kw)


def test_inpaint_holes_with_mask_shape_closes_three_components_into_two_windows(dev, narrow, inp):
    from pbe_amd import ops, pipeline
    from pbe_amd.window import shape_mask
    pic = wr.random_picture((300, 400), 63)
    mask = np.zeros((300, 400), dtype=np.uint8)
    mask[30:50, 40:54] = 255
    mask[30:50, 56:70] = 200                                                                       # two halves of one object, a 2-pixel gap
    mask[220:250, 300:340] = 129                                                                   # another object far away
    dp, dm = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev)
    S = {"close": 1.5}
    kw = dict(steps=STEPS, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"])
    assert ops.component_boxes(ops.mask_components(dm))[0] == 3
    out = pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"][:1], size=SIZE, feather=0, mask_shape=S, **kw)
    shaped = shape_mask(dm, **S)
    assert ops.component_boxes(ops.mask_components(shaped))[0] == 2 and np.array_equal(shaped.cpu().numpy(), mr.shape_mask_ref(mask, **S))
    hand = pipeline.inpaint_holes(narrow, [dp], [shaped], inp["ref"][:1], size=SIZE, feather=0, **kw)
    assert len(out["holes"]) == 2 and [h["box"] for h in out["holes"]] == [(30, 49, 40, 69), (220, 249, 300, 339)]
    assert [h["area"] for h in out["holes"]] == [20 * 30, 30 * 40] and out["holes"] == hand["holes"]
    assert torch.equal(out["latent"], hand["latent"]) and torch.equal(out["image"], hand["image"]) and torch.equal(out["pictures"][0], hand["pictures"][0])
    assert all(torch.equal(a, b) for a, b in zip(out["alphas"], hand["alphas"])) and torch.equal(out["inputs"]["mask"], hand["inputs"]["mask"])
    assert len(out["masks"]) == 1 and torch.equal(out["masks"][0], shaped) and sorted(out) == sorted(list(hand) + ["masks"])
    assert torch.equal(dm.cpu(), torch.from_numpy(mask)) and not torch.equal(out["pictures"][0], dp)
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError, match="x_T has leading size 2, expected 3"):                       # unshaped at feather 0: three holes
        pipeline.inpaint_holes(narrow, [dp], [dm], inp["ref"][:1], size=SIZE, feather=0, mask_shape=None, **kw)


# ---- 6. the CLI ------------------------------------------------------------------------------------------------------------------------
def _cli_files(tmp_path, golden_dir):
    import yaml
    from PIL import Image
    pic = wr.random_picture((300, 400), 64)
    mask = np.zeros((300, 400), dtype=np.uint8)
    yy, xx = np.mgrid[0:300, 0:400]
    mask[(yy - 60) ** 2 + (xx - 80) ** 2 <= 14 ** 2] = 255                                         # two tight outlines, far apart
    mask[(yy - 230) ** 2 * 4 + (xx - 320) ** 2 <= 24 ** 2] = 180
    Image.fromarray(pic).save(str(tmp_path / "picture.png"))
    Image.fromarray(mask, mode="L").save(str(tmp_path / "mask.png"))
    cfg = str(tmp_path / "narrow.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)
    ref = os.path.join(golden_dir, "examples", "reference_example_1.jpg")
    base = ["--config", cfg, "--ddim_steps", str(STEPS), "--image_path", str(tmp_path / "picture.png"), "--mask_path", str(tmp_path / "mask.png"),
            "--reference_path", ref, "--seed", "321", "--scale", "5", "--fixed_code", "--random_weights", "--H", "128", "--W", "128", "--paste_back"]
    return pic, mask, ref, base


def _load_cli():
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_maskshape_gpu", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _ref_planes(path, dev):
    from PIL import Image
    from pbe_amd import ops, preprocess
    u8 = np.array(Image.open(path).convert("RGB").resize((224, 224)), dtype=np.uint8)
    return ops.u8_to_planes(torch.from_numpy(u8).to(dev)[None], preprocess.CLIP_MEAN, preprocess.CLIP_STD)


def _same_file(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        return fa.read() == fb.read()


def test_inference_cli_mask_flags_with_paste_back(dev, golden_dir, tmp_path):
    """--paste_back --mask_grow 6 --mask_box: pasted/*.png and source/*_mask.png are those of pipeline.inpaint_window(mask_shape=...) made
    by hand; and without the flags, those of mask_shape=None."""
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    cli = _load_cli()
    pic, mask, ref_path, base = _cli_files(tmp_path, golden_dir)
    S = {"grow": 6.0, "box": True}
    dp, dm, ref = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev), _ref_planes(ref_path, dev)
    with torch.no_grad():
        model = build.narrow_model(dev)
    for tag, flags, shape in (("shaped", ["--mask_grow", "6", "--mask_box"], S), ("plain", [], None)):
        out, dump = str(tmp_path / f"out_{tag}"), str(tmp_path / f"{tag}.npz")
        cli.main(base + flags + ["--outdir", out, "--dump_tensors", dump])
        t = np.load(dump)
        direct = pipeline.inpaint_window(model, [dp], [dm], ref, size=SIZE, context=0.5, feather=8, steps=STEPS, scale=5.0, sampler="ddim",
                                         x_T=torch.from_numpy(t["x_T"]).to(dev), post_eps=torch.from_numpy(t["post_eps"]).to(dev), mask_shape=shape)
        assert tuple(t["window"]) == direct["windows"][0] and torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
        pasted = np.asarray(Image.open(os.path.join(out, "pasted", "picture_321.png")))
        assert np.array_equal(pasted, direct["pictures"][0].cpu().numpy()) and (pasted != pic).any()
        hand = str(tmp_path / f"hand_{tag}")
        trip = {**{k: direct["inputs"][k] for k in ("image", "mask", "inpaint")}, "ref": ref}
        preprocess.save_outputs_device(hand, "picture", 321, trip, direct["image"][0], 128, 128)
        for n in ("picture_321_mask.png", "picture_321_inpaint.png", "picture_321_GT.png"):
            assert _same_file(os.path.join(out, "source", n), os.path.join(hand, "source", n)), (tag, n)
        assert ("masks" in direct) == (shape is not None)
    a = np.asarray(Image.open(str(tmp_path / "out_shaped" / "source" / "picture_321_mask.png")))
    b = np.asarray(Image.open(str(tmp_path / "out_plain" / "source" / "picture_321_mask.png")))
    assert (a != 255).sum() > (b != 255).sum() > 0                                                 # the shaped hole (not white in mask.png) is the larger one


def test_inference_cli_mask_flags_per_hole(dev, golden_dir, tmp_path):
    """--paste_back --per_hole --mask_grow 6 --mask_box: one set of files per boxed hole; pasted/*.png and source/*_mask.png are those of
    pipeline.inpaint_holes(mask_shape=...) made by hand."""
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    cli = _load_cli()
    pic, mask, ref_path, base = _cli_files(tmp_path, golden_dir)
    S = {"grow": 6.0, "box": True}
    out = str(tmp_path / "out")
    x = cli.main(base + ["--per_hole", "--mask_grow", "6", "--mask_box", "--outdir", out])
    assert tuple(x.shape) == (2, 3, 128, 128)
    dp, dm, ref = torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev), _ref_planes(ref_path, dev)
    shape = (2, 4, 16, 16)
    x_T = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(321))
    post_eps = torch.randn(shape, generator=torch.Generator().manual_seed(321)).to(dev)
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint_holes(model, [dp], [dm], ref, size=SIZE, context=0.5, feather=8, steps=STEPS, scale=5.0, sampler="ddim", x_T=x_T,
                                        post_eps=post_eps, mask_shape=S)
    assert torch.equal(direct["image"].cpu(), x) and np.array_equal(direct["masks"][0].cpu().numpy(), mr.shape_mask_ref(mask, **S))
    assert [h["box"] for h in direct["holes"]] == [(40, 80, 60, 100), (212, 248, 290, 350)]         # each outline's box, grown by 6
    pasted = np.asarray(Image.open(os.path.join(out, "pasted", "picture_321.png")))
    assert np.array_equal(pasted, direct["pictures"][0].cpu().numpy()) and (pasted != pic).any()
    for i in range(2):
        hand = str(tmp_path / f"hand{i}")
        trip = {**{k: direct["inputs"][k][i:i + 1] for k in ("image", "mask", "inpaint")}, "ref": ref}
        preprocess.save_outputs_device(hand, f"picture_hole{i}", 321, trip, direct["image"][i], 128, 128)
        for n in (f"picture_hole{i}_321_mask.png", f"picture_hole{i}_321_inpaint.png"):
            assert _same_file(os.path.join(out, "source", n), os.path.join(hand, "source", n)), n
        assert _same_file(os.path.join(out, "results", f"picture_hole{i}_321.png"), os.path.join(hand, "results", f"picture_hole{i}_321.png"))


def test_load_triple_device_and_the_plain_cli_shape_the_mask(dev, golden_dir, tmp_path):
    """The third path, without --paste_back: preprocess.load_triple_device(mask_shape=...) is u8_to_planes of the shaped mask, None is
    the parent's tensors, and the CLI's latent and source/*_mask.png are those of pipeline.inpaint on that triple."""
    import yaml
    from PIL import Image
    from pbe_amd import ops, pipeline, preprocess
    from pbe_amd.window import shape_mask
    cli = _load_cli()
    pic = wr.random_picture((128, 128), 65)
    mask = np.zeros((128, 128), dtype=np.uint8)
    yy, xx = np.mgrid[0:128, 0:128]
    mask[(yy - 50) ** 2 + (xx - 70) ** 2 <= 12 ** 2] = 255
    mask[100, 5] = 127
    paths = [str(tmp_path / n) for n in ("picture.png", "mask.png")] + [os.path.join(golden_dir, "examples", "reference_example_1.jpg")]
    Image.fromarray(pic).save(paths[0])
    Image.fromarray(mask, mode="L").save(paths[1])
    S = {"open": 0.0, "close": 0.0, "grow": 6.0, "box": True}                                      # what the CLI makes of --mask_grow 6 --mask_box
    trip = preprocess.load_triple_device(*paths, dev, mask_shape=S)
    shaped = shape_mask(torch.from_numpy(mask).to(dev), **S)
    assert np.array_equal(shaped.cpu().numpy(), mr.shape_mask_ref(mask, **S)) and int((shaped == 255).sum()) == 37 * 37
    assert torch.equal(trip["mask"], ops.u8_to_planes(shaped[None], mask_mode=1)) and torch.equal(trip["inpaint"], ops.mul_planes(trip["image"], trip["mask"]))
    plain, none = preprocess.load_triple_device(*paths, dev), preprocess.load_triple_device(*paths, dev, mask_shape=None)
    assert sorted(plain) == sorted(none) == sorted(trip) and all(torch.equal(plain[k], none[k]) for k in plain)
    assert torch.equal(trip["image"], plain["image"]) and torch.equal(trip["ref"], plain["ref"]) and not torch.equal(trip["mask"], plain["mask"])
    cfg = str(tmp_path / "narrow.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)
    with torch.no_grad():
        model = build.narrow_model(dev)
    for tag, flags, t in (("shaped", ["--mask_grow", "6", "--mask_box"], trip), ("plain", [], plain)):
        out, dump = str(tmp_path / f"out_{tag}"), str(tmp_path / f"{tag}.npz")
        cli.main(flags + ["--config", cfg, "--ddim_steps", str(STEPS), "--image_path", paths[0], "--mask_path", paths[1], "--reference_path", paths[2],
                          "--seed", "321", "--scale", "5", "--fixed_code", "--random_weights", "--H", "128", "--W", "128", "--outdir", out, "--dump_tensors", dump])
        d = np.load(dump)
        hand = pipeline.inpaint(model, t["image"], t["mask"], t["ref"], steps=STEPS, scale=5.0, sampler="ddim", x_T=torch.from_numpy(d["x_T"]).to(dev),
                                post_eps=torch.from_numpy(d["post_eps"]).to(dev))
        assert torch.equal(hand["latent"].float().cpu(), torch.from_numpy(d["latent"])), tag
        by_hand = str(tmp_path / f"hand_{tag}")
        preprocess.save_outputs_device(by_hand, "picture", 321, t, hand["image"][0], 128, 128)
        for sub, n in (("source", "picture_321_mask.png"), ("source", "picture_321_inpaint.png"), ("results", "picture_321.png")):
            assert _same_file(os.path.join(out, sub, n), os.path.join(by_hand, sub, n)), (tag, n)
        assert not os.path.exists(os.path.join(out, "pasted"))
