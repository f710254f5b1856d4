"""The shape of a mask, host side (-m "not gpu"): the two numpy restatements of tests/maskref.py against each other, the algebra that makes
the border rule the right one, the strength of the GPU case lists (every wrong map of maskref.DIST2_FAULTS / GROW_FAULTS differs from the
reference on a case they hold), the host logic of pbe_amd.window.shape_mask, pipeline.inpaint_window / inpaint_holes and the CLI with the
HIP ops replaced - in these tests only - by maskref, and the declared symbols.  No kernel is launched."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import holesref as hr
import maskref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pbe_mask_dist2_workspace_bytes", "pbe_mask_dist2_u8_i32", "pbe_mask_from_dist2_u8", "pbe_fill_boxes_u8")
CPU_SHAPES = [(1, 300), (300, 1), (90, 130), (33, 65)]
ALGEBRA_R = (1, 1.5, 2, 5)


@pytest.fixture(autouse=True, scope="module")
def _the_entry_points_exist():
    """The reference and the case lists below exist for the kernels, so nothing here passes without the entry points.  The tests of
    sections 1 and 2 say something about tests/maskref.py and the case lists only, nothing about the kernels: those are judged by
    tests/test_maskshape_gpu.py."""
    from pbe_amd import lib
    missing = [n for n in NEW_SYMBOLS if n not in lib.SYMBOLS]
    assert not missing, f"pbe_amd.lib.SYMBOLS lacks {missing}"


def _cli():
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_maskshape", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
def test_the_definition_equals_the_separable_reference(shape):
    for pattern in hr.PATTERNS:
        mask = hr.case_mask(pattern, shape)
        for to_hole in (True, False):
            s = mr.the_set(mask, to_hole)
            full = mr.dist2_brute_full(s)
            for rmax in (0, 1, 3, 16):
                want = np.minimum(full, rmax * rmax + 1)
                got = mr.dist2_ref(s, rmax)
                assert np.array_equal(got, want), (pattern, shape, to_hole, rmax)
                assert got.max() <= rmax * rmax + 1 and (got == 0).sum() == s.sum()
                if not s.any():
                    assert (got == rmax * rmax + 1).all()                                          # an empty set: saturated everywhere
    s = mr.the_set(hr.case_mask("diagonal", shape), True)
    assert np.array_equal(mr.dist2_brute(s, 3), np.minimum(mr.dist2_brute_full(s), 10))


def test_single_pixel_discs_have_the_sizes_of_the_euclidean_disc():
    one = np.zeros((41, 41), dtype=np.uint8)
    one[20, 20] = 200
    for r, n in ((1, 5), (1.5, 9), (2, 13), (3, 29), (0, 1)):
        assert int((mr.grow_ref(one, r) == 255).sum()) == n, r
    cross = mr.grow_ref(one, 1)
    assert cross[19, 20] == cross[21, 20] == cross[20, 19] == cross[20, 21] == 255 and cross[19, 19] == 0
    assert (mr.grow_ref(one, 1.5)[19:22, 19:22] == 255).all()
    assert not mr.grow_ref(one, -1).any()                                                          # a single pixel does not survive shrinking
    corner = np.zeros((9, 9), dtype=np.uint8)
    corner[:4, :4] = 255                                                                           # the picture's border does not erode:
    assert np.array_equal(mr.grow_ref(corner, -1) == 255, np.pad(np.ones((3, 3), bool), ((0, 6), (0, 6))))
    assert (mr.grow_ref(np.full((5, 7), 255, np.uint8), -3) == 255).all()                          # and a picture that is all hole stays so


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
def test_the_algebra_that_makes_the_border_rule_right(shape):
    """With the outside of the picture in neither set, closing only adds, opening only removes, both are idempotent and growing the hole
    is shrinking the rest.  (With the outside counted as background, closing a hole at the border would cut it back.)"""
    for pattern in hr.PATTERNS:
        mask = hr.case_mask(pattern, shape)
        hole = mask >= 128
        inverse = np.where(hole, 0, 255).astype(np.uint8)
        for r in ALGEBRA_R:
            what = (pattern, shape, r)
            closed, opened = mr.close_ref(mask, r), mr.open_ref(mask, r)
            assert set(np.unique(closed)) <= {0, 255} and set(np.unique(opened)) <= {0, 255}
            assert ((closed == 255) | ~hole).all(), what                                           # close contains the mask
            assert ((opened == 0) | hole).all(), what                                              # open is contained in it
            assert np.array_equal(mr.close_ref(closed, r), closed), what
            assert np.array_equal(mr.open_ref(opened, r), opened), what
            assert np.array_equal(mr.grow_ref(mask, r), 255 - mr.grow_ref(inverse, -r)), what
            assert np.array_equal(mr.grow_ref(mask, -r), 255 - mr.grow_ref(inverse, r)), what


# ---- 2. the case lists catch every planted fault -------------------------------------------------------------------------------------------
# the case each wrong map is named to differ on: (pattern, shape, rmax, to_hole)
NAMED_DIST2 = {
    "the square (Chebyshev) element": ("last_corner", (90, 130), 2, True),                         # the diagonal neighbour: 2, not 1
    "city-block distance": ("last_corner", (90, 130), 2, True),                                    # the diagonal neighbour: 2, not 4
    "the outside of the picture counted as hole": ("no_hole", (90, 130), 7, True),
    "the outside of the picture counted as background": ("all_hole", (90, 130), 7, False),
    "a cap of rmax^2": ("last_corner", (90, 130), 7, True),                                        # far pixels: 50, not 49
    "a column pass swept down only": ("last_corner", (90, 130), 7, True),                          # the pixels above the corner
    "a column pass swept up only": ("diagonal", (90, 130), 7, True),                               # the pixels below the diagonal
    "a row pass that stops one tap early": ("last_corner", (90, 130), 7, True),                    # the pixel 7 columns to the left: 49
    "the threshold applied at 127": ("threshold", (90, 130), 1, True),
    "the threshold applied at 129": ("threshold", (90, 130), 1, True),
}
# the same for grow: (pattern, shape, r)
NAMED_GROW = {
    "`<` in place of `<=`": ("threshold4", (90, 130), 2),
    "the square (Chebyshev) element": ("last_corner", (90, 130), 2),                               # the diagonal neighbour of the corner joins
    "city-block distance": ("last_corner", (90, 130), 3),                                          # (2, 2) from the corner: 8 <= 9, but |dy| + |dx| = 4
    "the outside of the picture counted as hole": ("no_hole", (90, 130), 7),                       # a frame of 7 pixels appears
    "the outside of the picture counted as background": ("all_hole", (90, 130), -7),               # a frame of 7 pixels goes
    "a cap of rmax^2": ("last_corner", (90, 130), 7),                                              # 49 <= 49: every far pixel joins
    "a column pass swept down only": ("last_corner", (90, 130), 7),                                # nothing above the corner's row joins
    "a column pass swept up only": ("blobs", (90, 130), 7),                                        # nothing below a disc joins
    "a row pass that stops one tap early": ("last_corner", (90, 130), 7),                          # the pixel 7 columns to the left
    "the threshold applied at 127": ("threshold4", (90, 130), 1),
    "the threshold applied at 129": ("threshold4", (90, 130), 1),
}


@pytest.mark.parametrize("fault", list(mr.DIST2_FAULTS), ids=lambda s: s.replace(" ", "_"))
def test_every_wrong_distance_map_is_caught_by_the_case_list(fault):
    pattern, shape, rmax, to_hole = NAMED_DIST2[fault]
    assert (pattern, shape, rmax) in mr.DIST2_CASES
    got = mr.DIST2_FAULTS[fault](mr.case_mask(pattern, shape), to_hole, rmax)
    ref = mr.case_dist2(pattern, shape, to_hole, rmax)
    assert got.shape == ref.shape and not np.array_equal(got, ref), f"{fault}: equal to the reference on {NAMED_DIST2[fault]}"
    print(f"{fault}: {int((got != ref).sum())} of {ref.size} values differ on {NAMED_DIST2[fault]}")


@pytest.mark.parametrize("fault", list(mr.GROW_FAULTS), ids=lambda s: s.replace(" ", "_"))
def test_every_wrong_grow_is_caught_by_the_case_list(fault):
    pattern, shape, r = NAMED_GROW[fault]
    assert (pattern, shape, r) in mr.GROW_CASES
    mask = mr.case_mask(pattern, shape)
    got, ref = mr.GROW_FAULTS[fault](mask, r), mr.grow_ref(mask, r)
    assert not np.array_equal(got, ref), f"{fault}: equal to the reference on {(pattern, shape, r)}"
    print(f"{fault}: {int((got != ref).sum())} of {ref.size} bytes differ on {(pattern, shape, r)}")


def test_the_case_lists_hold_what_the_issue_names():
    assert mr.SHAPES == [(1, 300), (300, 1), (90, 130), (129, 257), (67, 1031)] and mr.RMAX == (0, 1, 2, 7, 33)
    assert all((p, (90, 130), 300) in mr.DIST2_CASES and (p, (1, 300), 300) in mr.DIST2_CASES for p in hr.PATTERNS)
    assert len(mr.DIST2_CASES) == len(hr.PATTERNS) * (5 * 5 + 2)
    assert mr.GROW_R == (0, 1, 1.5, 2, 3, 7, 16.5, -1, -2.5, -7)
    for s in mr.GROW_SHAPES:
        assert set(np.unique(mr.case_mask("threshold4", s))) == {127, 128, 129, 255}
    far = mr.case_dist2("last_corner", (90, 130), True, 7)                                         # true distances beyond rmax: saturated at 50
    assert far.max() == 50 and far[0, 0] == 50 and far[89, 122] == 49 and far[89, 121] == 50 and far[82, 129] == 49
    assert (mr.case_dist2("no_hole", (90, 130), True, 33) == 33 * 33 + 1).all()
    blobs = mr.case_mask("blobs", (129, 257))
    count = lambda m: hr.boxes_ref(hr.label_ref(m, 8)).shape[0]                                    # noqa: E731
    assert count(mr.open_ref(blobs, 1.5)) < count(blobs) and count(mr.close_ref(blobs, 2)) < count(blobs)


def test_fill_boxes_and_shape_mask_reference():
    boxes = [(0, 0, 0, 0), (3, 5, 2, 8), (4, 9, 7, 7)]
    out = mr.fill_boxes_ref(boxes, (10, 9))
    assert out.sum() == 255 * (1 + 3 * 7 + 6 - 2) and out[0, 0] == 255 and out[9, 7] == 255 and out[9, 8] == 0
    assert not mr.fill_boxes_ref(np.zeros((0, 4)), (4, 4)).any()
    m = np.zeros((40, 60), dtype=np.uint8)
    m[10, 10:20] = 200
    m[11:20, 10] = 129                                                                             # an L: its box is 10 x 10
    m[30, 50] = 255                                                                                # a speck
    assert np.array_equal(mr.shape_mask_ref(m), np.where(m >= 128, 255, 0))
    boxed = mr.shape_mask_ref(m, box=True)
    assert (boxed[10:20, 10:20] == 255).all() and boxed[30, 50] == 255 and int((boxed == 255).sum()) == 101
    assert int((mr.shape_mask_ref(m, open=1, box=True) == 255).sum()) == 0                         # open removes the one-pixel-wide L too
    assert np.array_equal(mr.shape_mask_ref(m, open=1, close=2, grow=3, box=True),
                          mr.fill_boxes_ref(hr.boxes_ref(hr.label_ref(mr.grow_ref(mr.close_ref(mr.open_ref(m, 1), 2), 3), 8))[:, 1:5], m.shape))


# ---- 3. host logic, the HIP ops replaced by maskref ------------------------------------------------------------------------------------
class FakeOps:
    """ops.mask_* / fill_boxes / the holes and window ops on CPU tensors, through maskref and holesref; `calls` is the order of calls and
    `seen` every mask a consumer was handed."""

    def __init__(self, monkeypatch):
        from pbe_amd import ops
        self.calls, self.seen = [], []
        for name in ("mask_grow", "mask_close", "mask_open", "fill_boxes", "mask_components", "component_boxes", "select_components", "window_image",
                     "window_mask", "feather_alpha", "paste_window", "mul_planes"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    @staticmethod
    def _t(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def mask_grow(self, mask, r, out=None):
        self.calls.append(("grow", float(r)))
        return self._t(mr.grow_ref(mask.numpy(), r))

    def mask_close(self, mask, r, out=None):
        self.calls.append(("close", float(r)))
        return self._t(mr.close_ref(mask.numpy(), r))

    def mask_open(self, mask, r, out=None):
        self.calls.append(("open", float(r)))
        return self._t(mr.open_ref(mask.numpy(), r))

    def fill_boxes(self, boxes, shape, out=None, device=None):
        self.calls.append(("box", len(boxes)))
        return self._t(mr.fill_boxes_ref(np.asarray(boxes), tuple(shape)))

    def mask_components(self, mask, connectivity=8, out=None):
        self.calls.append(("label", connectivity))
        self.seen.append(("mask_components", mask.clone()))
        return self._t(hr.label_ref(mask.numpy(), connectivity))

    def component_boxes(self, labels, capacity=4096):
        t = hr.boxes_ref(labels.numpy())
        return t.shape[0], t

    def select_components(self, labels, wanted, out=None):
        return self._t(hr.select_ref(labels.numpy(), wanted))

    def window_image(self, picture, window, size, mean=None, std=None, out=None):
        return out.zero_()

    def window_mask(self, mask, window, size, out=None):
        self.seen.append(("window_mask", mask.clone()))
        return out.fill_(1.0)

    def feather_alpha(self, mask, window, feather, out=None):
        self.seen.append(("feather_alpha", mask.clone()))
        return torch.zeros(window[2], window[3])

    def paste_window(self, result, alpha, picture, window):
        return picture

    def mul_planes(self, x, m):
        return x * m


def _speckled():
    """Two halves of one object 2 pixels apart, a second object, and a speck far from both."""
    m = np.zeros((120, 160), dtype=np.uint8)
    m[20:50, 20:40] = 255
    m[20:50, 42:60] = 200                                      # the gap: columns 40, 41
    m[80:100, 100:130] = 129
    m[5, 150] = 255                                            # the speck
    return m


def test_shape_mask_runs_its_stages_in_order_and_skips_defaults(monkeypatch):
    from pbe_amd.lib import PbeError
    from pbe_amd.window import shape_mask
    fake = FakeOps(monkeypatch)
    m = _speckled()
    t = torch.from_numpy(m.copy())
    for kw, order in (({}, ["grow"]), ({"grow": 2}, ["grow"]), ({"close": 1.5}, ["close"]), ({"open": 1}, ["open"]), ({"box": True}, ["label", "box"]),
                      ({"grow": -1.5, "open": 1, "box": True, "close": 2}, ["open", "close", "grow", "label", "box"]),
                      ({"box": True, "connectivity": 4, "grow": 3}, ["grow", "label", "box"])):
        fake.calls.clear()
        got = shape_mask(t, **kw)
        assert [c[0] for c in fake.calls] == order, (kw, fake.calls)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), mr.shape_mask_ref(m, **kw)), kw
        assert np.array_equal(t.numpy(), m), "shape_mask changed its input"
        if "connectivity" in kw:
            assert ("label", 4) in fake.calls
    fake.calls.clear()
    shape_mask(t)
    assert fake.calls == [("grow", 0.0)]                                                           # all defaults: the mask binarised
    fake.calls.clear()
    shape_mask(t, grow=-1.5, open=1, close=2)
    assert fake.calls == [("open", 1.0), ("close", 2.0), ("grow", -1.5)]
    none = shape_mask(t, open=40)                                                                  # nothing survives: not an error here
    assert not none.numpy().any()
    for bad, word in (({"open": -1}, "open"), ({"close": -0.5}, "close"), ({"grow": 2048}, "grow"), ({"grow": float("nan")}, "grow"), ({"grow": "3"}, "grow"),
                      ({"box": 1}, "box"), ({"connectivity": 6}, "connectivity"), ({"open": True}, "open")):
        fake.calls.clear()
        with pytest.raises(PbeError, match=word):
            shape_mask(t, **bad)
        assert fake.calls == [], f"{bad}: something ran before the refusal"
    with pytest.raises(TypeError):
        shape_mask(t, dilate=3)
    from pbe_amd.window import shape_args
    with pytest.raises(PbeError, match=r"unknown key.*dilate"):
        shape_args({"dilate": 3})
    assert shape_args({}) == {"open": 0, "close": 0, "grow": 0, "box": False, "connectivity": 8}


def test_inpaint_window_hands_the_shaped_mask_to_every_consumer(monkeypatch):
    from pbe_amd import pipeline
    from pbe_amd.lib import PbeError
    from pbe_amd.window import plan_window
    fake = FakeOps(monkeypatch)
    monkeypatch.setattr(pipeline, "inpaint", lambda model, image, mask, ref, **kw: {"image": torch.zeros(image.shape[0], 3, 32, 32)})
    m = _speckled()
    pic, t = torch.zeros((120, 160, 3), dtype=torch.uint8), torch.from_numpy(m.copy())
    S = {"open": 1, "close": 1.5, "grow": 4, "box": True}
    want = mr.shape_mask_ref(m, **S)
    out = pipeline.inpaint_window(None, [pic], [t], None, size=(32, 32), feather=2, mask_shape=S)
    assert [k for k, _ in fake.seen if k != "mask_components"] == ["window_mask", "feather_alpha"]
    for who, seen in fake.seen:
        if who != "mask_components":
            assert np.array_equal(seen.numpy(), want), f"{who} did not get the shaped mask"
    assert out["windows"] == [plan_window(want, (32, 32), 0.5, 2)]
    m2 = np.zeros((120, 160), dtype=np.uint8)
    m2[40:50, 40:50], m2[110, 150] = 255, 255                                                      # without its speck the hole's window is the smallest one
    small = pipeline.inpaint_window(None, [pic], [torch.from_numpy(m2)], None, size=(32, 32), feather=2, mask_shape={"open": 1})
    assert small["windows"] == [plan_window(mr.open_ref(m2, 1), (32, 32), 0.5, 2)] == [(29, 29, 32, 32)] != [plan_window(m2, (32, 32), 0.5, 2)]
    assert len(out["masks"]) == 1 and np.array_equal(out["masks"][0].numpy(), want) and np.array_equal(t.numpy(), m)
    fake.seen.clear(), fake.calls.clear()
    plain = pipeline.inpaint_window(None, [pic], [t], None, size=(32, 32), feather=2)
    assert "masks" not in plain and fake.calls == [] and all(np.array_equal(s.numpy(), m) for _, s in fake.seen)
    assert sorted(plain) == sorted(k for k in out if k != "masks")
    with pytest.raises(PbeError, match="unknown key"):
        pipeline.inpaint_window(None, [pic], [t], None, size=(32, 32), feather=2, mask_shape={"dilate": 2})
    with pytest.raises(PbeError, match="close"):
        pipeline.inpaint_window(None, [pic], [t], None, size=(32, 32), feather=2, mask_shape={"close": -1})


def test_inpaint_holes_labels_the_shaped_mask(monkeypatch):
    from pbe_amd import pipeline
    fake = FakeOps(monkeypatch)
    monkeypatch.setattr(pipeline, "inpaint", lambda model, image, mask, ref, **kw: {"image": torch.zeros(image.shape[0], 3, 32, 32)})
    m = _speckled()
    pic, t, ref = torch.zeros((120, 160, 3), dtype=torch.uint8), torch.from_numpy(m.copy()), torch.zeros(1, 3, 4, 4)
    raw = pipeline.inpaint_holes(None, [pic], [t], ref, size=(32, 32), feather=0)
    assert len(raw["holes"]) == 4 and "masks" not in raw and fake.calls == [("label", 8)]           # two halves, the object, the speck
    fake.seen.clear(), fake.calls.clear()
    S = {"open": 1, "close": 1.5}
    want = mr.shape_mask_ref(m, **S)
    out = pipeline.inpaint_holes(None, [pic], [t], ref, size=(32, 32), feather=0, mask_shape=S)
    assert [c[0] for c in fake.calls] == ["open", "close", "label"]
    assert len(out["holes"]) == 2 and [h["box"] for h in out["holes"]] == [(20, 49, 20, 59), (80, 99, 100, 129)]
    labelled = [s for k, s in fake.seen if k == "mask_components"]
    assert len(labelled) == 1 and np.array_equal(labelled[0].numpy(), want)
    own = [hr.select_ref(hr.label_ref(want, 8), h["labels"]) for h in out["holes"]]
    for who in ("window_mask", "feather_alpha"):
        got = [s.numpy() for k, s in fake.seen if k == who]
        assert len(got) == 2 and all(np.array_equal(g, o) for g, o in zip(got, own)), who
    assert np.array_equal(out["masks"][0].numpy(), want) and np.array_equal(t.numpy(), m)
    assert sorted(raw) == sorted(k for k in out if k != "masks")


def test_cli_mask_flags_and_their_refusals():
    cli = _cli()
    plain = cli.parse(["--paste_back"])
    assert (plain.mask_grow, plain.mask_close, plain.mask_open, plain.mask_box) == (0.0, 0.0, 0.0, False) and cli.mask_shape_of(plain) is None
    opt = cli.parse(["--mask_grow", "-2.5", "--mask_box"])
    assert cli.mask_shape_of(opt) == {"open": 0.0, "close": 0.0, "grow": -2.5, "box": True}
    opt = cli.parse(["--paste_back", "--per_hole", "--mask_close", "3", "--mask_open", "1.5", "--mask_grow", "6"])
    assert cli.mask_shape_of(opt) == {"open": 1.5, "close": 3.0, "grow": 6.0, "box": False}
    assert cli.mask_shape_of(cli.parse(["--mask_box"])) == {"open": 0.0, "close": 0.0, "grow": 0.0, "box": True}
    from pbe_amd.window import shape_args
    assert shape_args(cli.mask_shape_of(opt))["connectivity"] == 8
    for argv in (["--mask_close", "-1"], ["--mask_open", "-0.5"], ["--mask_grow", "2048"], ["--mask_grow", "-2047.5"], ["--mask_grow", "nan"],
                 ["--mask_close", "inf"], ["--mask_open", "3000"], ["--mask_grow", "wide"], ["--mask_box", "1"]):
        with pytest.raises(SystemExit):
            cli.parse(argv)


# ---- 4. declarations and refusals that need no device ------------------------------------------------------------------------------------
def test_new_symbols_are_declared_in_the_header_and_in_lib():
    from pbe_amd import lib
    header = open(os.path.join(ROOT, "include", "pbe_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pbe_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in lib.SYMBOLS, name
    assert "maskshape.hip" in lib.SOURCES and os.path.exists(os.path.join(ROOT, "pbe_amd", "csrc", "maskshape.hip"))
    assert os.path.join("csrc", "maskshape.hip") in lib.HASHED and lib.ABI_VERSION == 8
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}(" in integration for n in NEW_SYMBOLS)
    from pbe_amd.build import build
    build()
    handle = lib.load()
    assert handle.pbe_mask_dist2_workspace_bytes(100, 30) == 2 * 100 * 30 and handle.pbe_mask_dist2_workspace_bytes(16384, 16384) == 2 << 28
    assert handle.pbe_mask_dist2_workspace_bytes(0, 5) == 0 and handle.pbe_mask_dist2_workspace_bytes(5, 16385) == 0
    # refusals that happen before any device is touched
    assert handle.pbe_mask_dist2_u8_i32(None, None, 4, 4, 1, 1, None, 0, None) != 0
    assert handle.pbe_mask_from_dist2_u8(None, None, 4, 4, 1, 0, None) != 0
    assert handle.pbe_fill_boxes_u8(None, 1, None, 4, 4, None) != 0
    assert b"pbe_fill_boxes_u8" in handle.pbe_last_error()


def test_the_wrappers_refuse_cpu_tensors_and_bad_arguments_before_any_launch():
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    m = torch.zeros((8, 8), dtype=torch.uint8)
    for call in (lambda: ops.mask_dist2(m), lambda: ops.mask_grow(m, 2), lambda: ops.mask_close(m, 2), lambda: ops.mask_open(m, 2),
                 lambda: ops.fill_boxes([[0, 1, 0, 1]], (8, 8), out=m)):
        with pytest.raises(PbeError, match="GPU"):
            call()
    with pytest.raises(PbeError, match="GPU"):
        ops.fill_boxes([[0, 1, 0, 1]], (8, 8), device="cpu")
    for boxes, shape, word in (([[0, 8, 0, 1]], (8, 8), "box 0"), ([[0, 1, 0, 1], [3, 2, 0, 1]], (8, 8), "box 1"), ([[0, 1, -1, 1]], (8, 8), "box 0"),
                               ([[0, 1, 0, 1.5]], (8, 8), "integers"), ([[0, 1, 0]], (8, 8), r"\[n, 4\]"), ([[0, 0, 0, 0]] * 4097, (8, 8), "4097"),
                               ([[0, 1, 0, 1]], (8, 16385), "16384"), ([[0, 1, 0, 1]], (8,), "shape")):
        with pytest.raises(PbeError, match=word):
            ops.fill_boxes(boxes, shape)
    from pbe_amd.ops_picture import _radius
    for r in (2047.5, -2048, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(PbeError, match="real number in -2047 .. 2047"):
            _radius("r", r, True)
    with pytest.raises(PbeError, match="real number in 0 .. 2047"):
        _radius("r", -1, False)
    assert _radius("r", 1.5, True) * 2 == 3 and _radius("r", np.float32(-2.5), True) * 2 == -5 and _radius("r", np.int64(7), False) == 7
