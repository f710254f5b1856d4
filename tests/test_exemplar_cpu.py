"""The exemplar cut on the device, host side: tests/pilref.py (Pillow's 8-bit resize restated in numpy) against Pillow itself, byte for
byte; pbe_amd.exemplar.resample_tables against the restatement's tables; plan_crop's stated properties, exhaustively over small pictures;
the numpy twin of ops.mask_box against window.hole_box.  Every comparison is equality."""
import importlib.util
import itertools
import math
import os
import platform
from fractions import Fraction

import numpy as np
import pytest

import pilref as P


def _where():
    import PIL
    return f"Pillow {PIL.__version__} on {platform.machine()} / {platform.system()}"


@pytest.mark.parametrize("name", P.SOURCES)
def test_restatement_equals_pillow(name):
    a = P.source(name)
    for box, out_hw, filt in P.cases(name):
        got, want = P.resize(a, out_hw, box, filt), P.pillow(a, out_hw, box, filt)
        assert got.shape == want.shape and np.array_equal(got, want), \
            f"{name} box {box} -> {out_hw} {filt}: {int((got != want).sum())} bytes differ from {_where()}"


def test_default_filter_is_bicubic_and_skip_rules():
    from PIL import Image
    a = P.source("random_300x224")
    assert np.array_equal(np.array(Image.fromarray(a).resize((224, 224))), P.resize(a, (224, 224), None, "bicubic"))
    sq = P.source("random_224x224")
    for filt in P.FILTERS:                                         # both passes skipped: a copy, whatever the filter
        assert np.array_equal(P.resize(sq, (224, 224), None, filt), sq)
    assert not P.needs(224, 224, 0, 224) and P.needs(224, 224, 0.25, 224) and P.needs(224, 224, 0, 223) and P.needs(225, 224, 0, 225)
    # 300x224 whole: only the vertical pass; 225x1000 whole -> 224 wide: both; 225 high kept: only the horizontal one
    wide = P.source("random_225x1000")
    for filt in P.FILTERS:
        assert np.array_equal(P.resize(wide, (225, 224), None, filt), P.pillow(wide, (225, 224), None, filt))
        assert np.array_equal(P.resize(a, (224, 224), None, filt), P.pillow(a, (224, 224), None, filt))


def test_tall_pictures_take_the_height_first():
    """Image.resize's own rule: more than 100 times as tall as wide and the height shrinks -> the vertical pass runs first."""
    from pbe_amd.exemplar import vertical_first
    assert P.tall_first(1001, 10, 17) and not P.tall_first(1000, 10, 17) and not P.tall_first(1001, 10, 1001) and not P.tall_first(10, 1001, 5)
    for args in ((1001, 10, 17), (1000, 10, 17), (1001, 10, 1001), (1001, 10, 1002), (10, 1001, 5), (16384, 3, 224)):
        assert vertical_first(*args) == P.tall_first(*args)
    for hw in ((1001, 10), (1000, 10), (16384, 3)):
        a = P.random_picture(hw, 21)
        H, W = hw
        for box, out_hw, filt in ((None, (17, 9), "bicubic"), ((0.5, 2, W - 1, H - 0.5), (224, 224), "lanczos"), (None, (H + 1, 9), "bilinear"), (None, (17, W), "bicubic")):
            got, want = P.resize(a, out_hw, box, filt), P.pillow(a, out_hw, box, filt)
            assert np.array_equal(got, want), f"{hw} box {box} -> {out_hw} {filt}: {int((got != want).sum())} bytes differ from {_where()}"


def test_mask_fill_composition_equals_pillow_on_the_composed_picture():
    a = P.source("random_37x53")
    m = P.random_mask(a.shape[:2], 7)
    assert (m >= 128).any() and (m < 128).any() and (m == 128).any() and (m == 127).any()
    fill = (255, 0, 17)
    comp = P.compose(a, m, fill)
    assert np.array_equal(comp[m >= 128], a[m >= 128]) and (comp[m < 128] == np.array(fill, dtype=np.uint8)).all()
    for box, out_hw, filt in P.cases("random_37x53"):
        assert np.array_equal(P.resize(a, out_hw, box, filt, mask=m, fill=fill), P.pillow(comp, out_hw, box, filt))


@pytest.mark.parametrize("filt", P.FILTERS)
def test_resample_tables_equal_the_restatement(filt):
    from pbe_amd.exemplar import identity_tables, resample_tables
    axes = [(5, 0, 5, 9), (7, 0, 7, 224), (53, 1, 52, 224), (53, 0.25, 52.25, 9), (224, 0, 224, 17), (1000, 0, 1000, 224), (1200, 0, 1200, 9),
            (1200, 300, 900, 224), (1277, 0.5, 1275.5, 17), (1920, 0, 1920, 224), (481, 120, 361, 9), (1, 0, 1, 3), (3, 0, 3, 1), (16384, 0, 16384, 9)]
    for in_size, in0, in1, out in axes:
        b, k = resample_tables(in_size, in0, in1, out, filt)
        rb, rk = P.tables(in_size, in0, in1, out, filt)
        assert b.dtype == np.int32 and k.dtype == np.int32 and b.shape == (out, 2) and k.shape == rk.shape, (in_size, in0, in1, out)
        assert np.array_equal(b, rb) and np.array_equal(k, rk), (in_size, in0, in1, out)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= in_size).all() and (b[:, 1] <= k.shape[1]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()          # what the horizontal pass's staging walks
        for i in range(out):
            assert not k[i, b[i, 1]:].any()
    assert P.tables(1200, 0, 1200, 9, "bicubic")[1].shape[1] == 535
    ib, ik = identity_tables(4)
    assert np.array_equal(ib, [[0, 1], [1, 1], [2, 1], [3, 1]]) and np.array_equal(ik, [[1 << 22]] * 4)
    src = P.source("random_7x5")
    assert np.array_equal(P.apply_pass(src, *identity_tables(5)), src)


def test_resample_tables_and_boxes_refuse_bad_arguments():
    from pbe_amd.exemplar import resample_tables, validate_box
    from pbe_amd.lib import PbeError
    for args in ((5, 0, 5, 9, "nearest"), (5, -1, 5, 9, "bicubic"), (5, 0, 6, 9, "bicubic"), (5, 3, 3, 9, "bicubic"), (5, 0, 5, 0, "bicubic")):
        with pytest.raises(PbeError):
            resample_tables(*args)
    assert validate_box(None, (7, 5)) == (0.0, 0.0, 5.0, 7.0) and validate_box((0.25, 1, 5, 6.5), (7, 5)) == (0.25, 1.0, 5.0, 6.5)
    for box in ((-1, 0, 5, 7), (0, 0, 6, 7), (0, 0, 5, 7.5), (2, 0, 2, 7), (3, 0, 2, 7), (0, 0, 5), (0, 0, float("nan"), 7), "abcd"):
        with pytest.raises(PbeError):
            validate_box(box, (7, 5))


def _boxes(Hs, Ws):
    for ya, yb in itertools.combinations_with_replacement(range(Hs), 2):
        for xa, xb in itertools.combinations_with_replacement(range(Ws), 2):
            yield ya, yb, xa, xb


def test_plan_crop_properties_exhaustively():
    from pbe_amd.exemplar import plan_crop
    n = 0
    for (Hs, Ws), pad, square in itertools.product(((1, 1), (5, 7), (7, 5), (6, 6), (3, 9)), (0.0, 0.25, 0.5, 1.0, 3.0), (False, True)):
        fr = Fraction(pad).limit_denominator(1 << 20)
        for ya, yb, xa, xb in _boxes(Hs, Ws):
            n += 1
            x0, y0, x1, y1 = plan_crop((ya, yb, xa, xb), (Hs, Ws), pad, square)
            what = f"box {(ya, yb, xa, xb)} in {Hs} x {Ws}, pad {pad}, square {square} -> {(x0, y0, x1, y1)}"
            assert all(isinstance(v, int) for v in (x0, y0, x1, y1)), what
            assert 0 <= x0 < x1 <= Ws and 0 <= y0 < y1 <= Hs, what                              # inside the picture, not empty
            py, px = math.ceil(fr * (yb - ya + 1)), math.ceil(fr * (xb - xa + 1))
            gy0, gy1, gx0, gx1 = ya - py, yb + 1 + py, xa - px, xb + 1 + px                      # the grown box, exclusive ends
            assert y0 <= max(gy0, 0) and y1 >= min(gy1, Hs) and x0 <= max(gx0, 0) and x1 >= min(gx1, Ws), what     # holds it where the picture does
            eh, ew = gy1 - gy0, gx1 - gx0
            if square:
                side = max(eh, ew)
                assert y1 - y0 == min(side, Hs) and x1 - x0 == min(side, Ws), what              # shifted, not shrunk; clipped only by the picture
                if side <= min(Hs, Ws):
                    assert y1 - y0 == x1 - x0, what
                if gy0 - (side - eh) // 2 >= 0 and gy1 + (side - eh + 1) // 2 <= Hs and gx0 - (side - ew) // 2 >= 0 and gx1 + (side - ew + 1) // 2 <= Ws:
                    assert abs((y0 + y1) - (gy0 + gy1)) <= 1 and abs((x0 + x1) - (gx0 + gx1)) <= 1, what       # twice the centres: half a pixel
            else:
                assert y1 - y0 == min(eh, Hs) and x1 - x0 == min(ew, Ws), what
                if gy0 >= 0 and gy1 <= Hs and gx0 >= 0 and gx1 <= Ws:
                    assert (x0, y0, x1, y1) == (gx0, gy0, gx1, gy1), what
    assert n > 5000


def test_plan_crop_examples_and_errors():
    from pbe_amd.exemplar import plan_crop
    from pbe_amd.lib import PbeError
    assert plan_crop((10, 19, 30, 49), (100, 200)) == (30, 10, 50, 20)
    assert plan_crop((10, 19, 30, 49), (100, 200), pad=0.1) == (28, 9, 52, 21)
    assert plan_crop((10, 19, 30, 49), (100, 200), square=True) == (30, 5, 50, 25)
    assert plan_crop((0, 9, 30, 49), (100, 200), square=True) == (30, 0, 50, 20)              # shifted at the border, not shrunk
    assert plan_crop((0, 99, 0, 9), (100, 50), square=True) == (0, 0, 50, 100)                # the picture is narrower than the object is tall
    for bad in ((5, 4, 0, 1), (0, 100, 0, 1), (-1, 4, 0, 1), (0, 1, 0, 200), (0.5, 1, 0, 1), (0, 1, 0)):
        with pytest.raises(PbeError):
            plan_crop(bad, (100, 200))
    with pytest.raises(PbeError):
        plan_crop((0, 1, 0, 1), (100, 200), pad=-0.1)
    with pytest.raises(PbeError):
        plan_crop((0, 1, 0, 1), (100, 200), pad=float("nan"))


def test_mask_box_twin_agrees_with_hole_box():
    from pbe_amd.lib import PbeError
    from pbe_amd.window import hole_box
    rng = np.random.default_rng(3)
    for hw in ((1, 1), (17, 300), (33, 5), (64, 64), (100, 257)):
        for _ in range(6):
            m = rng.integers(0, 128, size=hw, dtype=np.uint8)
            for _ in range(int(rng.integers(1, 4))):
                m[rng.integers(0, hw[0]), rng.integers(0, hw[1])] = rng.choice([128, 200, 255])
            assert P.mask_box(m) == hole_box(m)
        empty = np.full(hw, 127, dtype=np.uint8)
        assert P.mask_box(empty) is None
        with pytest.raises(PbeError):
            hole_box(empty)


def test_cli_reference_flag_counts_are_argparse_errors():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_exemplar_cpu", os.path.join(root, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--image_path", "i.png", "--mask_path", "m.png", "--reference_path", "a.jpg", "b.jpg"]
    for bad in (["--reference_box", "0", "0", "10", "10"], ["--reference_box", "0", "0", "10", "10", "0", "0", "10"], ["--reference_mask", "m.png"],
                ["--reference_mask", "a.png", "b.png", "c.png"], ["--reference_fill", "1", "2", "3"], ["--reference_pad", "0.5"], ["--reference_square"]):
        with pytest.raises(SystemExit) as e:
            cli.parse(base + bad)
        assert e.value.code == 2, bad                                   # p.error
    opt = cli.parse(base + ["--reference_box", "0", "0", "10", "10", "1", "1", "9", "9.5", "--reference_pad", "0.25"])
    assert cli.reference_on_device(opt) and opt.reference_box[4:] == [1.0, 1.0, 9.0, 9.5]
    assert cli.reference_on_device(cli.parse(base + ["--reference_on_device"])) and not cli.reference_on_device(cli.parse(base))
