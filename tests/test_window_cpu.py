"""Windowed inpainting, the part that needs no GPU: the window planner (pbe_amd/window.py), the numpy restatements of the four kernels
on themselves (tests/windowref.py: what tests/test_window_gpu.py holds the device to), the gates against the mistakes they exist to
catch, and the wrappers' refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch

import windowref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the planner --------------------------------------------------------------------------------------------------------------------
def _check_plan(mask, working, context, r, what):
    from pbe_amd.window import hole_box, plan_window
    Hs, Ws = mask.shape
    H, W = working
    y0, x0, wh, ww = win = plan_window(mask, working, context, r)
    assert all(type(v) is int for v in win), (what, win)
    assert 0 <= y0 and 0 <= x0 and wh >= 1 and ww >= 1 and y0 + wh <= Hs and x0 + ww <= Ws, (what, win)                 # in the picture
    ya, yb, xa, xb = hole_box(mask)
    assert y0 <= ya and yb < y0 + wh and x0 <= xa and xb < x0 + ww, (what, win, (ya, yb, xa, xb))                      # holds the box
    m = 2 * r + 1
    for margin, at_border in ((ya - y0, y0 == 0), (y0 + wh - 1 - yb, y0 + wh == Hs), (xa - x0, x0 == 0), (x0 + ww - 1 - xb, x0 + ww == Ws)):
        assert at_border or margin >= m, (what, win, (ya, yb, xa, xb), m)
    assert wh >= min(H, Hs) and ww >= min(W, Ws), (what, win)                                                           # never magnified when avoidable
    if wh < Hs and ww < Ws:                                                                                             # unclamped: the aspect H : W, rounded up
        assert abs(wh * W - ww * H) < max(H, W), (what, win)
    return win


def _mask_with_box(Hs, Ws, ya, yb, xa, xb):
    m = np.zeros((Hs, Ws), dtype=np.uint8)
    m[ya, xa] = m[yb, xb] = 255          # two corners of the box are enough for the planner
    m[ya, xb] = 128
    return m


def test_planner_properties_random_sweep():
    rs = np.random.RandomState(11)
    n = 0
    for _ in range(300):
        H, W = [(32, 48), (64, 64), (128, 96), (512, 512)][rs.randint(4)]
        kind = rs.randint(4)
        Hs = rs.randint(H, 5 * H) if kind != 1 else rs.randint(max(H // 3, 2), H)        # kind 1 / 2: smaller than the working size in one dimension
        Ws = rs.randint(W, 5 * W) if kind != 2 else rs.randint(max(W // 3, 2), W)
        bh, bw = rs.randint(1, Hs + 1), rs.randint(1, Ws + 1)
        if rs.rand() < 0.5:
            bh, bw = min(bh, max(Hs // 8, 1)), min(bw, max(Ws // 8, 1))
        ya, xa = rs.randint(0, Hs - bh + 1), rs.randint(0, Ws - bw + 1)
        context, r = [0.0, 0.25, 0.5, 1.0, 0.3][rs.randint(5)], int(rs.choice([0, 1, 3, 8, 16, 40]))
        _check_plan(_mask_with_box(Hs, Ws, ya, ya + bh - 1, xa, xa + bw - 1), (H, W), context, r, f"draw {n}")
        n += 1
    assert n == 300


@pytest.mark.parametrize("where", ["top", "bottom", "left", "right", "top_left", "top_right", "bottom_left", "bottom_right"])
def test_planner_hole_at_a_border_or_corner(where):
    Hs, Ws, bh, bw = 300, 400, 30, 50
    ya = 0 if "top" in where else Hs - bh if "bottom" in where else 120
    xa = 0 if "left" in where else Ws - bw if "right" in where else 170
    for working, r in (((64, 64), 8), ((128, 96), 0), ((32, 48), 40)):
        y0, x0, wh, ww = _check_plan(_mask_with_box(Hs, Ws, ya, ya + bh - 1, xa, xa + bw - 1), working, 0.5, r, where)
        assert (y0 == 0) == ("top" in where or wh == Hs) and (x0 == 0) == ("left" in where or ww == Ws), (where, (y0, x0, wh, ww))
        assert ("bottom" not in where or y0 + wh == Hs) and ("right" not in where or x0 + ww == Ws)


def test_planner_exact_values_and_special_cases():
    from pbe_amd.lib import PbeError
    from pbe_amd.window import plan_window, validate_window
    # box 10 x 40, r = 8 (m = 17): need_h = 10 + 2 max(17, 5) = 44, need_w = 40 + 2 max(17, 20) = 80; 44 * 48 < 80 * 32, so the width decides
    m = _mask_with_box(200, 300, 100, 109, 150, 189)
    assert plan_window(m, (32, 48), 0.5, 8) == ((100 + 109 + 1 - 54) // 2, (150 + 189 + 1 - 80) // 2, 54, 80)      # 80 * 32 / 48 = 53.3 -> 54 rows
    assert plan_window(m, (64, 64), 0.5, 8) == ((210 - 80) // 2, (340 - 80) // 2, 80, 80)
    assert plan_window(m, (128, 128), 0.5, 8) == ((210 - 128) // 2, (340 - 128) // 2, 128, 128)                     # never below the working size
    # a picture of exactly the working size: the whole picture, whatever the hole
    assert plan_window(_mask_with_box(64, 96, 3, 5, 90, 95), (64, 96), 0.5, 8) == (0, 0, 64, 96)
    # too small in one dimension: an anisotropic window (whole height, working width)
    assert plan_window(_mask_with_box(40, 500, 10, 12, 200, 210), (64, 64), 0.5, 2) == (0, (411 - 64) // 2, 40, 64)
    with pytest.raises(PbeError, match="no hole"):
        plan_window(np.full((50, 60), 127, dtype=np.uint8), (32, 32))
    with pytest.raises(PbeError):
        plan_window(np.zeros((50, 60), dtype=np.float32), (32, 32))
    with pytest.raises(PbeError):
        plan_window(m, (32, 48), 0.5, -1)
    # a caller's window: validated, returned as ints; the mask may then be empty
    assert plan_window(np.zeros((50, 60), dtype=np.uint8), (32, 32), window=(np.int64(1), 2, 30, 40)) == (1, 2, 30, 40)
    for bad in ((-1, 0, 10, 10), (0, 0, 51, 10), (0, 21, 10, 40), (0, 0, 0, 10), (0.5, 0, 10, 10), (0, 0, 10), "abcd", None):
        with pytest.raises(PbeError):
            validate_window(bad, (50, 60))


# ---- 2. the restatements on themselves -------------------------------------------------------------------------------------------------
def test_identity_window_is_load_triple_bit_for_bit(golden_dir):
    from pbe_amd import preprocess
    d = os.path.join(golden_dir, "examples")
    paths = (os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png"), os.path.join(d, "reference_example_1.jpg"))
    trip = preprocess.load_triple(*paths)
    u8 = preprocess.load_triple_u8(*paths)
    assert u8["image"].shape == (512, 512, 3)
    ys = slice(100, 228)                                  # rows 100 .. 227 of the triple as a picture of its own keep the test quick
    pic, mask = np.ascontiguousarray(u8["image"][ys]), np.ascontiguousarray(u8["mask"][ys])
    win = (0, 0, 128, 512)
    assert np.array_equal(wr.image32(pic, win, (128, 512)), trip["image"][0, :, ys].numpy())
    assert np.array_equal(wr.mask_ref(mask, win, (128, 512)), trip["mask"][0, :, ys].numpy())
    assert 0 < wr.mask_ref(mask, win, (128, 512)).mean() < 1
    # a grey-level mask: the byte threshold 128 is the (1 - v / 255) < 0.5 of load_triple for all 256 values
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    v = 1 - ramp.astype(np.float32) / 255.0
    assert np.array_equal(wr.mask_ref(ramp, (0, 0, 16, 16), (16, 16))[0], np.where(v < 0.5, 0, 1).astype(np.float32))


@pytest.mark.parametrize("hw,size", [((64, 96), (32, 48)), ((106, 159), (32, 48)), ((20, 30), (32, 48)), ((100, 40), (32, 48)), ((53, 77), (32, 48)),
                                     ((400, 400), (10, 10)), ((32, 48), (32, 48)), ((33, 47), (97, 131))])
def test_filter_restatements_against_torch(hw, size):
    """filter64 and resample32 against F.interpolate(antialias=True) on the CPU within the 2e-6 of test_resize_bilinear_against_torch -
    against torch's fp64 result for every shape (filter64 to 1e-12: the same filter), and against its fp32 result except at
    33 x 47 -> 97 x 131, where ATen's own fp32 centre (rounding 2 u c, c up to 47, at support 1) is 2.2e-6 away from its fp64 result."""
    import torch.nn.functional as Fn
    x = torch.rand(3, *hw, generator=torch.Generator().manual_seed(hw[0] * 1000 + size[0]))
    ref32 = Fn.interpolate(x[None], size=size, mode="bilinear", align_corners=False, antialias=True)[0].numpy()
    ref64 = Fn.interpolate(x[None].double(), size=size, mode="bilinear", align_corners=False, antialias=True)[0].numpy()
    f64, ny, nx = wr.filter64(x.numpy(), size)
    f32 = wr.resample32(x.numpy(), size).astype(np.float64)
    assert np.abs(f64 - ref64).max() <= 1e-12 and np.abs(f32 - ref64).max() <= 2e-6
    if hw != (33, 47):
        assert np.abs(f64 - ref32).max() <= 2e-6 and np.abs(f32 - ref32).max() <= 2e-6
    for n_in, n_out in zip(hw, size):
        assert np.abs(wr.aa_matrix(n_in, n_out)[0] - wr.aa_matrix_float(n_in, n_out)).max() <= 1e-14          # the integer form is ATen's filter
    assert ny.max() <= 2 * max(hw[0] / size[0], 1) + 2 and nx.min() >= 1
    if hw == size:
        assert np.array_equal(wr.resample32(x.numpy(), size), x.numpy())          # scale 1: centre weight 1, neighbour 0


@pytest.mark.parametrize("case", wr.IMAGE_CASES, ids=[c[0] for c in wr.IMAGE_CASES])
def test_fp32_emulation_passes_the_image_bound(case):
    """The kernel's arithmetic on the CPU must pass the bound the GPU test applies - else the bound, not the device, is wrong."""
    name, shape, win, size = case
    pic = wr.random_picture(shape, 5)
    for mean, std in (((0.5,) * 3, (0.5,) * 3), ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))):
        worst = wr.gate_image(wr.image32(pic, win, size, mean, std), pic, win, size, mean, std, name)
        assert worst > 0 or name == "identity"
    if name == "scale40":                                   # 80 taps a side: pbe_resize_bilinear_f32 refuses the scale (2 * 40 + 2 > its 64)
        assert wr.image64(pic, win, size)[2].max() == 80


def test_alpha_facts():
    """alpha is exactly 1 on every hole pixel (also at the picture's corners), positive exactly within Chebyshev distance 2r of the
    hole, 0 beyond; r = 0 is the hole itself; with the planner's margin it is 0 on every window border inside the picture."""
    from pbe_amd.window import plan_window
    for seed, shape in ((1, (90, 130)), (2, (61, 47))):
        mask = wr.random_mask(shape, seed)
        mask[0, 0] = mask[-1, -1] = mask[0, -1] = mask[-1, 0] = 255                 # holes in the four corners
        whole = (0, 0, *shape)
        for r in (0, 1, 3, 16, 40):
            a = wr.alpha_ref(mask, whole, r)
            hole = mask >= 128
            assert a.dtype == np.float32 and np.all(a[hole] == 1.0) and a.max() <= 1.0 and a.min() >= 0.0
            assert np.array_equal(a > 0, wr.chebyshev_within(mask, 2 * r))
            if r == 0:
                assert np.array_equal(a, hole.astype(np.float32))
    rs = np.random.RandomState(3)
    for _ in range(40):
        Hs, Ws = rs.randint(150, 400), rs.randint(150, 400)
        mask = np.zeros((Hs, Ws), dtype=np.uint8)
        y, x = rs.randint(0, Hs - 20), rs.randint(0, Ws - 20)
        mask[y:y + rs.randint(1, 20), x:x + rs.randint(1, 20)] = 255
        r = int(rs.choice([0, 2, 8, 13]))
        y0, x0, wh, ww = win = plan_window(mask, (64, 96), float(rs.choice([0.0, 0.5])), r)
        a = wr.alpha_ref(mask, win, r)
        for edge, at_border in ((a[0], y0 == 0), (a[-1], y0 + wh == Hs), (a[:, 0], x0 == 0), (a[:, -1], x0 + ww == Ws)):
            assert at_border or not edge.any(), (win, r)


@pytest.mark.parametrize("scale", [0.3, 0.77, 1.0, 1.5, 2.0, 3.3125, 7.9, 40.0])
def test_footprint_rule_covers_every_hole_pixel(scale):
    rs = np.random.RandomState(int(scale * 100))
    H, W = 24, 36
    wh, ww = max(int(round(H * scale)), 1), max(int(round(W * scale * 1.07)), 1)
    mask = np.zeros((wh + 9, ww + 5), dtype=np.uint8)
    for _ in range(6):
        mask[rs.randint(0, wh + 9), rs.randint(0, ww + 5)] = 128                    # single pixels
    mask[rs.randint(0, wh + 9), ::3] = 255                                           # a dotted one-pixel line
    win = (4, 2, wh, ww)
    keep = wr.mask_ref(mask, win, (H, W))[0]
    hole = wr.crop(mask, win) >= 128
    ys, xs = np.nonzero(hole)
    # the working pixels whose footprint (Y wh) // H .. ceil((Y + 1) wh / H) - 1 holds window row y: all Y with Y wh // H <= y < ceil((Y + 1) wh / H)
    covered = np.zeros_like(hole)
    for Y in range(H):
        for X in range(W):
            if keep[Y, X] == 0:
                covered[(Y * wh) // H:-((-(Y + 1) * wh) // H), (X * ww) // W:-((-(X + 1) * ww) // W)] = True
            else:
                assert not hole[(Y * wh) // H:-((-(Y + 1) * wh) // H), (X * ww) // W:-((-(X + 1) * ww) // W)].any()
    assert hole.any() and covered[ys, xs].all()
    assert set(np.unique(keep)) <= {0.0, 1.0}


# ---- 3. the gates reject what they must ------------------------------------------------------------------------------------------------
def test_gates_reject_wrong_windows_and_wrong_alpha():
    pic = wr.random_picture((120, 170), 9)
    win, size = (7, 5, 106, 159), (32, 48)
    wr.gate_image(wr.image32(pic, win, size), pic, win, size)
    with pytest.raises(AssertionError, match="bound"):
        wr.gate_image(wr.image32(pic, (8, 5, 106, 159), size), pic, win, size)                       # shifted by one pixel
    with pytest.raises(AssertionError, match="bound"):
        wr.gate_image(wr.image32(pic, (7, 6, 106, 159), size), pic, win, size)
    sq, wsq = wr.random_picture((100, 100), 10), (10, 20, 64, 64)
    with pytest.raises(AssertionError, match="bound"):
        wr.gate_image(wr.image32(sq, (20, 10, 64, 64), (32, 32)), sq, wsq, (32, 32))                 # y and x exchanged
    mask = wr.random_mask((120, 170), 4)
    mask[0, 0] = 255
    assert not np.array_equal(wr.mask_ref(mask, (8, 5, 106, 159), size), wr.mask_ref(mask, win, size))
    assert not np.array_equal(wr.mask_ref(mask.T.copy(), (5, 7, 106, 106), (32, 32)), wr.mask_ref(mask, (7, 5, 106, 106), (32, 32)))
    for r in (1, 3, 16):
        good = wr.alpha_ref(mask, (0, 0, 100, 150), r)
        assert not np.array_equal(wr.alpha_ref(mask, (0, 0, 100, 150), r, dilate=False), good)       # alpha from the undilated mask
        assert not np.array_equal(wr.alpha_ref(mask, (0, 0, 100, 150), r, pad="constant"), good)     # zero padding in place of replicate
        assert not np.array_equal(wr.alpha_ref(mask, (1, 0, 100, 150), r), good)


@pytest.mark.parametrize("case", wr.PASTE_CASES, ids=[c[0] for c in wr.PASTE_CASES])
def test_paste_emulation_passes_and_the_gate_rejects_wrong_pastes(case):
    name, shape, win, size = case
    pic, result, alpha = wr.paste_inputs(shape, win, size, 21)
    good = wr.paste32(pic, result, alpha, win)
    changed, near, live = wr.gate_paste(good, pic, result, alpha, win, name)
    assert live > 0 and changed <= near
    with pytest.raises(AssertionError, match="differ from the fp64 reference"):
        wr.gate_paste(wr.paste32(pic, result, alpha, win, rounding=np.trunc), pic, result, alpha, win)           # truncation in place of rint
    with pytest.raises(AssertionError, match="outside"):
        bad = wr.paste32(pic, result, np.maximum(alpha, np.float32(0.25)), win, written=np.ones(alpha.shape, dtype=bool))
        wr.gate_paste(bad, pic, result, alpha, win)                                                               # writes where alpha == 0
    with pytest.raises(AssertionError):
        y0, x0, wh, ww = win
        wr.gate_paste(wr.paste32(pic, result, alpha, (y0 + 1, x0, wh, ww)), pic, result, alpha, win)             # pasted one pixel off
    if name == "identity":                                  # alpha == 1 at scale 1: the bytes are rint(255 result) exactly
        one = np.ones_like(alpha)
        got = wr.paste32(pic, result, one, win)
        assert np.array_equal(wr.crop(got, win), np.rint(np.float32(255) * result).astype(np.uint8).transpose(1, 2, 0))


def test_paste_formula_returns_the_byte_at_alpha_zero():
    b = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.rint(np.float32(255) * (b / np.float32(255))), b)


# ---- 4. no CPU fallback ----------------------------------------------------------------------------------------------------------------
def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from pbe_amd import ops, pipeline
    from pbe_amd.lib import PbeError
    pic, mask = torch.zeros(20, 30, 3, dtype=torch.uint8), torch.zeros(20, 30, dtype=torch.uint8)
    with pytest.raises(PbeError, match="GPU"):
        ops.window_image(pic, (0, 0, 10, 10), (8, 8))
    with pytest.raises(PbeError, match="GPU"):
        ops.window_mask(mask, (0, 0, 10, 10), (8, 8))
    with pytest.raises(PbeError, match="GPU"):
        ops.feather_alpha(mask, (0, 0, 10, 10), 2)
    with pytest.raises(PbeError, match="GPU"):
        ops.paste_window(torch.zeros(3, 8, 8), torch.zeros(10, 10), pic, (0, 0, 10, 10))
    with pytest.raises(PbeError):
        pipeline.inpaint_window(None, [pic], [mask, mask], None)
    with pytest.raises(PbeError):
        pipeline.inpaint_window(None, [], [], None)
