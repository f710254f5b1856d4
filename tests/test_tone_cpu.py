"""Tone matching of a pasted window, the part that needs no GPU: the restatements of tests/toneref.py on themselves, the host-side fit
(pbe_amd.window.fit_tone) against its restatement and its own properties, the recovery of a planted tone through the emulated
kernels, the strength of the case list tests/test_tone_gpu.py runs, the paste gate against the mistakes it exists to catch, and the
wrappers' refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import maskref as mr
import toneref as tr
import windowref as wr

F = np.float32


# ---- 1. the statistics' restatement ----------------------------------------------------------------------------------------------------
def test_stats_ref_against_a_plain_loop():
    rs = np.random.RandomState(3)
    image = rs.uniform(-1.4, 1.4, (2, 3, 4, 5)).astype(F)
    result = rs.uniform(-0.2, 1.2, (2, 3, 4, 5)).astype(F)
    sel = tr.SEL_VALUES[rs.randint(0, tr.SEL_VALUES.size, size=(2, 1, 4, 5))]
    image[0, 1, 2, 3], result[1, 0, 0, 0], result[0, 2, 3, 4] = np.nan, np.inf, F(100.5 / 255.0)
    sel[0, 0, 2, 3] = sel[1, 0, 0, 0] = sel[0, 0, 3, 4] = 1.0
    t = tr.stats_ref(image, result, sel)
    assert t.dtype == np.int64 and t.shape == (2, 3, 6) and np.array_equal(t, tr.stats_loop(image, result, sel))
    assert np.all(t[:, 0, 0] == t[:, 1, 0]) and np.all(t[:, 0, 0] == t[:, 2, 0]) and 0 < t[0, 0, 0] < 20
    assert np.array_equal(tr.stats_ref(image, result, np.zeros_like(sel)), np.zeros((2, 3, 6), dtype=np.int64))


def test_quantiser_facts():
    b = np.arange(256)
    x = ((b.astype(F) / F(255)) - F(0.5)) / F(0.5)                       # what window_image makes of a byte at mean = std = 0.5
    assert np.array_equal(tr.quant_image(x), b), "the image quantiser does not return the byte"
    assert np.array_equal(tr.quant_result(b.astype(F) / F(255)), b)
    odd = np.array([np.nan, np.inf, -np.inf, -0.3, 1.7, -0.0, 1.0], dtype=F)
    assert tr.quant_result(odd).tolist() == [0, 255, 0, 0, 255, 0, 255]
    assert tr.quant_image(F(2) * odd - F(1)).tolist() == [0, 255, 0, 0, 255, 0, 255]
    # exact ties: wherever 255 * r is k + 0.5 exactly in fp32, the byte is the even neighbour; everywhere it is the nearest integer of the fp32 product
    k = np.arange(255)
    r = ((k + 0.5) / 255.0).astype(F)
    p = F(255) * r
    tie = p == (k + 0.5).astype(F)
    assert tie.sum() > 50, "no exact tie among the planted values"
    assert np.array_equal(tr.quant_result(r)[tie], (k + (k % 2))[tie])
    assert np.array_equal(tr.quant_result(r), np.rint(p.astype(np.float64)).astype(np.int64))
    # 0.5 * x is exact, so the contracted form fma(0.5, x, 0.5) rounds the same sum once: the same bits
    xs = np.random.RandomState(1).uniform(-1.5, 1.5, 20000).astype(F)
    assert np.array_equal(F(0.5) * xs + F(0.5), wr.fma32(F(0.5), xs, F(0.5)))


# ---- 2. the fit ------------------------------------------------------------------------------------------------------------------------
def _same_fit(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x == y, (x, y)


def test_fit_tone_equals_the_fraction_restatement():
    from pbe_amd.window import fit_tone
    rs = np.random.RandomState(5)
    for i in range(40):
        g, b = rs.uniform(0.7, 1.4), rs.uniform(-0.08, 0.08)
        table = tr.random_table(rs, int(rs.randint(1, 4)), int(rs.choice([1, 10, 63, 64, 65, 500, 4000])), g, b, noise=float(rs.choice([0.0, 3.0, 20.0])))
        for mode in ("affine", "mean"):
            limit, least = float(rs.choice([1.0, 1.1, 1.25, 2.0])), int(rs.choice([0, 64, 100]))
            _same_fit(fit_tone(table, mode, limit, least), tr.fit_ref(table, mode, limit, least))
    table = tr.random_table(rs, 2, 300, 0.9, 0.03)
    want = fit_tone(table)
    _same_fit(fit_tone(torch.from_numpy(table)), want)                   # a host tensor, an array, a nested list: one result
    _same_fit(fit_tone(table.tolist()), want)
    for f in want:
        assert all(type(v) is float and float(F(v)) == v for v in f["gain"] + f["offset"]), "gain and offset are not fp32 values"
        assert type(f["n"]) is int and type(f["identity"]) is bool


def test_fit_tone_properties():
    from pbe_amd.window import fit_tone
    rs = np.random.RandomState(6)
    o = rs.randint(0, 256, size=(2, 3, 500)).astype(np.int64)
    all_on = np.ones((2, 500), dtype=bool)
    for f in fit_tone(tr._sums(o, o, all_on)):                           # q = o: the identity, exactly
        assert f["identity"] and f["gain"] == [1.0] * 3 and f["offset"] == [0.0] * 3 and f["rms_before"] == [0.0] * 3 and f["rms_after"] == [0.0] * 3
        assert f["clamped"] == [False] * 3 and f["n"] == 500
    for g, b in ((0.9, 0.04), (1.1, -0.03), (1.0, 0.05), (1.2, 0.0)):
        table = tr.random_table(rs, 2, 2000, g, b, noise=2.0, o_range=(40, 190))         # no byte of q is clipped; little noise: little attenuation of the slope
        for f in fit_tone(table, "mean"):
            assert f["gain"] == [1.0] * 3 and f["clamped"] == [False] * 3 and not f["identity"]
            assert all(a <= c for a, c in zip(f["rms_after"], f["rms_before"]))
        for f in fit_tone(table, "affine"):
            assert f["clamped"] == [False] * 3 and all(abs(x - g) < 0.02 for x in f["gain"]) and all(abs(x - b) < 0.02 for x in f["offset"])
            assert all(a <= c for a, c in zip(f["rms_after"], f["rms_before"])) and all(a < 8.0 for a in f["rms_after"])
    for g, end in ((1.6, 1.25), (0.6, 0.8)):                             # clamping at both ends is flagged, and the value is the limit's
        for f in fit_tone(tr.random_table(rs, 1, 2000, g, 0.0, noise=1.0, o_range=(0, 150))):
            assert f["clamped"] == [True] * 3 and f["gain"] == [float(F(end))] * 3
    small = tr.random_table(rs, 1, 63, 0.9, 0.04)
    assert fit_tone(small)[0]["identity"] and fit_tone(small)[0]["gain"] == [1.0] * 3 and fit_tone(small)[0]["offset"] == [0.0] * 3
    assert not fit_tone(small, min_pixels=63)[0]["identity"] and not fit_tone(tr.random_table(rs, 1, 64, 0.9, 0.04))[0]["identity"]
    assert fit_tone(np.zeros((1, 3, 6), dtype=np.int64), min_pixels=0)[0]["identity"]                # no pixel at all
    q = np.full((1, 3, 400), 77, dtype=np.int64)                         # a flat result: zero variance gives gain 1, the offset still fits
    f = fit_tone(tr._sums(rs.randint(100, 120, size=(1, 3, 400)).astype(np.int64), q, np.ones((1, 400), dtype=bool)))[0]
    assert f["gain"] == [1.0] * 3 and f["clamped"] == [False] * 3 and all(0.08 < b < 0.17 for b in f["offset"])


def test_fit_tone_refusals():
    from pbe_amd.lib import PbeError
    from pbe_amd.window import fit_tone
    table = tr.random_table(np.random.RandomState(7), 2, 100)
    for kw in (dict(mode="median"), dict(mode=None), dict(gain_limit=0.99), dict(gain_limit=float("nan")), dict(gain_limit=float("inf")), dict(min_pixels=-1)):
        with pytest.raises(PbeError):
            fit_tone(table, **kw)
    for bad in (table[:, :2], table[:, :, :5], table[0], table.astype(np.float64), 5):
        with pytest.raises(PbeError):
            fit_tone(bad)
    uneven = table.copy()
    uneven[1, 2, 0] += 1
    with pytest.raises(PbeError, match="different"):
        fit_tone(uneven)


# ---- 3. a planted tone is recovered ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g0,b0", tr.RECOVERY)
def test_a_planted_tone_is_recovered(g0, b0):
    """The result is the original with a tone of its own, hole included; the fit sees the known pixels only, a margin away from the hole.
    Pasted through the fitted map the picture comes back (emulated here: the largest byte difference was 0); the plain paste is off by 13
    to 16 grey levels."""
    from pbe_amd.window import fit_tone
    pic, mask, result = tr.recovery_case(g0, b0)
    win, r = tr.RECOVERY_WINDOW, tr.RECOVERY_FEATHER
    size = win[2:]
    image = wr.image32(pic, win, size)
    sel = wr.mask_ref(mr.grow_ref(mask, tr.RECOVERY_MARGIN), win, size)
    hole = wr.mask_ref(mask, win, size) == 0
    assert hole.any() and not sel[hole].any() and 1000 < sel.sum() < sel.size - hole.sum()
    stats = tr.stats_ref(image[None], result[None], sel[None])
    fit = fit_tone(stats)[0]
    assert not fit["identity"] and fit["clamped"] == [False] * 3 and all(a < 0.6 for a in fit["rms_after"]) and all(b > 4.0 for b in fit["rms_before"])
    alpha = wr.alpha_ref(mask, win, r)
    plain = wr.paste32(pic, result, alpha, win)
    fixed = tr.paste_tone32(pic, result, alpha, win, fit["gain"], fit["offset"])
    off_plain, off_fixed = np.abs(plain.astype(int) - pic).max(), np.abs(fixed.astype(int) - pic).max()
    print(f"planted ({g0}, {b0}): fitted gain {fit['gain']}, offset {fit['offset']}; largest byte difference {off_fixed} with the map, {off_plain} without")
    assert off_fixed <= 1 and off_plain >= 10


# ---- 4. the GPU case list tells every wrong variant from the table ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def stats_cases():
    return [(shape, mode, tr.stats_inputs(shape, mode)) for shape, mode in tr.STATS_CASES]


@pytest.mark.parametrize("fault", list(tr.STATS_FAULTS), ids=[k.replace(" ", "_") for k in tr.STATS_FAULTS])
def test_the_gpu_cases_catch_the_fault(stats_cases, fault):
    hit = [(shape, mode) for shape, mode, (image, result, sel) in stats_cases
           if not np.array_equal(tr.stats_ref(image, result, sel, **tr.STATS_FAULTS[fault]), tr.stats_ref(image, result, sel))]
    assert hit, f"no GPU case tells '{fault}' from the right table"


def test_the_gpu_cases_hold_what_they_claim(stats_cases):
    for shape, mode, (image, result, sel) in stats_cases:
        t = tr.stats_ref(image, result, sel)
        B, H, W = shape
        assert t.shape == (B, 3, 6) and (t >= 0).all()
        if mode == "zeros":
            assert not t.any()
        if mode == "ones":
            assert np.all(t[:, :, 0] == H * W)
        if mode == "mixed" and H * W > 1000:
            assert all(np.any(sel == v) if v == v else np.isnan(sel).any() for v in tr.SEL_VALUES) and np.signbit(sel[sel == 0]).any()
            for a in (image, result):
                assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
            assert (image > 1).any() and (image < -1).any() and (result > 1).any() and (result < 0).any()
    assert tr.stats_ref(*tr.stats_inputs((1, 300, 300), "ones"))[0, :, 3:].max() > 2 ** 32


# ---- 5. the paste gate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.PASTE_CASES, ids=[c[0] for c in wr.PASTE_CASES])
def test_tone_paste_emulation_passes_and_the_gate_rejects_wrong_pastes(case):
    name, shape, win, size = case
    pic, result, alpha = wr.paste_inputs(shape, win, size, 21)
    for gain, offset in tr.TONES + [((1.25,) * 3, (-0.1,) * 3)]:
        good = tr.paste_tone32(pic, result, alpha, win, gain, offset)
        changed, near, live = tr.gate_paste_tone(good, pic, result, alpha, win, gain, offset, name)
        print(f"{name} gain {gain}: {near} of {live} reference values at a tie ({100.0 * near / live:.3f} %), {changed} bytes differ")
        assert live > 0 and changed <= near, (name, gain, changed, near, live)
        for fault, msg in (("after_blend", "differ from the fp64 reference"), ("no_offset", "differ from the fp64 reference"), ("writes_everywhere", "outside")):
            with pytest.raises(AssertionError, match=msg):
                tr.gate_paste_tone(tr.paste_tone32(pic, result, alpha, win, gain, offset, fault=fault), pic, result, alpha, win, gain, offset)
        with pytest.raises(AssertionError, match="differ from the fp64 reference"):
            tr.gate_paste_tone(wr.paste32(pic, result, alpha, win), pic, result, alpha, win, gain, offset)            # the map not applied at all
    # tone (1, 0) is the plain paste, bit for bit: fmaf(1, r, 0) = r
    assert np.array_equal(tr.paste_tone32(pic, result, alpha, win, (1.0,) * 3, (0.0,) * 3), wr.paste32(pic, result, alpha, win))
    with pytest.raises(AssertionError, match="tolerance is derived"):
        tr.gate_paste_tone(pic, pic, result, alpha, win, (3.0,) * 3, (0.0,) * 3)


# ---- 6. no CPU fallback ----------------------------------------------------------------------------------------------------------------
def test_tone_ops_refuse_cpu_tensors_and_bad_arguments():
    from pbe_amd import ops, ops_picture, pipeline
    from pbe_amd.lib import PbeError
    from pbe_amd.window import tone_selection
    image, result, sel = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8)
    with pytest.raises(PbeError, match="GPU"):
        ops.tone_stats(image, result, sel)
    pic = torch.zeros(20, 30, 3, dtype=torch.uint8)
    with pytest.raises(PbeError, match="GPU"):
        ops.paste_window(torch.zeros(3, 8, 8), torch.zeros(10, 10), pic, (0, 0, 10, 10), tone=((1, 1, 1), (0, 0, 0)))
    for bad in ((1.0, 0.0), ((1, 1), (0, 0, 0)), ((1, 1, 1), (0, 0, float("nan"))), ((1, float("inf"), 1), (0, 0, 0)), "ab", ((1, 1, 1), (0, 0, 0), (0, 0, 0))):
        with pytest.raises(PbeError, match="tone"):
            ops_picture._tone_pair(bad)
    g, b = ops_picture._tone_pair(((1.25, 1, 0.5), (0.1, 0, -0.1)))
    assert list(g) == [1.25, 1.0, 0.5] and list(b) == [float(F(0.1)), 0.0, float(F(-0.1))]
    for tone in ("median", True, 1):
        with pytest.raises(PbeError, match="tone"):
            pipeline.inpaint_window(None, [pic], [pic[:, :, 0]], None, tone=tone)
        with pytest.raises(PbeError, match="tone"):
            pipeline.inpaint_holes(None, [pic], [pic[:, :, 0]], None, tone=tone)
    for margin in (-1, 1.5, None):
        with pytest.raises(PbeError, match="margin"):
            tone_selection(pic[:, :, 0], (0, 0, 10, 10), (8, 8), margin)
    with pytest.raises(PbeError, match="2047"):
        tone_selection(torch.zeros(16384, 4, dtype=torch.uint8), (0, 0, 16384, 4), (4, 4), 1)
