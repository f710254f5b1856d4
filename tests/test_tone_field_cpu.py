"""The tone field without a GPU: tests/fieldref.py against itself (plain loop against vectorised, fp32 emulation against fp64 under the
derived tolerances), the properties the issue names (a constant difference stays a constant bit for bit, too little evidence gives
zeros, the clamp), a planted smooth tone recovered, every wrong variant told from the right answer by a case the GPU tests run as well,
and the refusals of the host layer that need no device."""
import numpy as np
import pytest

import fieldref as fr
import maskref as mr
import toneref as tr
import windowref as wr

F = np.float32
SMALL_CELL_CASES = [c for c in fr.CELL_CASES if c[0][0] * c[0][1] * c[0][2] <= 1100]


@pytest.fixture(scope="module")
def cell_tables():
    """The vectorised table of every cell case, computed once and left unchanged."""
    out = {}
    for case in fr.CELL_CASES:
        shape, mode, cell = case
        image, result, sel = tr.stats_inputs(shape, mode)
        out[case] = (image, result, sel, fr.cells_ref(image, result, sel, cell))
    return out


# ---- the cell table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL_CELL_CASES, ids=fr.cell_case_id)
def test_cells_loop_equals_vectorised(cell_tables, case):
    image, result, sel, want = cell_tables[case]
    got = fr.cells_loop(image, result, sel, case[2])
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


def test_cell_table_properties(cell_tables):
    for case, (image, result, sel, t) in cell_tables.items():
        (B, H, W), mode, cell = case
        assert t.shape == (B, 4) + fr.grid_of(H, W, cell)
        # the cells add up to tone_stats' whole-window numbers: n and So - Sq
        stats = tr.stats_ref(image, result, sel)
        assert np.array_equal(t[:, 0].sum(axis=(1, 2)), stats[:, 0, 0])
        assert np.array_equal(t[:, 1:].sum(axis=(2, 3)), stats[:, :, 1] - stats[:, :, 2])
        assert t[:, 0].max() <= cell * cell and np.abs(t[:, 1:]).max() <= 255 * cell * cell < 1 << 21
        if mode == "zeros":
            assert not t.any()
        if mode == "ones":
            full = np.minimum(cell, H - np.arange(t.shape[2]) * cell)[:, None] * np.minimum(cell, W - np.arange(t.shape[3]) * cell)[None, :]
            assert np.array_equal(t[:, 0], np.broadcast_to(full, t[:, 0].shape))


@pytest.mark.parametrize("name", list(fr.CELL_FAULTS))
def test_cell_faults_are_told_apart(cell_tables, name):
    hit = [fr.cell_case_id(case) for case, (image, result, sel, want) in cell_tables.items()
           if not np.array_equal(fr.cells_ref(image, result, sel, case[2], **fr.CELL_FAULTS[name]), want)]
    assert hit, f"no cell case tells '{name}' from the right table"


# ---- the field -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields():
    out = {}
    for grid in fr.FIELD_GRIDS:
        t = fr.random_table(grid)
        out[grid] = (t, fr.field64(t), fr.field32(t))
    return out


@pytest.mark.parametrize("grid", fr.FIELD_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_field32_is_within_the_derived_tolerance_of_fp64(fields, grid):
    t, f64, f32 = fields[grid]
    L = fr.levels_of(grid)
    assert len(fr.pull(t)) == L and fr.pull(t)[-1].shape == (4, 1, 1)
    assert [int(v) for v in fr.pull(t)[-1][:, 0, 0]] == [int(v) for v in t.astype(np.int64).sum(axis=(1, 2))]
    assert f32.dtype == F and f32.shape == (3,) + grid and np.abs(f32).max() <= 0.125 + fr.field_tol(L)      # the blend's roundings may pass the limit by an ulp
    err = float(np.abs(f32.astype(np.float64) - f64).max())
    print(f"grid {grid}: {L} levels, |fp32 - fp64| <= {err:.3g}, tolerance {fr.field_tol(L):.3g}")
    assert err <= fr.field_tol(L)
    assert np.abs(f64).max() > 0.05, "the case does not exercise the field"


@pytest.mark.parametrize("grid", [(1, 1), (3, 2), (5, 7), (13, 16)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("d", [7, -3, 31])
def test_a_constant_difference_stays_a_constant_bit_for_bit(grid, d):
    t = fr.constant_table(grid, d)
    f = fr.field32(t)
    assert (t[0] == 0).any() or grid == (1, 1)
    assert np.array_equal(f.view(np.int32), np.full(f.shape, F(d / 255.0), dtype=F).view(np.int32)), f"grid {grid}, d {d}: the field is not (float)(d / 255) everywhere"
    assert np.array_equal(fr.field64(t), np.full(f.shape, d / 255.0))


def test_too_little_evidence_gives_zeros_and_the_clamp_holds():
    t = fr.random_table((5, 7))
    empty = t.copy()
    empty[:] = 0
    assert not fr.field32(empty).any() and not fr.field32(empty, min_pixels=0).any()
    few = np.zeros((4, 5, 7), dtype=np.int32)
    few[:, 2, 3] = (63, 630, -630, 63)
    assert not fr.field32(few).any() and fr.field32(few, min_pixels=63).any()
    # a difference beyond the limit: every value is clamped, at any limit
    big = fr.constant_table((5, 7), 60)
    for limit in (0.125, 0.05):
        f = fr.field32(big, limit=limit)
        assert np.array_equal(f, np.full(f.shape, F(limit), dtype=F))
        assert np.array_equal(fr.field32(-big * np.array([-1, 1, 1, 1])[:, None, None], limit=limit), -f)
    assert abs(float(np.abs(fr.field32(fr.random_table((13, 16), amp=120.0))).max()) - 0.125) <= fr.field_tol(5)


@pytest.mark.parametrize("name", list(fr.FIELD_FAULTS))
def test_field_faults_are_told_apart(fields, name):
    hit = []
    for grid, (t, f64, _) in fields.items():
        bad = fr.field32(t, **fr.FIELD_FAULTS[name])
        if np.abs(bad.astype(np.float64) - f64).max() > fr.field_tol(fr.levels_of(grid)):
            hit.append(grid)
    assert hit, f"no field grid tells '{name}' from the right field"


# ---- the paste -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pastes():
    return {case[0]: (case,) + fr.paste_field_inputs(case) for case in fr.PASTE_CASES}


@pytest.mark.parametrize("name", [c[0] for c in fr.PASTE_CASES])
def test_paste_field_emulation_passes_its_gate(pastes, name):
    case, pic, result, alpha, field = pastes[name]
    _, shape, win, size, cell = case
    emu = fr.paste_field32(pic, result, alpha, win, field, cell)
    changed, near, live = fr.gate_paste_field(emu, pic, result, alpha, win, field, cell, what=name)
    print(f"{name}: {changed} of {live} bytes of the fp32 emulation differ from fp64, {near} ({100.0 * near / live:.3f} %) lie at a tie")
    assert near <= wr.PASTE_TIE_CAP * live and changed <= near
    assert (emu != wr.paste32(pic, result, alpha, win)).any()
    # a zero field is the plain paste, a constant field b the tone paste at gain 1 and offset b, byte for byte
    assert np.array_equal(fr.paste_field32(pic, result, alpha, win, np.zeros_like(field), cell), wr.paste32(pic, result, alpha, win))
    b = F(0.0625)
    assert np.array_equal(fr.paste_field32(pic, result, alpha, win, np.full_like(field, b), cell), tr.paste_tone32(pic, result, alpha, win, (1.0,) * 3, (b,) * 3))


@pytest.mark.parametrize("fault", fr.PASTE_FAULTS)
def test_paste_faults_are_rejected(pastes, fault):
    hit = []
    for name, (case, pic, result, alpha, field) in pastes.items():
        _, shape, win, size, cell = case
        try:
            fr.gate_paste_field(fr.paste_field32(pic, result, alpha, win, field, cell, fault=fault), pic, result, alpha, win, field, cell, what=name)
        except AssertionError:
            hit.append(name)
    assert hit, f"no paste case rejects '{fault}'"


# ---- a planted smooth tone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fr.RAMP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_planted_ramp_is_followed(shape):
    """Over the blend zone (0 < alpha < 1: where the window is mixed with the picture) the field's rms error against the planted ramp is
    at most a quarter of what one offset per window leaves.  The constant channel is only reported: there the field may be noisier."""
    pic, mask, result, planted = fr.ramp_case(shape)
    win = (0, 0) + shape
    image = wr.image32(pic, win, shape)
    sel = wr.mask_ref(mr.grow_ref(mask, fr.RAMP_MARGIN), win, shape)
    cells = fr.cells_ref(image[None], result[None], sel[None])[0]
    field = fr.field32(cells)
    top = fr.pull(cells)[-1][:, 0, 0]
    offset = [int(top[1 + c]) / (255.0 * int(top[0])) for c in range(3)]
    alpha = wr.alpha_ref(mask, win, fr.RAMP_FEATHER)
    zone = (alpha > 0) & (alpha < 1)
    assert zone.sum() > 100 and not sel[0][mask >= 128].any()
    ef, em = fr.ramp_errors(field, offset, planted, zone)
    print(f"{shape}: rms error over the blend zone, grey levels: field {ef.round(3).tolist()}, one offset {em.round(3).tolist()}, ratio {(ef[:2] / em[:2]).round(3).tolist()}")
    assert (ef[:2] <= 0.25 * em[:2]).all()


# ---- the host layer's refusals that need no device -------------------------------------------------------------------------------------
def test_modes_and_refusals():
    from pbe_amd import pipeline, window
    from pbe_amd.lib import PbeError
    assert window.TONE_MODES == pipeline.TONE_MODES == ("mean", "affine", "field")
    with pytest.raises(PbeError, match="tone_field"):
        window.fit_tone([[[0] * 6] * 3], mode="field")
    with pytest.raises(PbeError, match="match_tone_field"):
        pipeline.match_tone(None, None, [], [], (8, 8), "field")
    for kw, pattern in ((dict(cell=5), "cell"), (dict(cell=True), "cell"), (dict(limit=0.0), "limit"), (dict(limit=float("nan")), "limit"),
                        (dict(limit=float("inf")), "limit"), (dict(limit="x"), "limit"), (dict(min_pixels=-1), "min_pixels"), (dict(min_pixels=1.5), "min_pixels")):
        with pytest.raises(PbeError, match=pattern):
            window.tone_field(None, None, None, **kw)
    assert [window.field_levels(g) for g in fr.FIELD_GRIDS] == [fr.levels_of(g) for g in fr.FIELD_GRIDS] == [1, 4, 3, 4, 4, 5, 7]
    pipeline._check_tone("inpaint_window", "field")
    with pytest.raises(PbeError, match="tone"):
        pipeline._check_tone("inpaint_window", "median")
