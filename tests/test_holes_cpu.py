"""One window per hole, host side (-m "not gpu"): the numpy restatement of tests/holesref.py against scipy, the strength of the GPU case
list (every wrong labeller of holesref.MUTANTS differs from the reference on one of its masks), the planner of pbe_amd/window.py
(plan_window_box, group_components, plan_holes) against that restatement, the CLI's flag checks and the declared symbols.  No kernel is
launched."""
import importlib.util
import os
import re

import numpy as np
import pytest

import holesref as hr
import windowref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pbe_mask_components_workspace_bytes", "pbe_mask_components_u8_i32", "pbe_component_boxes_workspace_bytes", "pbe_component_boxes_i32",
               "pbe_select_components_u8")


@pytest.fixture(autouse=True, scope="module")
def _the_entry_points_exist():
    """The reference and the case list below exist for the kernels: without the entry points nothing here says anything."""
    from pbe_amd import lib
    missing = [n for n in NEW_SYMBOLS if n not in lib.SYMBOLS]
    assert not missing, f"pbe_amd.lib.SYMBOLS lacks {missing}"


def _random_holes(shape, seed, n=7):
    """A mask of n small rectangles and single pixels at random places."""
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 128, size=shape).astype(np.uint8)
    for _ in range(n):
        y, x = rs.randint(0, shape[0]), rs.randint(0, shape[1])
        m[y:y + rs.randint(1, 9), x:x + rs.randint(1, 12)] = rs.choice([128, 255])
    return m


def test_reference_labels_agree_with_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for pattern, shape in hr.CASES:
        mask = hr.case_mask(pattern, shape)
        for conn in (8, 4):
            lab, n = ndi.label(mask >= 128, structure=np.ones((3, 3), dtype=int) if conn == 8 else None)
            ref = hr.case_labels(pattern, shape, conn)
            want = np.full(mask.shape, -1, dtype=np.int64)
            if n:
                first = ndi.minimum(np.arange(mask.size).reshape(mask.shape), lab, index=np.arange(1, n + 1)).astype(np.int64)
                want = np.where(lab > 0, first[np.maximum(lab, 1) - 1], -1)
            assert np.array_equal(ref, want), (pattern, shape, conn)
            table = hr.boxes_ref(ref)
            assert table.shape == (n, 6) and int(table[:, 5].sum()) == int((mask >= 128).sum())
            if 0 < n < 50:
                objects = ndi.find_objects(lab)
                for l, ya, yb, xa, xb, area in table.tolist():
                    k = int(lab[l // mask.shape[1], l % mask.shape[1]])
                    ys, xs = objects[k - 1]
                    assert (ya, yb + 1, xa, xb + 1) == (ys.start, ys.stop, xs.start, xs.stop) and area == int((lab == k).sum())


def test_the_case_list_says_what_the_issue_names():
    lab = lambda p, s, c: hr.case_labels(p, s, c)                              # noqa: E731
    count = lambda p, s, c: hr.boxes_ref(lab(p, s, c)).shape[0]                # noqa: E731
    for s in hr.SHAPES:
        assert count("all_hole", s, 8) == count("all_hole", s, 4) == 1 and (lab("all_hole", s, 4) == 0).all()
        assert count("no_hole", s, 8) == 0 and (lab("no_hole", s, 8) == -1).all()
        assert count("last_corner", s, 8) == 1 and lab("last_corner", s, 8)[-1, -1] == s[0] * s[1] - 1
        assert count("checkerboard", s, 8) == (1 if min(s) > 1 else (max(s) + 1) // 2) and count("checkerboard", s, 4) == (s[0] * s[1] + 1) // 2
        assert count("spiral", s, 8) == count("spiral", s, 4) == 1 and count("serpentine", s, 4) == 1
        m = hr.case_mask("threshold", s)
        assert set(np.unique(m)) == {127, 128} and np.array_equal(lab("threshold", s, 8) >= 0, m == 128)
    assert count("checkerboard", (90, 130), 4) > 4096
    assert count("diagonal", (90, 130), 8) == 2 and count("diagonal", (90, 130), 4) == 90 + 60
    assert int((hr.case_mask("spiral", (129, 257)) >= 128).sum()) > 15000          # a path of tens of thousands of pixels
    wide = lab("wide_u", (129, 257), 4)
    assert wide[0, 256] == 0 and wide[0, 128] == 128                               # the far arm takes the first pixel's index through the last row
    for p in ("noise41", "noise59"):
        dens = float((hr.case_mask(p, (129, 257)) >= 128).mean())
        assert abs(dens - (0.41 if p == "noise41" else 0.59)) < 0.02
        assert 1 <= count(p, (129, 257), 8) < count(p, (129, 257), 4)
    assert count("noise41", (129, 257), 8) > 100


@pytest.mark.parametrize("mutant", hr.MUTANTS, ids=[m.__name__ for m in hr.MUTANTS])
def test_every_mutant_is_caught_by_the_case_list(mutant):
    caught = next(((p, s) for p, s in hr.CASES if not np.array_equal(mutant(hr.case_mask(p, s), 8), hr.case_labels(p, s, 8))), None)
    assert caught is not None, f"no mask of holesref.CASES tells {mutant.__name__} from the reference"
    print(f"{mutant.__name__}: caught by {caught}")


def test_mutants_are_wrong_for_the_reason_they_name():
    m, ref = hr.case_mask("wide_u", (129, 257)), hr.case_labels("wide_u", (129, 257), 8)
    assert ref[0, 0] == 0 and ref[0, 256] == 0
    for T in hr.TILES:
        got = hr.tile_local(T)(m, 8)
        assert np.array_equal(got >= 0, ref >= 0) and not np.array_equal(got, ref)
        assert got[0, 0] == 0 and got[0, 256] == 256                                               # the arms meet in row 128 only: another tile
    allh = hr.case_mask("all_hole", (90, 130))
    assert np.array_equal(hr.first_seen(allh, 8), hr.case_labels("all_hole", (90, 130), 8))        # (0, 0) is first in both orders
    anti = hr.case_mask("antidiagonal", (90, 130))
    assert not np.array_equal(hr.first_seen(anti, 8), hr.case_labels("antidiagonal", (90, 130), 8))
    diag = hr.case_mask("diagonal", (90, 130))
    assert np.array_equal(hr.no_diagonal(diag, 4), hr.case_labels("diagonal", (90, 130), 4))
    assert not np.array_equal(hr.no_diagonal(diag, 8), hr.case_labels("diagonal", (90, 130), 8))


def test_plan_window_is_plan_window_box_of_the_hole_box():
    from pbe_amd.window import hole_box, plan_window, plan_window_box
    n = 0
    for name, shape, win, size in wr.IMAGE_CASES:
        for seed in (4, 5, 6):
            mask = wr.random_mask(shape, seed)
            for context, feather in ((0.5, 8), (0.0, 0), (1.25, 3), (0.1, 40)):
                assert plan_window(mask, size, context, feather) == plan_window_box(hole_box(mask), shape, size, context, feather)
                n += 1
    assert n == len(wr.IMAGE_CASES) * 12
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError, match="not inside"):
        plan_window_box((0, 20, 0, 5), (20, 30), (8, 8))
    with pytest.raises(PbeError, match="feather"):
        plan_window_box((0, 2, 0, 5), (20, 30), (8, 8), 0.5, -1)


def test_grouping_equals_the_reference_and_ignores_the_row_order():
    from pbe_amd.window import group_components
    rs = np.random.RandomState(3)
    merged_some = 0
    for seed in range(12):
        mask = _random_holes((150, 220), seed, n=4 + seed)
        table = hr.boxes_ref(hr.label_ref(mask, 8))
        for r in (0, 1, 3, 8):
            want = hr.groups_ref(table, r)
            got = group_components(table, r)
            assert [(g[0], g[1]) for g in got] == want, (seed, r)
            assert sorted(l for g in got for l in g[0]) == table[:, 0].tolist()                    # a partition: no component dropped or doubled
            areas = {int(row[0]): int(row[5]) for row in table}
            assert all(g[2] == sum(areas[l] for l in g[0]) for g in got)
            for _ in range(3):
                assert group_components(table[rs.permutation(table.shape[0])], r) == got
            merged_some += len(got) < table.shape[0]
    assert merged_some > 10
    # A and B join; D is far from both (8 and 13) but only 5 rows below their union box, which reaches over it
    chain = np.array([[0, 0, 4, 0, 4, 25], [900, 8, 12, 9, 13, 25], [5000, 17, 18, 0, 1, 4]], dtype=np.int64)
    assert [g[0] for g in group_components(chain, 1)] == [(0, 900, 5000)] == [g[0] for g in hr.groups_ref(chain, 1)]
    assert [g[0] for g in group_components(chain, 0)] == [(0,), (900,), (5000,)]                   # gaps 5, 8 and 13 > 2
    two = np.array([[0, 0, 0, 0, 0, 1], [7, 0, 0, 7, 7, 1]], dtype=np.int64)                      # distance 7: 2m = 6 at r = 1, 10 at r = 2
    assert len(group_components(two, 1)) == 2 and len(group_components(two, 2)) == 1
    assert len(group_components(two[:, [0, 3, 4, 1, 2, 5]], 1)) == 2                               # the same along y


@pytest.mark.parametrize("r", [0, 1, 8])
def test_alpha_supports_of_different_groups_are_disjoint(r):
    from pbe_amd.window import group_components
    several = 0
    for seed in range(6):
        mask = _random_holes((120, 160), 100 + seed, n=9)
        labels = hr.label_ref(mask, 8)
        groups = group_components(hr.boxes_ref(labels), r)
        assert [(g[0], g[1]) for g in groups] == [(ls, box) for ls, box, _ in hr.group_masks_ref(mask, r)]
        cover = np.zeros(mask.shape, dtype=np.int64)
        for ls, box, gm in hr.group_masks_ref(mask, r):
            alpha = wr.alpha_ref(gm, (0, 0, *mask.shape), r)
            assert (alpha[gm >= 128] == 1).all()
            cover += alpha > 0
        assert cover.max() == 1, f"seed {seed} r {r}: a pixel lies in the blend zone of {cover.max()} groups"
        whole = wr.alpha_ref(mask, (0, 0, *mask.shape), r) > 0
        assert np.array_equal(cover > 0, whole)                                                    # together they are the whole mask's zone
        several += len(groups) > 1
    assert several >= 4


def test_plan_holes_windows_limits_and_errors():
    from pbe_amd.lib import PbeError
    from pbe_amd.window import plan_holes, plan_window
    mask = np.zeros((200, 300), dtype=np.uint8)
    mask[70:130, 110:190] = 255
    mask[60:64, 100:104] = 200                                                                     # 7 rows above the large one: one group at r = 8
    table = hr.boxes_ref(hr.label_ref(mask, 8))
    assert table.shape[0] == 2
    plan = plan_holes(table, mask.shape, (128, 128), 0.5, 8)
    assert plan == [((60 * 300 + 100, 70 * 300 + 110), (60, 129, 100, 189), plan_window(mask, (128, 128), 0.5, 8))]
    far = np.zeros((300, 400), dtype=np.uint8)
    far[30:50, 40:70] = 255
    far[220:250, 300:340] = 129
    t2 = hr.boxes_ref(hr.label_ref(far, 8))
    plan = plan_holes(t2[::-1], far.shape, (128, 128), 0.5, 8)
    assert [p[0] for p in plan] == [(30 * 400 + 40,), (220 * 400 + 300,)] and [p[1] for p in plan] == [(30, 49, 40, 69), (220, 249, 300, 339)]
    for (ls, box, win), gm in zip(plan, (hr.select_ref(hr.label_ref(far, 8), p[0]) for p in plan)):
        assert win == plan_window(gm, (128, 128), 0.5, 8)                                          # each as if it were the only hole
    with pytest.raises(PbeError, match=r"2 separate holes.*max_holes = 1.*inpaint_window"):
        plan_holes(t2, far.shape, (128, 128), 0.5, 8, max_holes=1)
    assert len(plan_holes(t2, far.shape, (128, 128), 0.5, 8, max_holes=2)) == 2
    with pytest.raises(PbeError, match="no hole"):
        plan_holes(np.zeros((0, 6), dtype=np.int64), far.shape, (128, 128))
    with pytest.raises(PbeError, match="no hole"):
        plan_window(np.zeros((20, 20), dtype=np.uint8), (8, 8))


def test_cli_flag_combinations_that_must_exit():
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_holes", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    for argv, word in ((["--per_hole"], "--paste_back"), (["--per_hole", "--paste_back", "--n_samples", "2"], "--n_samples 2"),
                       (["--per_hole", "--paste_back", "--dump_tensors", "x.npz"], "--dump_tensors"), (["--reference_per_hole", "--paste_back"], "--per_hole")):
        with pytest.raises(SystemExit) as e:
            cli.parse(argv)
        assert word in str(e.value), (argv, e.value)
    opt = cli.parse(["--per_hole", "--paste_back", "--reference_per_hole", "--reference_path", "a.png", "b.png"])
    assert opt.per_hole and opt.reference_per_hole and opt.max_holes == 16
    plain = cli.parse(["--paste_back"])
    assert not plain.per_hole and not plain.reference_per_hole


def test_new_symbols_are_declared_in_the_header_and_in_lib():
    from pbe_amd import lib
    header = open(os.path.join(ROOT, "include", "pbe_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pbe_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in lib.SYMBOLS, name
    assert "holes.hip" in lib.SOURCES and os.path.exists(os.path.join(ROOT, "pbe_amd", "csrc", "holes.hip"))
    assert lib.ABI_VERSION == 8
    from pbe_amd.build import build
    build()
    handle = lib.load()
    assert handle.pbe_mask_components_workspace_bytes(100, 100) > 0
    assert handle.pbe_component_boxes_workspace_bytes(100, 100, 4096) >= 2 * 4 * 2 * 4096 and handle.pbe_component_boxes_workspace_bytes(100, 100, 0) == 0
