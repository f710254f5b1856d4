"""Per-element fp64 gate of the SiLU / erf-GELU / quick-GELU / GEGLU arms of the GEMM and conv epilogue, at every place igemm_kernel.h
applies them (tests/actref.py has the rounding model, the operands and the derivations):

  stage() with a compile-time activation (tiles with <= 96 accumulator registers), stage() with the run-time p.act (tiles 0 and 7),
  splitk_reduce_kernel, the fp8 tiles - all on operands whose pre-activation is exact, so the bound is the activation term plus the fp16
  store and nothing else - and, through tilecheck.expect on random operands, the LayerNorm fold followed by an activation and the gather /
  halo / split-K conv forms.  Every launch is forced onto its tile (ops.tune(1, ...)) and the recorded plan is asserted."""
import pytest
import torch

import actref
import tilecheck

pytestmark = pytest.mark.gpu

ACTS = (1, 2, 3, 4)
ARMS_TILES, RUNTIME_TILES, F8_TILES = (1, 2, 3, 4, 5, 6, 8, 9, 15, 16, 17, 18, 21), (0, 7), (3, 4, 6, 8, 9)
SPLITK = ((4, 2), (0, 3))


def test_tile_lists_are_the_geometry():
    assert list(ARMS_TILES) == actref.dense_tiles(True) and list(RUNTIME_TILES) == actref.dense_tiles(False) and list(F8_TILES) == actref.f8_tiles()


def _sweep(dev, site, tile, act, splits):
    """Every epilogue variant of one (tile, act) pair: exactness on the host first, then launch, plan check and per-element check."""
    bm = actref.tiles()[tile][0]
    worst = None
    with actref.forced_tile(tile, splits) as forced:
        for variant in actref.variants_of(act, splits):
            o = actref.dense_operands(bm, variant, act == 4, splits)
            actref.assert_exact(o)
            for resid in (False,) if act == 4 else (False, True):
                what = f"{site} tile {tile} split {splits} act {act} {variant}{' +resid' if resid else ''}"
                got = actref.launch_dense(o, act, dev, resid).cpu()
                forced.check(what)
                want, bound = actref.expect_exact(o["pre"], act, o["resid"] if resid else None)
                rep = tilecheck.check(got, want, bound, what)
                worst = rep if worst is None or rep.ratio > worst.ratio else worst
    print(f"\n[actgate] {site} act {act}: {worst}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("tile", ARMS_TILES)
def test_dense_compile_time_arm(dev, tile, act):
    _sweep(dev, "dense-arms", tile, act, 1)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("tile", RUNTIME_TILES)
def test_dense_run_time_act(dev, tile, act):
    _sweep(dev, "dense-runtime", tile, act, 1)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("tile,splits", SPLITK)
def test_splitk_reduce(dev, tile, splits, act):
    _sweep(dev, "splitk-reduce", tile, act, splits)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("tile", F8_TILES)
def test_fp8_tiles(dev, tile, act):
    bm = actref.tiles()[tile][0]
    o = actref.f8_operands(bm, act == 4)
    actref.assert_exact(o)
    worst = None
    with actref.forced_tile(tile, 1) as forced:
        for resid in (False,) if act == 4 else (False, True):
            what = f"fp8 tile {tile} act {act} bias{' +resid' if resid else ''}"
            got = actref.launch_f8(o, act, dev, resid).cpu()
            forced.check(what)
            want, bound = actref.expect_exact(o["pre"], act, o["resid"] if resid else None)
            rep = tilecheck.check(got, want, bound, what)
            worst = rep if worst is None or rep.ratio > worst.ratio else worst
    print(f"\n[actgate] fp8 act {act}: {worst}")


@pytest.mark.parametrize("act", (1, 2, 3))
@pytest.mark.parametrize("tile", (3, 4, 8, 9))
def test_layernorm_fold_then_activation(dev, tile, act):
    """ops.gemm(ln=..., act=1|2|3) on one extended-epilogue tile of each width: random operands, rows with mean >> std, pre-activation std 3."""
    case = actref.ln_case(tile, act)
    with actref.forced_tile(tile, 1) as forced:
        t = tilecheck.run_gemm(case, dev)
        forced.check(case.key)
    rows = tilecheck.gemm_rows(case.M, actref.tiles()[tile][0], tilecheck.seed_of(case.key))
    got, want, bound, labels = tilecheck.reference_gemm(case, t, [(0, rows)])
    assert want.abs().max() >= 10
    rep = tilecheck.check(got, want, bound, f"ln-fold tile {tile} act {act}", labels)
    print(f"\n[actgate] ln-fold act {act}: {rep}")


@pytest.mark.parametrize("act", (1, 2, 3))
@pytest.mark.parametrize("tile,splits", ((3, 1), (11, 1), (11, 2)))
def test_conv_activation(dev, tile, splits, act):
    """ops.conv3x3(act=1|2|3) with row vector and residual at 8x16x16x128 -> 160: the gather tile, the halo tile, the halo tile with split-K
    (the reduce kernel applies the activation); every output row of every sample is checked."""
    case = actref.conv_case(tile, splits, act)
    with actref.forced_tile(tile, splits) as forced:
        t = tilecheck.run_conv(case, dev)
        forced.check(case.key)
    sel = [(b, oy) for b in range(case.B) for oy in range(case.Ho)]
    got, want, bound, labels = tilecheck.reference_conv(case, t, sel)
    assert want.abs().max() >= 10
    rep = tilecheck.check(got, want, bound, f"conv tile {tile} split {splits} act {act}", labels)
    print(f"\n[actgate] conv{'-splitk' if splits > 1 else '-halo' if tile == 11 else '-gather'} act {act}: {rep}")


@pytest.mark.parametrize("act,other", ((1, 3), (2, 3), (3, 2)))
def test_gate_rejects_another_activation(dev, act, other):
    """Positive control on the device: the launch runs `other`, the gate expects `act` - it must report a ratio > 1 (GELU and quick-GELU
    differ by at most 0.02 anywhere: far inside the _close limit, far outside this gate)."""
    o = actref.dense_operands(128, "bias")
    with actref.forced_tile(3, 1) as forced:
        right, wrong = actref.launch_dense(o, act, dev).cpu(), actref.launch_dense(o, other, dev).cpu()
        forced.check("positive control")
    want, bound = actref.expect_exact(o["pre"], act)
    assert tilecheck.compare(right, want, bound).ratio <= 1.0
    rep = tilecheck.compare(wrong, want, bound, f"act {other} against the gate of act {act}")
    assert rep.ratio > 1.0, str(rep)


def test_gate_rejects_swapped_geglu_rows(dev):
    """Positive control for act 4, which no other activation can stand in for (it halves the width): the same launch with the value and
    gate rows of W exchanged computes gate * gelu(value) - the gate must report a ratio > 1."""
    from pbe_amd import ops
    o = actref.dense_operands(128, "bias", True)
    swapped = torch.stack([o["W"][1::2], o["W"][0::2]], 1).reshape(o["N"], o["K"]).contiguous()
    with actref.forced_tile(3, 1) as forced:
        right = actref.launch_dense(o, 4, dev).cpu()
        wrong = ops.gemm(o["A"].to(dev), swapped.to(dev), o["bias"].to(dev), act=4).cpu()
        forced.check("positive control, GEGLU")
    want, bound = actref.expect_exact(o["pre"], 4)
    assert tilecheck.compare(right, want, bound).ratio <= 1.0
    rep = tilecheck.compare(wrong, want, bound, "GEGLU with value and gate rows exchanged")
    assert rep.ratio > 1.0, str(rep)
