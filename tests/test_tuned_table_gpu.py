"""Every entry of the tuned tile table (pbe_amd/tuned_mi355x.json) launched at its own shape and checked against an fp64 reference,
element by element, on sampled output rows (tests/tilecheck.py: launch rule, sampling and rounding model).

Per entry: the launch ran exactly the table's (tile, split-K) (ops._PLANS), the sampled elements are within their bounds, the row /
group statistics the epilogue emitted match fp64 sums of the stored output, and a halo conv tile at split 1 reproduces the bits of the
gather tile 9 wherever tile 9 plans for the shape.  One sensitivity test per form shows the gate rejects a launch whose last 64-wide
k-slice was zeroed.  PBE_TILECHECK_REPORT=<file> appends one JSON line per entry (worst bound ratio, location)."""
import json
import os

import pytest
import torch

import tilecheck as tc

pytestmark = pytest.mark.gpu

TABLE = tc.load_table()
KEYS = list(TABLE)


def _ids():
    try:
        return [tc.case_of(k).id for k in KEYS]
    except Exception:                            # library not built at collection time: the key alone
        return KEYS


def _launch(case, dev, mutate=False):
    from pbe_amd import ops
    try:
        ops._PLANS = []
        t = tc.run_case(case, dev, mutate=mutate)
        plans = ops._PLANS
    finally:
        ops._PLANS = None
    assert len(plans) == 1 and plans[0][0] == case.key, (case.describe(), plans)
    _, cfg, splits, bm, bn, _ = plans[0]
    assert (cfg, max(1, splits)) == (case.tile, case.splits), f"{case.describe()}: launch ran tile {cfg} split-K {splits}"
    return t, bm


def _report(case, rep, **extra):
    path = os.environ.get("PBE_TILECHECK_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(key=case.key, id=case.id, form=case.form, tile=case.tile, splits=case.splits, ratio=rep.ratio,
                                    where=rep.where, n=rep.n, **extra)) + "\n")


@pytest.mark.parametrize("key", KEYS, ids=_ids())
def test_tuned_entry_against_fp64(dev, key):
    from pbe_amd import ops
    case = tc.case_of(key)
    with torch.no_grad():
        t, bm = _launch(case, dev)
        got, want, bound, labels = tc.sampled(case, t, bm)
        rep = tc.check(got, want, bound, case.describe(), labels)
        extra = {}
        y = t["out"]
        if case.row_stats:
            st = t["stats"]
            s = st.buf[:st.parts].double().sum(0)
            yd = y.double()
            ref = torch.stack([yd.sum(1), (yd ** 2).sum(1)], 1)
            assert torch.allclose(s, ref, rtol=2e-6, atol=1e-4), f"{case.id}: row statistics off by {(s - ref).abs().max().item():.3e}"
            extra["row_stats"] = st.parts
        st = getattr(y, "_pbe_gstats", None) if case.form == "c" else None
        if st is not None:
            B, G = case.B, st.groups
            tot = st.view().double().sum(1)
            yg = y.double().view(B, case.Ho * case.Wo, G, case.Cout // G)
            ref = torch.stack([yg.sum((1, 3)), (yg ** 2).sum((1, 3))], -1)
            assert torch.allclose(tot, ref, rtol=2e-6, atol=1e-3), f"{case.id}: group statistics off by {(tot - ref).abs().max().item():.3e}"
            extra["group_stats"] = st.blocks
        if case.form == "c" and 10 <= case.tile <= 14 and case.splits == 1:
            try:
                ops.tune(1, 9 | (1 << 8))
                ops._PLANS = []
                y9 = ops.conv3x3(t["x1"], t["wpacked"], t["bias"], x2=t["x2"], stride=case.stride, pad=case.pad, upsample=bool(case.ups), **t["kw"])
                p9 = ops._PLANS[0]
            finally:
                ops.tune(1, -1)
                ops._PLANS = None
            if (p9[1], max(1, p9[2])) == (9, 1):
                assert torch.equal(y, y9), f"{case.id}: halo tile {case.tile} and gather tile 9 differ in {int((y != y9).sum())} elements"
                extra["halo_equal_tile9"] = True
    _report(case, rep, **extra)


@pytest.mark.parametrize("form", ["g", "gx", "g8", "c"])
def test_gate_rejects_zeroed_last_kslice(dev, form):
    """The gate can fail on the GPU: the same launch with the weights' last 64-wide k-slice (conv: last input-channel block) zeroed in a
    device copy is rejected against the reference of the intact operands."""
    key = tc.sensitivity_key(TABLE, form)
    case = tc.case_of(key)
    with torch.no_grad():
        t, bm = _launch(case, dev, mutate=True)                          # (t holds the intact operands the reference reads)
        got, want, bound, labels = tc.sampled(case, t, bm)
    rep = tc.compare(got, want, bound, case.describe(), labels)
    assert rep.ratio > 1.0, f"zeroed k-slice not detected: {rep}"
