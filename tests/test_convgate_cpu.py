"""The gate of the conv-side block chains (tests/convref.py) on the CPU: plain() pinned to the oracle, the pack restatements pinned to
the packers bit for bit, the emulation under its own verdict on every case test_convgate_gpu.py runs (both summation orders, both
GroupNorm statistics routes), and the planted wiring faults, each of which the verdict must reject on a case the test names.

The eps faults (GroupNorm eps 1e-5 against 1e-6) are the reason for the `flat` and `hole` recipes: on a unit-variance map the swap moves
the output by about 5e-6 relative, which no whole-tensor limit sees - test_eps_faults_pass_the_rel_l2_terms_on_unit_inputs holds that
claim to the verdict's own rel-L2 terms - while on a map whose group variance is near eps it moves rstd by a tenth and more."""
import pytest
import torch
import torch.nn.functional as F

import convref as R
from oracle_loader import O

IDS = [c["id"] for c in R.CASES]
EPS_FAULTS = [n for n in R.FAULTS if "eps" in n]


def _nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous()


def _oracle(c, sd, inp):
    """The block by oracle/pbe_oracle.py (fp32, NCHW) -> NHWC."""
    kind, x = c["kind"], _nchw(inp["x"])
    if kind == "res":
        if inp["skip"] is not None:
            x = torch.cat([x, _nchw(inp["skip"])], 1)
        y = O.res_block(sd, "", x, inp["emb"])
    elif kind in ("unet_up", "vup"):
        y = O.conv(F.interpolate(x, scale_factor=2, mode="nearest"), sd, "conv", padding=1)
    elif kind == "unet_down":
        y = O.conv(x, sd, "op", stride=2, padding=1)
    elif kind == "vdown":
        y = O.conv(F.pad(x, (0, 1, 0, 1)), sd, "conv", stride=2)
    elif kind == "unet_in":
        y = O.conv(x, sd, "input_blocks.0.0", padding=1)
    elif kind == "unet_out":
        y = O.conv(F.silu(O.group_norm(x, sd, "out.0", 1e-5)), sd, "out.2", padding=1)
    elif kind == "vres":
        y = O.vae_resnet(sd, "", x)
    elif kind == "vattn":
        y = O.vae_attn(sd, "", x)
    else:
        h = O.conv(x, sd, "conv_in", padding=1)
        y = O.conv(F.silu(O.group_norm(h, sd, "norm_out", 1e-6)), sd, "conv_out", padding=1)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("cid", IDS)
def test_plain_is_the_oracles_block(cid):
    """plain() (fp64) against the oracle (fp32): rel-L2 <= 1e-5.  The ResBlock's plain takes the embedding rows unrounded here, as the
    oracle computes them from emb; and ref64 stays within the weight roundings of it (the phase form of the upsampling conv included)."""
    r = R.refs(cid)
    inp = dict(r.inp)
    if inp["emb"] is not None:
        inp["emb_out"] = R.emb_rows64(r.sd, inp["emb"])
    got = R.plain(r.c, r.sd, inp)
    want = _oracle(r.c, r.sd, inp)
    assert got.shape == want.shape
    rel = R.rel_l2(want, got)
    assert rel <= 1e-5, (cid, rel)
    if R.unit_scale(r.c):
        assert R.rel_l2(r.ref64(), r.plain()) <= 1e-3, cid


def test_pack_restatements_equal_the_packers_bit_for_bit():
    from pbe_amd import ops
    g = torch.Generator().manual_seed(11)
    for co, ci in ((64, 64), (32, 192), (4, 128)):
        w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
        assert torch.equal(R.packed_conv3x3(w), ops.pack_conv3x3(w)), (co, ci)
        assert torch.equal(R.packed_up_phases(w), ops.pack_conv3x3_up_phases(w)), (co, ci)
    for co, ci, pad in ((64, 9, 16), (64, 3, 8), (128, 4, 8)):
        w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
        assert torch.equal(R.packed_conv3x3(w, pad), ops.pack_conv3x3(w, pad)), (co, ci)
    for shape in ((128, 192, 1, 1), (64, 32)):
        w = torch.randn(shape, generator=g)
        assert torch.equal(R.packed_linear(w), ops.pack_linear(w)), shape
    # the AttnBlock packs cat([q, k]) as one matrix: the same values row for row
    wq, wk = torch.randn(64, 64, 1, 1, generator=g), torch.randn(64, 64, 1, 1, generator=g)
    assert torch.equal(torch.cat([R.packed_linear(wq), R.packed_linear(wk)], 0), ops.pack_linear(torch.cat([wq, wk], 0)))
    # the values the arithmetic uses ARE the packed values: the same multiset per output channel
    w = torch.randn(8, 64, 3, 3, generator=g)
    assert torch.equal(R.round_conv(w).reshape(8, -1).sort(1).values, R.packed_conv3x3(w).sort(1).values)
    assert torch.equal(torch.stack([k.reshape(8, -1) for k in R.phase_weights(w)]).sort(2).values, R.packed_up_phases(w).sort(2).values)


def _stats_modes(c):
    """(stats, stats_rows) the emulation takes for a case: both routes for the U-Net ResBlock (the conv's tile rows must divide HW)."""
    modes = [("two_pass", None)]
    HW = c["hw"][0] * c["hw"][1]
    if c["kind"] == "res":
        modes += [("conv", rows) for rows in (32, 64, 128, 256) if HW % rows == 0 and HW >= 64]
    return modes


@pytest.mark.parametrize("cid", IDS)
def test_emulation_passes_its_own_verdict(cid):
    r = R.refs(cid)
    for stats, rows in _stats_modes(r.c):
        for reverse in (False, True):
            ok, text = r.verdict(r.emu(reverse, stats, rows), stats, rows)
            print(f"convgate cpu  {cid:34s} {stats:8s} rows {rows or '-':>4} {'reverse' if reverse else 'forward'}: {text}")
            assert ok, (cid, stats, rows, reverse, text)


@pytest.mark.parametrize("cid", IDS)
def test_a_third_summation_order_passes_the_verdict(cid):
    """What PEAK is for: the chain summed in an order neither emulation took (every K in a seeded permutation) is accepted."""
    r = R.refs(cid)
    for seed in (1, 2):
        ok, text = r.verdict(r.emu(reverse=seed))
        print(f"convgate cpu  {cid:34s} two_pass permuted K, seed {seed}: {text}")
        assert ok, (cid, seed, text)


def _rejecting_cases(name, recipes=None, kind=None):
    out = []
    for c in R.CASES:
        if not R.fault_applies(name, c) or (recipes and c["recipe"] not in recipes) or (kind and c["kind"] != kind):
            continue
        r = R.refs(c["id"])
        ok, text = r.verdict(r.emu(fault=name))
        if not ok:
            out.append((c["id"], text))
    return out


@pytest.mark.parametrize("name", list(R.FAULTS))
def test_fault_is_rejected(name):
    """Every planted fault is rejected by the verdict on at least one case of each block kind it applies to."""
    for kind in R.FAULTS[name][0]:
        hits = _rejecting_cases(name, kind=kind)
        assert hits, f"fault '{name}' ({R.FAULTS[name][2]}) is rejected on no {kind} case"
        print(f"convgate cpu  fault '{name}' [{kind}]: rejected on {hits[0][0]} ({len(hits)} case(s)): {hits[0][1]}")


@pytest.mark.parametrize("name", EPS_FAULTS)
def test_eps_fault_is_rejected_on_a_flat_or_hole_case(name):
    for kind in R.FAULTS[name][0]:
        hits = _rejecting_cases(name, ("flat", "hole"), kind)
        assert hits, f"eps fault '{name}' is rejected on no flat / hole case of {kind}"
        print(f"convgate cpu  eps fault '{name}' [{kind}]: rejected on {hits[0][0]}: {hits[0][1]}")


@pytest.mark.parametrize("name", EPS_FAULTS)
def test_eps_faults_pass_the_rel_l2_terms_on_unit_inputs(name):
    """Why the flat / hole recipes exist: on unit-variance inputs the rel-L2 terms (the emulation factor and BLOCK_TOL) accept the swap."""
    seen = 0
    for c in R.CASES:
        if R.fault_applies(name, c) and c["recipe"] == "unit":
            r = R.refs(c["id"])
            assert r.rel_l2_terms_accept(r.emu(fault=name)), (name, c["id"])
            seen += 1
    assert seen, name


def test_cases_hold_what_the_gate_names():
    have = {(c["kind"], c["form"]) for c in R.CASES}
    assert have >= {("res", "id"), ("res", "1x1"), ("res", "cat"), ("unet_up", "phase"), ("unet_down", "s2p1"), ("unet_out", "head"),
                    ("unet_in", "small"), ("vres", "id"), ("vres", "nin"), ("vattn", "attn"), ("vdown", "p0101"), ("vup", "phase"),
                    ("venc", "head"), ("vdec", "head")}
    assert {c["kind"] for c in R.CASES} == set(R.KINDS)
    assert all(c["B"] == 3 for c in R.CASES)
    for kind in ("res", "vres"):                                       # the three maps and both channel counts on the chained blocks
        assert {c["hw"] for c in R.CASES if c["kind"] == kind} == {(8, 8), (12, 8), (16, 16)}
        assert {c["C"] for c in R.CASES if c["kind"] == kind} == {64, 128}
    cat = [c for c in R.CASES if c["form"] == "cat"]
    assert all((c["C"], c["C2"], c["Cout"]) == (128, 64, 128) for c in cat) and {c["hw"] for c in cat} == {(8, 8), (12, 8), (16, 16)}
    att = [c for c in R.CASES if c["kind"] == "vattn"]
    assert {(c["C"], c["hw"]) for c in att} >= {(64, (12, 8)), (128, (16, 16))} and any(c["qk"] == 3.0 for c in att)
    assert all(c["hw"] == (8, 6) for c in R.CASES if c["kind"] in ("unet_up", "vup"))
    assert all(c["hw"] == (15, 13) for c in R.CASES if c["kind"] == "vdown") and all(c["hw"] == (16, 16) for c in R.CASES if c["kind"] == "unet_down")
    assert {c["recipe"] for c in R.CASES} == {"unit", "offset", "flat", "hole"}
    assert [c["kind"] for c in R.CASES if c["recipe"] == "hole"] == ["venc"]
    assert {c["Cout"] for c in R.CASES if c["kind"] == "venc"} == {8} and {c["Cout"] for c in R.CASES if c["kind"] == "vdec"} == {3}
    for c in R.CASES:                                                  # distinct embedding rows per sample; the hole is exactly zero
        inp = R.refs(c["id"]).inp
        if c["kind"] == "res":
            e = inp["emb_out"]
            assert not torch.equal(e[0], e[1]) and not torch.equal(e[1], e[2]) and not torch.equal(e[0], e[2])
            assert float(R.refs(c["id"]).sd["out_layers.3.weight"].abs().sum()) > 0
        if c["recipe"] == "hole":
            assert bool((inp["x"] == 0).all(-1).any()) and bool((inp["x"] != 0).any())
    assert len(set(IDS)) == len(IDS)
    for name, (kinds, forms, _) in R.FAULTS.items():
        assert any(R.fault_applies(name, c) for c in R.CASES), name


def test_flat_cases_make_eps_matter():
    """The recipe does what it is for: at every norm an eps fault names, swapping eps on a `flat` / `hole` case moves the block's output
    by more than 1e-2 rel-L2 (on a unit-variance map: about 5e-6)."""
    for name in EPS_FAULTS:
        for c in R.CASES:
            if not R.fault_applies(name, c) or c["recipe"] not in ("flat", "hole"):
                continue
            r = R.refs(c["id"])
            shift = R.rel_l2(r.emu(fault=name), r.ref64())
            assert shift > 1e-2, (name, c["id"], shift)
