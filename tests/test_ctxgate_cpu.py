"""The per-element gate of the multi-token cross-attention kernel (tests/ctxgate.py) judged on the CPU, without a GPU: the emulation of
the kernel's arithmetic passes it on every case tests/test_ctxgate_gpu.py launches, in three summation orders of both MFMA sums; the
exact pins are exact; and a list of faults planted in the emulation is rejected wherever each fault applies.  Run with -s for the fault
table (which gate rejects what) and the largest share of the bound the emulation reaches.

The faults (ctxgate.emulate, ctxgate.applies):
  eps0, eps1e-6          eps 0 / GroupNorm's 1e-6 in place of 1e-5.  Must be rejected on `flat` (variance about eps: eps decides rstd); on `unit`
                         every variance is near 1 and the old verdict accepts both - recorded, asserted.
  w16_first              the weights rounded to fp16 BEFORE normalising (and again after).  One more half-ulp on each weight: below anything
                         Y can show under its own store rounding, so it must be rejected where the map is the weight itself (H = 1), by
                         the map's per-element term; `peaked` is left out (the weights are one-hot: 1 and 0 round to themselves), and
                         so is `far` (|x| is 16 std, so the first MFMA's own allowance, ACC_C U32 sqrt(C) sum|x kq| rstd = 6e-4 log2
                         units = 4e-4 relative, is as large as the half-ulp 2.4e-4 .. 4.9e-4 being looked for).
  drop_colsum            the mean * colsum term of the fold left out.  Everywhere but `peaked` (a leader 32 log2 units ahead keeps the
                         weights one-hot under any shift of a few units).
  clamp_early            the table row clamped at tokens - 2: a sample's last row reads the row before.  On the row-weight pins, bit for bit.
  block2_from_block0     columns 64 .. of S taken from columns 0 .. (the wave that owns blocks 0 and 2 storing one accumulator twice).  NJ = 3
                         cases where block 2 holds a live token, but `peaked`.
  drop_kbias_column      kbias of one live column (the largest in size) of the last sample zeroed.  Everywhere but `peaked`.
  log2w_by_head          log2w added per column c / Nk instead of c % Nk.  Every weighted case.
  map_div_nk             the head mean of the map divided by Nk instead of H.  Every case with H != Nk (the row sums give it away).
"""
import pytest
import torch

import ctxgate as cg
import ctxref as cr
import kbiasref as kr
import regionref as rr

CASES = [(s, r) for s in cg.NEW_SHAPES + [cg.VIEW_SHAPE] for r in cg.RECIPES]
Y_FAULTS = {"eps0": dict(eps=0.0), "eps1e-6": dict(eps=1e-6), "w16_first": dict(fault="w16_first"), "drop_colsum": dict(fault="drop_colsum"),
            "block2_from_block0": dict(fault="block2_from_block0"), "drop_kbias_column": dict(fault="drop_kbias_column"),
            "log2w_by_head": dict(fault="log2w_by_head"), "map_div_nk": dict(fault="map_div_nk")}


def _case_id(c):
    return f"{cg.shape_id(c[0])}-{c[1]}"


@pytest.fixture(scope="module")
def shares():
    got = {}
    yield got
    if got:
        k = max(got, key=got.get)
        print(f"\nlargest share of the Y bound the emulation reaches: {got[k]:.3f} ({k}; {len(got)} cases x orders)")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_emulation_passes_in_every_summation_order(case, shares):
    """Forward, reverse and a seeded permutation of both MFMA sums, every form, Y and map."""
    shape, recipe = case
    o = cg.operands(shape, recipe)
    for form in cg.FORMS:
        table, _ = cg.form_table(shape, recipe, form)
        ref = cg.reference(o, table)
        emu = cg.emulate(o, table)
        for order in cg.ORDERS:
            y, m = cg.emulate(o, table, order=order)
            v = cg.verdict(y, o, table, ref=ref, emu=emu[0])
            ok, ratio, where, text = cg.map_verdict(m, o, table, ref=ref, emu=emu[1])
            shares[f"{_case_id(case)} {form} {order}"] = v.ratio
            assert v.ok, f"{form} {order}: {v}"
            assert ok, f"{form} {order}: {text}"


def _old_list_cases():
    """The operands of the four older GPU files' kernel tests: (name, Operands, table)."""
    for B, N, C, H, Nk, parts in cr.KERNEL_SHAPES:
        yield f"plain {B}-{N}-{C}-{H}-{Nk}-{parts}", cr.random_operands(B, N, C, H, Nk, parts, seed=1), None
    B, N, C, H, Nk, parts = cr.LARGE_LOGITS_SHAPE
    yield "large logits", cr.random_operands(B, N, C, H, Nk, parts, seed=3, logit_scale=60.0), None
    for B, N, C, H, Nk, parts in kr.CTX_SHAPES:
        o = cr.random_operands(B, N, C, H, Nk, parts)
        lw = torch.log2(kr.ctx_weights(B, Nk, 11 + C)).float()
        yield f"weights {B}-{N}-{C}-{H}-{Nk}-{parts}", o, lw[:, None, :].expand(B, N, Nk).contiguous()
    for s in rr.SHAPES:
        yield "regions " + rr.shape_id(s), cr.random_operands(*s[:6]), rr.kernel_case(s)["table"].float()


def test_emulation_passes_on_the_older_lists(shares):
    for name, o, table in _old_list_cases():
        v = cg.verdict(cg.emulate(o, table, order="reverse")[0], o, table)
        shares[name] = v.ratio
        assert v.ok, f"{name}: {v}"


def test_emulation_passes_on_the_map_list(shares):
    """mapref.SHAPES in the three forms test_map_kernel_against_fp64_reference launches: Y and the map."""
    import mapref as mr
    for s in mr.SHAPES:
        B, N, C, H, Nk, parts = s
        o = cr.random_operands(B, N, C, H, Nk, parts)
        tables = {"plain": None, "weights": mr.weights_table(o, kr.ctx_weights(B, Nk, 11 + C)).float(), "regions": mr.region_case(s)["table"].float()}
        for form, table in tables.items():
            y, m = cg.emulate(o, table, order="permuted")
            v = cg.verdict(y, o, table)
            ok, ratio, where, text = cg.map_verdict(m, o, table)
            shares[f"map list {mr.shape_id(s)} {form}"] = v.ratio
            assert v.ok and ok, f"{mr.shape_id(s)} {form}: {v}; {text}"


def test_folded_weights_are_the_table_form():
    """What test_ctx_weights_gpu.py hands its gate - log2 w added to kbias through fp32, -inf included - is judged as the table form is."""
    B, N, C, H, Nk, parts = kr.CTX_SHAPES[1]
    o = cr.random_operands(B, N, C, H, Nk, parts)
    w = kr.ctx_weights(B, Nk, 11 + C)
    table = torch.log2(w).float()[:, None, :].expand(B, N, Nk).contiguous()
    y = cg.emulate(o, table)[0]
    a, b = cg.verdict(y, kr.fold_log2w(o, w, through_fp32=True)), cg.verdict(y, o, table)
    assert a.ok and b.ok and abs(a.ratio - b.ratio) < 1e-3, (str(a), str(b))


# ---- exact pins ------------------------------------------------------------------------------------------------------------------------
PINS = [(f, s) for f in cg.FORMS for s in cg.PIN_SHAPES[f]]


def test_pin_shapes_cover_what_the_issue_asks():
    for f in cg.FORMS:
        assert any((s[3] * s[4] + 31) // 32 == 3 for s in cg.PIN_SHAPES[f]) and any(s[1] % 64 for s in cg.PIN_SHAPES[f]), f


@pytest.mark.parametrize("pin", PINS, ids=lambda p: f"{p[0]}-{cg.shape_id(p[1])}")
def test_pins_are_exact(pin):
    """The expected Y is representable in fp16, the emulation gives its bits in every summation order, the fp64 reference rounds to
    them (it lies within 1e-11 of them), the map is exact; on the row-weight pins the token changes at every row and tile seam."""
    form, shape = pin
    o, table, lw, want, hot = cg.pin_case(form, shape)
    bits = want.half()
    assert torch.equal(bits.double(), want) and float(want.abs().max()) < 128
    ref = cg.reference(o, table)
    assert float((ref[0] - want).abs().max()) < 1e-11 and torch.equal(ref[0].half(), bits)
    assert float((ref[2] - hot).abs().max()) < 1e-14
    for order in cg.ORDERS:
        y, m = cg.emulate(o, table, order=order)
        assert torch.equal(y, bits), f"{order}: {int((y != bits).sum())} elements differ"
        assert torch.equal(m.double(), hot), order
    if form == "regions":
        B, N, Nk = shape[0], shape[1], shape[4]
        keep = torch.isfinite(table).float().argmax(-1)
        assert bool((torch.isfinite(table).sum(-1) == 1).all()) and bool((keep[:, 1:] != keep[:, :-1]).all())
        y, _ = cg.emulate(o, table, fault="clamp_early")
        wrong = (y != bits).any(1).view(B, N)
        assert bool(wrong[:, N - 1].all()) and not bool(wrong[:, :N - 1].any())      # rejected, and by the last row of every sample alone


# ---- the fault table -------------------------------------------------------------------------------------------------------------------
def test_planted_faults_are_rejected_where_they_apply():
    """Every fault on every case: the new gate must reject it wherever ctxgate.applies says it applies; what the old ctxref.verdict says
    is recorded.  The eps faults are accepted by the old verdict on every `unit` case and rejected by the new gate on every `flat` one."""
    tally = {f: dict(applies=0, new=0, old=0, cases=0, new_all=0) for f in Y_FAULTS}
    missed = []
    eps_unit_old, eps_flat_new = [], []
    for shape, recipe in CASES:
        o = cg.operands(shape, recipe)
        for form in cg.FORMS:
            table, lw = cg.form_table(shape, recipe, form)
            ref = cg.reference(o, table)
            emu = cg.emulate(o, table)
            for name, kw in Y_FAULTS.items():
                if name == "log2w_by_head" and form != "weights":
                    continue
                if name == "block2_from_block0" and cg.nj_of(shape) != 3:
                    continue
                y, m = cg.emulate(o, table, log2w=lw, **kw) if name == "log2w_by_head" else cg.emulate(o, table, **kw)
                v = cg.verdict(y, o, table, ref=ref, emu=emu[0])
                new_rej = not v.ok or not cg.map_verdict(m, o, table, ref=ref, emu=emu[1])[0]
                t = tally[name]
                t["cases"] += 1
                t["new_all"] += new_rej
                t["old"] += not v.old_ok
                if name in ("eps0", "eps1e-6") and recipe == "unit":
                    eps_unit_old.append(v.old_ok)
                if name in ("eps0", "eps1e-6") and recipe == "flat":
                    eps_flat_new.append(new_rej)
                if cg.applies(name, shape, recipe, form, table):
                    t["applies"] += 1
                    t["new"] += new_rej
                    if not new_rej:
                        missed.append(f"{name} on {cg.shape_id(shape)} {recipe} {form}: {v}")
    print("\nfault                 cases  applies  new gate rejects (where it applies / anywhere)  old verdict rejects (anywhere)")
    for name, t in tally.items():
        print(f"{name:22s}{t['cases']:5d}{t['applies']:9d}{t['new']:12d} /{t['new_all']:4d}{t['old']:40d}")
    assert not missed, "\n".join(missed)
    assert all(t["applies"] > 0 for t in tally.values())
    assert eps_unit_old and all(eps_unit_old), "the old verdict no longer accepts an eps fault on `unit`"
    assert eps_flat_new and all(eps_flat_new)
