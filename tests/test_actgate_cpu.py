"""CPU half of the activation gate (tests/actref.py): the operand builders are exact, the table is complete, the tile lists follow from the
tile geometry, the plain fp32 restatement of the kernel arithmetic passes the per-element bound on every case's operands, and the gate
rejects the mutations the whole-tensor _close limit of test_gemm_epilogue lets through.  No kernel runs here."""
import pytest
import torch

import accgate
import actref
import tilecheck

OPERANDS = actref.all_operand_sets()


def _ratio(got, want, bound):
    return tilecheck.compare(got, want, bound).ratio


def test_table_covers_every_finite_fp16_up_to_24():
    t = actref.table16()
    assert t.numel() == 39938
    every = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.float16)
    every = every[torch.isfinite(every) & (every.float().abs() <= 24.0)]
    assert set(t.view(torch.int16).tolist()) == set(every.view(torch.int16).tolist())       # by bit pattern: +0 and -0, every subnormal
    assert actref.table8().numel() == 254
    # the plain-bias launch of every tile height holds each of them as a pre-activation (bit for bit: W itself, alpha 1, bias +0)
    for bm in (64, 128, 256):
        o = actref.dense_operands(bm, "bias")
        assert o["M"] >= o["K"] and o["alpha"] == 1.0 and not o["bias"].any() and not torch.signbit(o["bias"]).any()
        assert set(o["W"].view(torch.int16).view(-1).tolist()) == set(t.view(torch.int16).tolist())
        g = actref.dense_operands(bm, "bias", True)
        assert set(g["W"][1::2].contiguous().view(torch.int16).view(-1).tolist()) == set(t.view(torch.int16).tolist())      # the gate columns
        assert set(g["W"][0::2].float().reshape(-1).tolist()) == set(actref.VALUE_SET)
    for bm in (64, 128):
        assert set(actref.f8_operands(bm)["w8"].view(-1).tolist()) == set(actref.table8().tolist())


def test_tile_lists_follow_from_the_geometry():
    """ARMS = TM * TN * 4 <= 96 accumulator registers (igemm_kernel.h): a tile added to kTiles changes these lists, and the GPU sweep with them."""
    assert actref.dense_tiles(True) == [1, 2, 3, 4, 5, 6, 8, 9, 15, 16, 17, 18, 21]
    assert actref.dense_tiles(False) == [0, 7]
    assert actref.f8_tiles() == [3, 4, 6, 8, 9]
    assert [actref.acc_regs(t) for t in (0, 7)] == [128, 160]
    assert [(t[0], t[1]) for t in actref.tiles()][:10] == [(256, 256), (256, 128), (128, 256), (128, 128), (128, 64), (64, 128), (64, 64), (256, 320),
                                                             (128, 320), (128, 160)]


@pytest.mark.parametrize("label,o", OPERANDS, ids=[l for l, _ in OPERANDS])
def test_operands_are_exact(label, o):
    actref.assert_exact(o)
    M, K = o["M"], o["K"]
    if "A" in o:                                                     # the product the kernel forms IS pre: one-hot rows
        assert torch.equal(o["A"].double() @ o["W"].double().t(), o["W"].double()[:, torch.arange(M) % K].t())
        assert (o["A"].float().sum(1) == 1).all()
    else:
        a = o["a8"].view(torch.float8_e4m3fn).double()
        assert torch.equal(a @ o["Wv"].double().t(), o["Wv"].double()[:, torch.arange(M) % K].t())


def test_slopes_and_fit_constant():
    """max |act'| on an fp64 grid (step 2^-10 over [-24, 24]) under ACT_DMAX; the GELU fit in exact (fp64) arithmetic within GELU_FIT."""
    x = torch.arange(-24 * 1024, 24 * 1024 + 1, dtype=torch.float64) / 1024
    h = 2.0 ** -20
    for act, stated in ((1, 1.0998), (2, 1.1290), (3, 1.0998)):
        d = ((actref.act64(x + h, act) - actref.act64(x - h, act)) / (2 * h)).abs().max().item()
        print(f"max |{actref.ACT_NAME[act]}'| = {d:.5f}")
        assert abs(d - stated) < 2e-4 and d <= actref.ACT_DMAX[act]
    for xs in (x, actref.table16().double()):
        u = xs.abs()
        r, _ = actref._gelu_fit64(u)
        fit = xs.clamp_min(0) - u * torch.exp2(-(u * r + 1))
        err = (fit - actref.act64(xs, 2)).abs().max().item()
        print(f"GELU fit in fp64: max |error| = {err:.3e}")
        assert err <= tilecheck.GELU_FIT


def test_activation_term_alone_on_the_table():
    """Before the fp16 store: |fp32 restatement - fp64| within the activation term on every table value."""
    x = actref.table16().float()
    for act in (1, 2, 3):
        r = ((actref.act_f32(x, act).double() - actref.act64(x, act)).abs() / actref.act_term(x, act)).max().item()
        print(f"{actref.ACT_NAME[act]}: activation term alone, worst ratio {r:.3f}")
        assert r < 1.0


def test_emulation_passes_on_every_case():
    worst = {}
    for label, o in OPERANDS:
        acts = (4,) if "geglu" in label else (1, 2, 3)
        for act in acts:
            for resid in (False, True) if act != 4 else (False,):
                want, bound = actref.expect_exact(o["pre"], act, o["resid"] if resid else None)
                r = _ratio(actref.emulate(o, act, resid=resid), want, bound)
                assert r < 1.0, (label, act, resid, r)
                worst[act] = max(worst.get(act, 0.0), r)
    for act, r in sorted(worst.items()):
        print(f"{actref.ACT_NAME[act]}: emulation, worst |got - want| / bound = {r:.4f}")
    assert set(worst) == {1, 2, 3, 4}


@pytest.mark.parametrize("mutation", actref.MUTATIONS)
def test_gate_rejects_mutation(mutation):
    """Each mutation is outside the per-element bound.  The first four pass the whole-tensor _close limit of test_gemm_epilogue (the gap this
    gate closes); the two wiring mutations are errors of order one, which _close rejects as well - recorded, not a gap."""
    act = actref.MUTATION_ACT[mutation]
    table_mutation = mutation in ("tanh_gelu", "quick_1p7", "silu_clamp")
    o = actref.dense_operands(128, "bias" if table_mutation else "rv_half")
    resid = mutation == "resid_before_act"
    want, bound = actref.expect_exact(o["pre"], act, o["resid"] if resid else None)
    assert _ratio(actref.emulate(o, act, resid=resid), want, bound) < 1.0
    got = actref.emulate(o, act, resid=resid, mutation=mutation, bn=64)
    rep = tilecheck.compare(got, want, bound, mutation)
    ok, err, lim = accgate.close_verdict(got, want, actref.CLOSE_EPILOGUE)
    print(f"{rep}; _close: max|d| {err:.3e} vs limit {lim:.3e} -> {'accepted' if ok else 'rejected'}")
    assert rep.ratio > 1.0, str(rep)
    assert ok == (mutation not in ("skip_last_column_tile", "resid_before_act")), (mutation, err, lim)


@pytest.mark.parametrize("act", [1, 2, 3])
def test_expect_carries_the_activation(act):
    """tilecheck.expect(act = 1 / 2 / 3): with an exact product the bound is actref's exact one; with accumulation noise it grows by the slope
    times that noise, and an fp32 evaluation of a random GEMM epilogue stays inside it while another activation does not."""
    o = actref.dense_operands(128, "rv48")
    M, K = o["M"], o["K"]
    acc = o["W"].double()[:, torch.arange(M) % K].t()
    rv = o["rowvec"].double()[torch.arange(M) // o["group_rows"]]
    al = torch.full((o["N"],), o["alpha"], dtype=torch.float64)
    want, bound = tilecheck.expect(acc, torch.zeros_like(acc), K, alpha=al, bias=o["bias"].double(), rowvec=rv, act=act, resid=o["resid"].double())
    w0, b0 = actref.expect_exact(o["pre"], act, o["resid"])
    assert torch.equal(want, w0) and (bound >= b0 - tilecheck.U32 * want.abs() - 1e-18).all() and (bound <= b0 * 1.001 + 16 * tilecheck.U32 * (o["pre"].abs() + 4)).all()
    g = torch.Generator().manual_seed(act)
    A, W = torch.randn(96, 256, generator=g).half(), (torch.randn(72, 256, generator=g) * (3.0 / 16)).half()
    bias = torch.randn(72, generator=g)
    acc, S = A.double() @ W.double().t(), A.double().abs() @ W.double().abs().t()
    want, bound = tilecheck.expect(acc, S, 256, bias=bias.double(), act=act)
    pre32 = A.float() @ W.float().t() + bias
    assert _ratio(actref.act_f32(pre32, act).half(), want, bound) < 1.0
    assert _ratio(actref.act_f32(pre32, act % 3 + 1).half(), want, bound) > 1.0
    assert want.abs().max() > 8


def _stand_ins(monkeypatch):
    """ops.gemm(ln=...) / ops.conv3x3 / ops.row_stats replaced by the plain fp32 restatement, so that tilecheck's own builders and references
    run here on CPU tensors exactly as test_actgate_gpu.py drives them on the device."""
    import torch.nn.functional as F
    from pbe_amd import ops

    def gemm(a, w, bias, act=0, ln=None, **kw):
        x = a.float()
        mean = x.mean(1, keepdim=True)
        rstd = torch.rsqrt(((x * x).mean(1, keepdim=True) - mean * mean).clamp_min(0) + ln[2])
        pre = rstd * (x @ w.float().t()) + ((-mean * rstd) * ln[1][None, :] + bias[None, :])         # the fold's association (stage(), EXL)
        return actref.act_f32(pre, act).half()

    def conv3x3(x, wp, bias, rowvec=None, resid=None, act=0, **kw):
        Co, Ci = wp.shape[0], wp.shape[1] // 9
        w = wp.float().view(Co, Ci // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(Co, Ci, 3, 3)     # pack_conv3x3 undone
        y = F.conv2d(x.float().permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1) + (bias[None, :] + rowvec.float())[:, None, None, :]
        return (actref.act_f32(y, act).half().float() + resid.float()).half()
    monkeypatch.setattr(ops, "row_stats", lambda a: a)
    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "conv3x3", conv3x3)


@pytest.mark.parametrize("act", [1, 2, 3])
def test_random_operand_cases_pass_emulated(monkeypatch, act):
    """The LayerNorm-fold and conv cases of test_actgate_gpu.py with the fp32 restatement in the kernel's place: inside the bound with the
    right activation, outside it with another one; |pre| reaches 10."""
    _stand_ins(monkeypatch)
    cpu = torch.device("cpu")
    case, other = actref.ln_case(3, act), actref.ln_case(3, act % 3 + 1)
    rows = tilecheck.gemm_rows(case.M, 128, tilecheck.seed_of(case.key))
    got, want, bound, labels = tilecheck.reference_gemm(case, tilecheck.run_gemm(case, cpu), [(0, rows)])
    rep = tilecheck.compare(got, want, bound, f"ln-fold act {act}", labels)
    print(rep)
    assert rep.ratio < 1.0 and want.abs().max() >= 10
    wrong = tilecheck.run_gemm(other, cpu)["out"][rows]
    assert tilecheck.compare(wrong, want, bound).ratio > 1.0
    case, other = actref.conv_case(11, 2, act), actref.conv_case(11, 2, act % 3 + 1)
    sel = [(b, oy) for b in range(case.B) for oy in range(case.Ho)]
    got, want, bound, labels = tilecheck.reference_conv(case, tilecheck.run_conv(case, cpu), sel)
    rep = tilecheck.compare(got, want, bound, f"conv act {act}", labels)
    print(rep)
    assert rep.ratio < 1.0 and want.abs().max() >= 10
    wrong = torch.cat([tilecheck.run_conv(other, cpu)["out"][b, oy] for b, oy in sel])
    assert tilecheck.compare(wrong, want, bound).ratio > 1.0
