"""The gate of the exemplar-conditioning chain (tests/clipref.py) on the CPU: plain() pinned to the oracle, the pack restatements pinned bit
for bit to what the modules' _pack() holds, the emulation under its own verdict on every case test_clipgate_gpu.py runs (forward, reverse
and eight seeded permutation orders), every planted wiring fault rejected on every case it applies to, and the one-site faults that the
verdict rejects while its rel-L2 terms alone accept them - the gap the per-element gate closes.

Why the one-site faults: the rel-L2 term holds the result to 1.5 x the emulation's own error, so a fault spread over every row is as
visible to it as to the peak term.  What it cannot see is a fault whose energy is small because it sits at ONE place - one key of one
query in one head, one bias element on one row - although the element itself is off by ten and more times the spread of two summation
orders.  Each of those is asserted here on the cases clipref.GAP_FAULTS names."""
import pytest
import torch

import clipref as R
from oracle_loader import O

IDS = [c["id"] for c in R.CASES]
PERMUTATIONS = tuple(range(1, 9))


def _oracle_layer(sd, x, Bn, N, heads):
    """One encoder layer from the oracle's primitives, as the loop body of O.clip_vision_pooled states it."""
    d = x.shape[-1]
    x = x.reshape(Bn, N, d)
    h = O.layer_norm(x, sd, "layer_norm1", R.EPS)
    q, k, v = (O.linear(h, sd, "self_attn." + n).reshape(Bn, N, heads, d // heads).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
    w = (q @ k.transpose(-1, -2) * (d // heads) ** -0.5).softmax(-1)
    x = x + O.linear((w @ v).transpose(1, 2).reshape(Bn, N, d), sd, "self_attn.out_proj")
    h = O.linear(O.layer_norm(x, sd, "layer_norm2", R.EPS), sd, "mlp.fc1")
    return (x + O.linear(h * torch.sigmoid(1.702 * h), sd, "mlp.fc2")).reshape(Bn * N, d)


def _oracle(c, sd, inp):
    ccfg, mcfg = R.oracle_cfgs(c)
    if c["kind"] == "layer":
        return _oracle_layer(sd, inp["x"].float(), c["B"], c["N"], c["heads"])
    if c["kind"] == "tower":
        return O.clip_vision_pooled(sd, inp["pixels"], ccfg, prefix="")
    if c["kind"] == "mapper":
        return O.layer_norm(O.xf_mapper(sd, inp["z"].float().unsqueeze(1), mcfg, "mapper."), sd, "final_ln")[:, 0]
    return O.learned_conditioning(sd, inp["pixels"], ccfg, mcfg)


@pytest.mark.parametrize("cid", IDS)
def test_plain_is_the_oracles_stage(cid):
    """plain() (fp64) against the oracle (fp32): rel-L2 <= 1e-5; and ref64 stays within the weight roundings of it."""
    r = R.refs(cid)
    want, got = _oracle(r.c, r.sd, r.inp), r.plain()["out"]
    assert got.shape == want.shape, (got.shape, want.shape)
    rel = R.rel_l2(want, got)
    assert rel <= 1e-5, (cid, rel)
    if r.c["recipe"] in ("unit", "outlier"):
        for n in r.names():
            assert R.rel_l2(r.ref64()[n], r.plain()[n]) <= 1e-3, (cid, n)


def test_the_towers_layer_is_the_layer_cases_layer():
    """The oracle pins the tower's pooled output only; the streams the tower cases gate come from the same _layer the layer cases run, and
    the pooled output is post_layernorm of the last stream's CLS rows."""
    r = R.refs("tower-256h4-img56x2-unit")
    c, sd = r.c, r.sd
    for mode in ("plain", "ref64"):
        outs = getattr(r, mode)()
        A = R._Arith(mode)
        again = R._layer(A, sd, "encoder.layers.1.", outs["stream0"], c["B"], c["N"], c["heads"])
        assert torch.equal(again, outs["stream1"])
        cls = outs["stream1"].reshape(c["B"], c["N"], -1)[:, 0]
        assert torch.equal(A.ln(cls, sd["post_layernorm.weight"], sd["post_layernorm.bias"]), outs["out"])


def test_pack_restatements_equal_the_modules_packs_bit_for_bit():
    """The values ref64 and the emulation use are what _EncoderLayer, _VisionTransformer, ResidualAttentionBlock and HipLinear pack."""
    from ldm.models.diffusion.ddpm import HipLinear
    from ldm.modules.encoders.modules import FrozenCLIPImageEmbedder
    c = R.case_by_id("cond-256h4-img56x2to96-outlier")
    sd = R.refs(c["id"]).sd
    ccfg = dict(hidden_size=c["hidden"], intermediate_size=c["mlp"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                image_size=c["image"], patch_size=c["patch"], layer_norm_eps=R.EPS)
    m = FrozenCLIPImageEmbedder(clip_config=ccfg, mapper_layers=c["layers"])
    pre = "cond_stage_model."
    res = m.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=False)
    assert not res.unexpected_keys and res.missing_keys == ["transformer.vision_model.embeddings.position_ids"], res
    vm, t = m.transformer.vision_model, pre + "transformer.vision_model."
    p = vm.pk()
    assert p.kp == R.KP and p.wpatch.dtype == torch.float16 and tuple(p.wpatch.shape) == (c["hidden"], R.KP)
    assert torch.equal(p.wpatch, R.packed_patch(sd[t + "embeddings.patch_embedding.weight"]))
    assert bool((p.wpatch[:, 3 * c["patch"] ** 2:] == 0).all())
    assert torch.equal(p.cls, R.packed_embedding(sd[t + "embeddings.class_embedding"])) and p.cls.dtype == torch.float16
    assert torch.equal(p.pos, R.packed_embedding(sd[t + "embeddings.position_embedding.weight"])) and p.pos.dtype == torch.float16
    for have, name in ((p.gpre, "pre_layrnorm.weight"), (p.bpre, "pre_layrnorm.bias"), (p.gpost, "post_layernorm.weight"), (p.bpost, "post_layernorm.bias")):
        assert have.dtype == torch.float32 and torch.equal(have, R.packed_norm(sd[t + name])), name
    for i, layer in enumerate(vm.encoder.layers):
        q, lp = f"{t}encoder.layers.{i}.", layer.pk()
        W = lambda n: R.packed_linear(sd[q + n + ".weight"])      # noqa: E731
        Bv = lambda n: R.packed_norm(sd[q + n + ".bias"])         # noqa: E731
        assert torch.equal(lp.wqk, torch.cat([W("self_attn.q_proj"), W("self_attn.k_proj")], 0)) and lp.wqk.dtype == torch.float16
        assert torch.equal(lp.bqk, torch.cat([Bv("self_attn.q_proj"), Bv("self_attn.k_proj")], 0)) and lp.bqk.dtype == torch.float32
        for have, n in ((lp.wv, "self_attn.v_proj"), (lp.wo, "self_attn.out_proj"), (lp.w1, "mlp.fc1"), (lp.w2, "mlp.fc2")):
            assert torch.equal(have, W(n)), n
        for have, n in ((lp.bv, "self_attn.v_proj"), (lp.bo, "self_attn.out_proj"), (lp.c1, "mlp.fc1"), (lp.c2, "mlp.fc2")):
            assert have.dtype == torch.float32 and torch.equal(have, Bv(n)), n
        for have, n in ((lp.g1, "layer_norm1.weight"), (lp.b1, "layer_norm1.bias"), (lp.g2, "layer_norm2.weight"), (lp.b2, "layer_norm2.bias")):
            assert have.dtype == torch.float32 and torch.equal(have, R.packed_norm(sd[q + n])), n
        assert (layer.heads, layer.eps) == (c["heads"], R.EPS)
    w = c["hidden"]
    for i, blk in enumerate(m.mapper.resblocks):
        q, bp = f"{pre}mapper.resblocks.{i}.", blk.pk()
        assert torch.equal(bp.wv, R.packed_linear(sd[q + "attn.c_qkv.weight"][2 * w:])) and torch.equal(bp.bv, R.packed_norm(sd[q + "attn.c_qkv.bias"][2 * w:]))
        for have, n in ((bp.wp, "attn.c_proj"), (bp.wf, "mlp.c_fc"), (bp.wo, "mlp.c_proj")):
            assert have.dtype == torch.float16 and torch.equal(have, R.packed_linear(sd[q + n + ".weight"])), n
        for have, n in ((bp.bp, "attn.c_proj"), (bp.bf, "mlp.c_fc"), (bp.bo, "mlp.c_proj")):
            assert have.dtype == torch.float32 and torch.equal(have, R.packed_norm(sd[q + n + ".bias"])), n
        for have, n in ((bp.g1, "ln_1.weight"), (bp.b1, "ln_1.bias"), (bp.g2, "ln_2.weight"), (bp.b2, "ln_2.bias")):
            assert torch.equal(have, R.packed_norm(sd[q + n])), n
        assert bp.eps == R.EPS
    assert m.final_ln.eps == R.EPS and torch.equal(m.final_ln.weight.float(), R.packed_norm(sd[pre + "final_ln.weight"]))
    lin = HipLinear(c["hidden"], R.PROJ)
    lin.load_state_dict({"weight": sd["proj_out.weight"], "bias": sd["proj_out.bias"]})
    pw, pb = lin._packed()
    assert torch.equal(pw, R.packed_linear(sd["proj_out.weight"])) and torch.equal(pb, R.packed_norm(sd["proj_out.bias"]))
    # the values the arithmetic takes ARE the packed values
    A = R._Arith("ref64")
    assert torch.equal(A.w(sd[t + "embeddings.patch_embedding.weight"]).reshape(c["hidden"], -1), p.wpatch[:, :3 * c["patch"] ** 2].double())
    assert torch.equal(A.w(sd[t + "embeddings.position_embedding.weight"]), p.pos.double())
    assert torch.equal(A.w(sd["proj_out.weight"]), pw.double())


@pytest.mark.parametrize("cid", IDS)
def test_emulation_passes_its_own_verdict_in_ten_orders(cid):
    """Forward, reverse and eight seeded permutations of every K and every key tile: each is a valid fp32 order, and the verdict must
    accept every one (what PEAK = 2 and the choice of the set E is taken over are for)."""
    r = R.refs(cid)
    for order in (False, True) + PERMUTATIONS:
        ok, text = r.verdict(r.emu(order))
        print(f"clipgate cpu  {cid:34s} order {order!s:5s}:\n{text}")
        assert ok, (cid, order, text)


@pytest.mark.parametrize("name", list(R.FAULTS) + list(R.GAP_FAULTS))
def test_fault_is_rejected_on_every_case_it_applies_to(name):
    seen = 0
    for c in R.CASES:
        if R.fault_applies(name, c):
            r = R.refs(c["id"])
            ok, text = r.verdict(r.emu(fault=name))
            assert not ok, f"fault '{name}' is accepted on {c['id']}:\n{text}"
            seen += 1
            print(f"clipgate cpu  fault '{name}' rejected on {c['id']}: {text.splitlines()[-1]}")
    assert seen, name


@pytest.mark.parametrize("name", list(R.GAP_FAULTS))
def test_the_rel_l2_terms_accept_what_the_verdict_rejects(name):
    """One wrong key, bias or row: the verdict without its peak term accepts the run, the verdict rejects it."""
    cids, what = R.GAP_FAULTS[name]
    for cid in cids:
        r = R.refs(cid)
        bad = r.emu(fault=name)
        ok, text = r.verdict(bad)
        assert r.rel_l2_terms_accept(bad), (name, cid)
        assert not ok and "peak" in text.split("REJECTED:")[-1], (name, cid, text)
        ref = r.ref64()["out"]
        wrong = int(((bad["out"].double() - r.emu()["out"].double()).abs() > 0).sum())
        print(f"clipgate cpu  gap '{name}' ({what}) on {cid}: {wrong} of {ref.numel()} elements differ from the clean emulation; {text}")
    assert len(R.GAP_FAULTS) >= 6


def test_one_token_attention_is_c_proj_of_v():
    """The algebraic claim of ldm/modules/encoders/xf.py in fp64: multi-head attention over ONE token (q and k scaled by ch^-1/4 each,
    softmax over the keys) has weight exactly 1, so with heads = 1 it equals c_proj(V), V = rows 2w:3w of c_qkv.  With heads > 1 the same
    identity holds per head, but V is then each head's last third of c_qkv, not rows 2w:3w - which is why ResidualAttentionBlock takes
    heads = 1 only."""
    g = torch.Generator().manual_seed(5)
    w, bs = 64, 3
    x = torch.randn(bs, 1, w, generator=g, dtype=torch.float64) * 3
    Wqkv, bqkv = torch.randn(3 * w, w, generator=g, dtype=torch.float64), torch.randn(3 * w, generator=g, dtype=torch.float64)
    Wp, bp = torch.randn(w, w, generator=g, dtype=torch.float64), torch.randn(w, generator=g, dtype=torch.float64)

    def full(heads):
        ch = w // heads
        qkv = (x @ Wqkv.t() + bqkv).reshape(bs, 1, heads, 3 * ch)
        q, k, v = qkv.split(ch, -1)
        s = ch ** -0.25
        weight = torch.softmax(torch.einsum("bthc,bshc->bhts", q * s, k * s), -1)
        assert torch.equal(weight, torch.ones_like(weight))
        return torch.einsum("bhts,bshc->bthc", weight, v).reshape(bs, 1, w) @ Wp.t() + bp, v.reshape(bs, 1, w)
    out, v = full(1)
    short = (x @ Wqkv[2 * w:].t() + bqkv[2 * w:]) @ Wp.t() + bp
    assert torch.equal(v, x @ Wqkv[2 * w:].t() + bqkv[2 * w:]) and torch.equal(out, short)
    out4, v4 = full(4)
    assert torch.equal(out4, v4 @ Wp.t() + bp) and R.rel_l2(out4, short) > 0.5
    from ldm.modules.encoders.xf import ResidualAttentionBlock
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError):
        ResidualAttentionBlock(1, w, 4)
    # and the emulation's mapper block IS that shortcut: plain() of the mapper case equals the full attention written out
    r = R.refs("mapper-256x2-unit")
    z, sd, wd = r.inp["z"].double(), r.sd, r.c["hidden"]
    for i in range(r.c["layers"]):
        q = f"mapper.resblocks.{i}."
        ln = lambda t, n: torch.nn.functional.layer_norm(t, (wd,), sd[q + n + ".weight"].double(), sd[q + n + ".bias"].double(), R.EPS)      # noqa: E731
        qkv = ln(z, "ln_1") @ sd[q + "attn.c_qkv.weight"].double().t() + sd[q + "attn.c_qkv.bias"].double()
        qq, kk, vv = qkv.split(wd, -1)
        weight = torch.softmax((qq * wd ** -0.25 * kk * wd ** -0.25).sum(-1, keepdim=True), -1)
        z = z + (weight * vv) @ sd[q + "attn.c_proj.weight"].double().t() + sd[q + "attn.c_proj.bias"].double()
        hh = ln(z, "ln_2") @ sd[q + "mlp.c_fc.weight"].double().t() + sd[q + "mlp.c_fc.bias"].double()
        z = z + torch.nn.functional.gelu(hh) @ sd[q + "mlp.c_proj.weight"].double().t() + sd[q + "mlp.c_proj.bias"].double()
    z = torch.nn.functional.layer_norm(z, (wd,), sd["final_ln.weight"].double(), sd["final_ln.bias"].double(), R.EPS)
    assert R.rel_l2(r.plain()["out"], z) <= 1e-13


def test_cases_hold_what_the_gate_names():
    by = lambda kind: [c for c in R.CASES if c["kind"] == kind]      # noqa: E731
    assert {c["kind"] for c in R.CASES} == set(R.KINDS) and all(c["B"] == 3 for c in R.CASES) and len(set(IDS)) == len(IDS)
    lay = by("layer")
    assert {(c["hidden"], c["heads"], c["mlp"], c["N"]) for c in lay} == {(256, 4, 1024, 17), (256, 4, 1024, 65), (128, 4, 512, 65)}
    for n in (17, 65):
        assert {c["recipe"] for c in lay if c["hidden"] == 256 and c["N"] == n} == {"unit", "outlier", "peaked", "flat"}
    assert (17 + 7) // 8 * 8 == 24 and 17 % 8 == 1 and 65 == 64 + 1                      # V^T padded to 24; one full key tile plus one key
    assert {(c["image"], c["N"]) for c in by("tower")} == {(56, 17), (112, 65)}
    assert all((c["hidden"], c["heads"], c["layers"], c["patch"]) == (256, 4, 2, 14) for c in by("tower") + by("cond"))
    assert all((c["hidden"], c["layers"]) == (256, 2) for c in by("mapper")) and {c["recipe"] for c in by("mapper")} == {"unit", "outlier", "flat"}
    assert all(c["image"] == 56 for c in by("cond")) and R.PROJ == 96 and R.KP == 592
    assert {c["recipe"] for c in R.CASES} == {"unit", "outlier", "peaked", "flat"}
    assert {c["kind"] for c in R.CASES if c["recipe"] == "flat"} == {"layer", "mapper"}
    assert {c["kind"] for c in R.CASES if c["recipe"] == "peaked"} == {"layer", "tower"}
    import accgate as ag
    assert ag.instantiation(3, 4, 65, 65, 64) == "64,1" and ag.instantiation(3, 4, 65, 65, 32) == "32,1"
    from test_model_gpu import BLOCK_TOL, FWD_TOL
    assert (R.BLOCK_TOL, R.FWD_TOL) == (BLOCK_TOL, FWD_TOL) == (2e-3, 4e-3)
    import convref
    assert (R.PEAK, R.REL_L2_FACTOR) == (convref.PEAK, convref.REL_L2_FACTOR) == (2.0, 1.5)
    for name in list(R.FAULTS) + list(R.GAP_FAULTS):
        assert any(R.fault_applies(name, c) for c in R.CASES), name
    for c in R.CASES:                                                  # the recipes do what they say
        r = R.refs(c["id"])
        if c["recipe"] == "outlier":
            a, b = R.outlier_channels(c)
            t = r.inp.get("x", r.inp.get("z"))
            if t is None:
                t = r.sd[[k for k in r.sd if k.endswith("position_embedding.weight")][0]].half()
            assert abs(float(t[:, a].float().mean()) - 32) < 1 and abs(float(t[:, b].float().mean()) + 32) < 1
        if "pixels" in r.inp:                                          # what preprocessing sends: bytes through CLIP's normalisation
            px = r.inp["pixels"]
            back = px * torch.tensor(R.CLIP_STD).view(1, 3, 1, 1) + torch.tensor(R.CLIP_MEAN).view(1, 3, 1, 1)
            assert px.dtype == torch.float32 and float((back * 255 - (back * 255).round()).abs().max()) < 1e-3
            assert not torch.equal(px[0], px[1]) and not torch.equal(px[1], px[2])


def test_flat_cases_make_eps_matter():
    """On the flat mapper case final_ln's eps decides rstd: 1e-6 for 1e-5 moves the output by more than 1e-2 rel-L2 (on the unit case by
    about 5e-6, which no gate sees - the eps fault applies to `flat` alone)."""
    r = R.refs("mapper-256x2-flat")
    assert R.rel_l2(r.emu(fault="final_ln eps 1e-6")["out"], r.ref64()["out"]) > 1e-2
    u = R.refs("mapper-256x2-unit")
    moved = R._run(R._Arith("emu", fault="final_ln eps 1e-6"), u.c, u.sd, u.inp)["out"].half()
    assert R.rel_l2(moved, u.emu()["out"].double()) < 1e-4 and u.verdict({"out": moved})[0]
    for cid in ("layer-256h4-N17-flat", "layer-256h4-N65-flat"):       # and the flat layer's norms meet rows whose variance is near eps
        f = R.refs(cid)
        assert float(f.inp["x"].float().var(-1).max()) < 2 * R.EPS and float(f.ref64()["out"].var(-1).max()) < 20 * R.EPS
