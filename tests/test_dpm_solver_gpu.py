"""The DPM-Solver++(2M) sampler on the GPU: the update kernel pbe_dpmpp_update per element against fp64 (tests/dpmref.py: operands between
poison, outputs in sentinel arenas, the bound derived there) and against pbe_plms_update in its first-order form; the sampler on the narrow
model against the restatement of tests/dpmref.py over the oracle U-Net; the machinery it inherits from PLMSSampler._eps (HIP graphs, the
shared guidance prefix, regions, attribution maps) bit for bit; and the public surface (pipeline.inpaint(sampler="dpm"), --dpm_solver).

No test here claims a quality or convergence gain: on the name-seeded weights every sampler converges at first order
(tests/test_dpm_solver_cpu.py shows the order on an analytic model instead)."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import cases
import dpmref
import guard
import modelbuild as build
import regionref as rr
from oracle_loader import O
from test_model_gpu import SAMPLER_OPT_TOL, rel_l2, report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _coef(second):
    """A row of the 20-step table of the v1 schedule: second order (row 10) or first order (row 19, the first step of a run)."""
    from ldm.models.diffusion.dpm_solver import dpmpp_coefficients
    _, a, ap = O.ddim_parameters(O.schedule_buffers()["alphas_cumprod"], O.ddim_timesteps_uniform(20))
    return dpmpp_coefficients(a, ap, 2)[10 if second else 19].tolist()


def _operands(B, HW, dup, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(dup * B, HW, 4, generator=g).half(), torch.randn(B, 4, HW, generator=g) * 3.0, torch.randn(B, 4, HW, generator=g))


def _launch(dev, eps, ld, dup, cfg, x, x0_prev, coef, want_x0, misalign=False):
    """One raw pbe_dpmpp_update launch: eps [dup*B, HW, 4] embedded with leading dimension ld (channels 4 .. ld-1, the rows before and
    after: NaN), x / x0_prev embedded flat, outputs in sentinel arenas, checked untouched outside / fully written inside.
    misalign: the eps base 4 bytes off an 8-byte boundary (ld 8) - the kernel's per-element read path."""
    from pbe_amd import lib
    B, _, HW = x.shape
    if misalign:
        flat = torch.full((2 + dup * B * HW * ld,), float("nan"), dtype=torch.float16)
        flat[2:].view(dup * B * HW, ld)[:, :4] = eps.reshape(-1, 4)
        ev, _ = guard.embed(flat, device=dev)
        eptr = ev.data_ptr() + 4
        assert eptr % 8 == 4
    else:
        ev, _ = guard.embed(eps.reshape(-1, 4), col_pad=ld - 4, device=dev)
        assert ev.stride(0) == ld
        eptr = ev.data_ptr()
    xv = guard.embed(x.reshape(-1), device=dev)[0]
    pv = None if x0_prev is None else guard.embed(x0_prev.reshape(-1), device=dev)[0]
    outs = {"x_next": guard.sentinel_out((B * 4 * HW,), dtype=torch.float32, device=dev)}
    if want_x0:
        outs["x0"] = guard.sentinel_out((B * 4 * HW,), dtype=torch.float32, device=dev)
    arr = (C.c_float * 5)(*coef)
    lib.check(lib.load().pbe_dpmpp_update(eptr, ld, dup, cfg, xv.data_ptr(), None if pv is None else pv.data_ptr(), arr,
                                          outs["x0"][0].data_ptr() if want_x0 else None, outs["x_next"][0].data_ptr(), B, HW, _stream()), "pbe_dpmpp_update")
    for name, (view, arena) in outs.items():
        guard.assert_untouched(arena, view, f"dpmpp_update {name}")
        guard.assert_fully_written(view, f"dpmpp_update {name}")
    return (outs["x0"][0].view(B, 4, HW) if want_x0 else None), outs["x_next"][0].view(B, 4, HW)


# ---- 6. the kernel against fp64, per element ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [8, 16])
@pytest.mark.parametrize("HW", [65, 256, 384])
def test_kernel_against_fp64(dev, HW, ld):
    """B = 2 (the conditional half sits B*HW tokens behind the unconditional one), 130 / 512 / 768 tokens (a ragged last block, exact
    blocks), dup 1 / 2, with and without x0_prev, x0_out given and NULL.  Bound: dpmref's docstring (8 * 2^-24 * S per element; the
    derivation gives 4 and 6).  tests/test_dpm_solver_cpu.py shows the gate rejecting swapped halves and k1 applied to x0."""
    from pbe_amd import ops
    B = 2
    worst = [0.0, 0.0]
    for dup in (1, 2):
        eps, x, x0p = _operands(B, HW, dup, 7 * HW + ld + dup)
        for prev in (True, False):
            coef = _coef(prev)
            ref = dpmref.update_reference(eps, dup, 5.0, x, x0p if prev else None, coef)
            what = f"HW {HW} ld {ld} dup {dup} prev {prev}"
            full = _launch(dev, eps, ld, dup, 5.0, x, x0p if prev else None, coef, True)
            lean = _launch(dev, eps, ld, dup, 5.0, x, x0p if prev else None, coef, False)           # x0_out NULL
            worst = [max(a, b) for a, b in zip(worst, dpmref.update_gate(full[0], full[1], ref, what))]
            dpmref.update_gate(None, lean[1], ref, what + " (no x0_out)")
            assert lean[0] is None and torch.equal(lean[1], full[1])
            # the ops wrapper on plain tensors: the same bits
            e4 = torch.zeros(dup * B, HW, 1, ld, dtype=torch.float16)
            e4[..., :4] = eps.view(dup * B, HW, 1, 4)
            xn, x0 = ops.dpmpp_update(e4.to(dev), dup, 5.0, x.view(B, 4, HW, 1).to(dev), x0p.view(B, 4, HW, 1).to(dev) if prev else None, coef)
            assert torch.equal(xn.view(B, 4, HW), full[1]) and torch.equal(x0.view(B, 4, HW), full[0])
            assert ops.dpmpp_update(e4.to(dev), dup, 5.0, x.view(B, 4, HW, 1).to(dev), None, _coef(False), want_pred=False)[1] is None
    report(f"dpmpp_update HW {HW} ld {ld}: worst |d x0| / (u S0) (gate 8)", worst[0], 8.0)
    report(f"dpmpp_update HW {HW} ld {ld}: worst |d x_next| / (u Sn) (gate 8)", worst[1], 8.0)


def test_kernel_misaligned_eps_and_refusals(dev):
    """An eps base that is not 8-byte aligned takes the per-element read path: same gate.  k1 != 0 without x0_prev, ld < 4 and dup 3 are
    refused before anything is launched."""
    from pbe_amd import lib, ops
    from pbe_amd.lib import PbeError
    B, HW = 2, 65
    eps, x, x0p = _operands(B, HW, 2, 4242)
    coef = _coef(True)
    got = _launch(dev, eps, 8, 2, 5.0, x, x0p, coef, True, misalign=True)
    dpmref.update_gate(got[0], got[1], dpmref.update_reference(eps, 2, 5.0, x, x0p, coef), "misaligned eps")
    aligned = _launch(dev, eps, 8, 2, 5.0, x, x0p, coef, True)
    assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1])
    e4, x4 = torch.zeros(2 * B, HW, 1, 8, dtype=torch.float16, device=dev), x.view(B, 4, HW, 1).to(dev)
    with pytest.raises(PbeError):
        ops.dpmpp_update(e4, 2, 5.0, x4, None, coef)                                     # k1 != 0, no x0_prev
    out = torch.empty_like(x4)
    arr = (C.c_float * 5)(*coef)
    L = lib.load()
    assert L.pbe_dpmpp_update(e4.data_ptr(), 8, 2, 5.0, x4.data_ptr(), None, arr, None, out.data_ptr(), B, HW, _stream()) != 0
    assert L.pbe_dpmpp_update(e4.data_ptr(), 3, 2, 5.0, x4.data_ptr(), x4.data_ptr(), arr, None, out.data_ptr(), B, HW, _stream()) != 0
    assert L.pbe_dpmpp_update(e4.data_ptr(), 8, 3, 5.0, x4.data_ptr(), x4.data_ptr(), arr, None, out.data_ptr(), B, HW, _stream()) != 0
    for bad in (dict(dup=3), dict(x=x4[:, :3]), dict(eps=e4[:B]), dict(prev=x4[:1]), dict(coef=coef[:4]), dict(eps=e4.float()), dict(x=x4.cpu())):
        a = dict(eps=e4, dup=2, x=x4, prev=x4, coef=coef)
        a.update(bad)
        with pytest.raises(PbeError):
            ops.dpmpp_update(a["eps"], a["dup"], 5.0, a["x"], a["prev"], a["coef"])


# ---- 7. the first-order form against pbe_plms_update with DDIM's coefficients ---------------------------------------------------------
@pytest.mark.parametrize("dup", [1, 2])
def test_first_order_kernel_against_plms_update(dev, dup):
    """kx x + k0 x0 against sqrt(a') x0 + sqrt(1 - a') e of pbe_plms_update (one Adams-Bashforth weight of 1, no history) on the same
    inputs, rows of the 20-step table.  pred_x0 is the same arithmetic in both kernels and is held to the fp64 gate's bound,
    8 * 2^-24 * S0, on every row.  x_next is held to 8 * 2^-24 * Sn (S of the DPM form) on rows 19 and 0, the rows at which a 2M run
    takes the first-order form (its first and last step).
    In between that bound is not one two correct kernels can meet: pbe_plms_update's own rounding error is relative to ITS terms,
    Sp = |a'^1/2| S0 + |(1 - a')^1/2| Se, which stay large where x is small and Sn nearly vanishes (the DPM form is the more accurate
    one there), and the two kernels get separately rounded fp32 coefficients.  Both forms evaluated in correctly rounded fp32 on the CPU
    differ by up to 9.0 / 13.8 / 11.1 u Sn on rows 15 / 10 / 5 (7.1 and 3.9 on rows 19 and 0) while the DPM form stays within 1.8 u Sn of
    fp64.  On rows 15, 10 and 5 the difference is therefore held to each kernel's own bound of that form plus the coefficient rounding:
    8 u Sn + 8 u Sp + 3 u (Sn + Sp) (at most 3 rounded coefficients meet in a term)."""
    from ldm.models.diffusion.dpm_solver import dpmpp_coefficients
    from pbe_amd import ops
    B, HW = 2, 384
    eps, x, _ = _operands(B, HW, dup, 900 + dup)
    _, a, ap = O.ddim_parameters(O.schedule_buffers()["alphas_cumprod"], O.ddim_timesteps_uniform(20))
    table = dpmpp_coefficients(a, ap, 1)
    e4 = torch.zeros(dup * B, HW, 1, 8, dtype=torch.float16)
    e4[..., :4] = eps.view(dup * B, HW, 1, 4)
    e4, x4 = e4.to(dev), x.view(B, 4, HW, 1).to(dev)
    eu, ec = dpmref._halves(eps, dup)
    se = eu.abs() if dup == 1 else eu.abs() + 5.0 * (ec.abs() + eu.abs())
    for i in (19, 15, 10, 5, 0):
        a_t, a_n = float(a[i]), float(ap[i])
        coef8 = [1.0, 0.0, 0.0, 0.0, float(np.sqrt(1.0 - a_t)), 1.0 / float(np.sqrt(a_t)), float(np.sqrt(a_n)), float(np.sqrt(1.0 - a_n))]
        coef5 = table[i].tolist()
        p_next, p_x0, _ = ops.plms_update(e4, dup, 5.0, x4, [], coef8, want_e_t=False)
        d_next, d_x0 = ops.dpmpp_update(e4, dup, 5.0, x4, None, coef5)
        _, _, s0, sn = dpmref.update_reference(eps, dup, 5.0, x, None, coef5)
        p64 = (p_x0.cpu().double().view(B, 4, HW), p_next.cpu().double().view(B, 4, HW))
        w0 = dpmref.update_gate(d_x0, None, (p64[0], p64[1], s0, sn), f"row {i} dup {dup} vs plms_update")[0]
        err = (d_next.cpu().double().view(B, 4, HW) - p64[1]).abs()
        wn = float((err / (dpmref.U32 * sn + dpmref.FLOOR)).max())
        if i in (19, 0):
            report(f"dpmpp 1st order vs plms_update row {i} dup {dup}: worst |d| / (u S) (gate 8)", max(w0, wn), 8.0)
        print(f"row {i} dup {dup}: x0 {w0:.2f} u S0, x_next {wn:.2f} u Sn")
        if i in (19, 0):
            dpmref.update_gate(None, d_next, (p64[0], p64[1], s0, sn), f"row {i} dup {dup} vs plms_update")
        else:
            sp = coef8[6] * s0 + coef8[7] * se
            assert bool((err <= dpmref.U32 * (8 * sn + 8 * sp + 3 * (sn + sp)) + dpmref.FLOOR).all()), (i, dup, wn)


# ---- the narrow model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def narrow_sd(narrow):
    return {k: v.detach().float().cpu() for k, v in narrow.state_dict().items()}


def _oracle_model(narrow_sd):
    sd = {k[len("model.diffusion_model."):]: v for k, v in narrow_sd.items() if k.startswith("model.diffusion_model.")}
    return lambda x9, t, ctx: O.unet_forward(sd, x9, t, ctx, cases.UNET_NARROW)


def _sampler(narrow, graph=False, paired=True):
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(narrow)
    s.use_graph, s.share_guidance_prefix = graph, paired
    return s


def _kw(narrow, dev, golden_dir, c, S=6):
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    return dict(S=S, batch_size=2, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"].to(dev),
                test_model_kwargs={"inpaint_image": torch.from_numpy(gold["z_inpaint"]).to(dev), "inpaint_mask": torch.from_numpy(gold["mask_lat"]).to(dev)})


def _three_tokens(narrow, dev):
    g = torch.Generator().manual_seed(8)
    refs = torch.randn(2, 3, 3, 224, 224, generator=g)
    return narrow.proj_out(narrow.get_learned_conditioning(refs.to(dev)))


# ---- 8. the sampler against dpmref over the oracle U-Net ------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", ["one", "ragged3"])
def test_narrow_sampler_against_dpmref(dev, narrow, narrow_sd, golden_dir, tokens):
    """order 2, S = 6 (the reference grid has 7 points there: a first-order start, five second-order steps, a first-order end), scale 5:
    the conditioning of narrow.npz, and a ragged weighted 3-token batch (weights (2, 1, 0) and (0, 0, 1): the oracle runs per sample on
    [t0, t0, t1] and [t2], the one-token unconditional vector repeated to each length)."""
    inp = cases.narrow_inputs()
    gold = np.load(os.path.join(golden_dir, "narrow.npz"))
    z_inp, m = torch.from_numpy(gold["z_inpaint"]), torch.from_numpy(gold["mask_lat"])
    ac = O.schedule_buffers()["alphas_cumprod"]
    model = _oracle_model(narrow_sd)
    uc = narrow_sd["learnable_vector"]
    with torch.no_grad():
        if tokens == "one":
            c = torch.from_numpy(gold["c"]).to(dev)
            z0, inter = _sampler(narrow).sample(order=2, **_kw(narrow, dev, golden_dir, c))
            want, info = dpmref.dpm_sample(model, 6, inp["x_T"], c.float().cpu(), uc, 5.0, z_inp, m, ac, order=2)
            assert info["calls"] == 7 and len(inter["x_inter"]) == 3
        else:
            c, w, eq = _three_tokens(narrow, dev), torch.tensor([[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), [[0, 0, 1], [2]]
            z0, _ = _sampler(narrow).sample(order=2, conditioning_weights=w, **_kw(narrow, dev, golden_dir, c))
            cc = c.float().cpu()
            want = torch.cat([dpmref.dpm_sample(model, 6, inp["x_T"][b:b + 1], cc[b:b + 1, eq[b]], uc.expand(1, len(eq[b]), -1), 5.0,
                                                z_inp[b:b + 1], m[b:b + 1], ac, order=2)[0] for b in range(2)])
    v = rel_l2(z0, want)
    report(f"narrow DPM-Solver++(2M) S=6 (7 calls), {tokens} vs dpmref", v, SAMPLER_OPT_TOL)
    assert v <= SAMPLER_OPT_TOL, v


# ---- 9. mask / x0 blending with injected noise ----------------------------------------------------------------------------------------
def test_narrow_sampler_blend_against_dpmref(dev, narrow, narrow_sd):
    inp = cases.sampler_option_inputs()
    d = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in inp.items()}
    with torch.no_grad():
        smp = _sampler(narrow)
        it = iter(d["noises"])
        smp.noise_like = lambda shape, device: next(it)
        z0, _ = smp.sample(S=6, batch_size=2, shape=[4, 16, 16], conditioning=d["c"], verbose=False, unconditional_guidance_scale=5.0,
                           unconditional_conditioning=d["uc"], eta=0.0, x_T=d["x_T"].clone(), mask=d["blend_mask"], x0=d["x0"], order=2,
                           test_model_kwargs={"images_inpaint": d["z_inpaint"], "images_mask": d["mask_lat"]})
        want = dpmref.dpm_sample(_oracle_model(narrow_sd), 6, inp["x_T"], inp["c"], inp["uc"], 5.0, inp["z_inpaint"], inp["mask_lat"],
                                 O.schedule_buffers()["alphas_cumprod"], order=2, blend=(inp["blend_mask"], inp["x0"], inp["noises"]))[0]
    v = rel_l2(z0, want)
    report("narrow DPM-Solver++(2M) S=6, mask + x0 blending (injected noise) vs dpmref", v, SAMPLER_OPT_TOL)
    assert v <= SAMPLER_OPT_TOL, v


# ---- 10. what the sampler inherits ----------------------------------------------------------------------------------------------------
def _keys(fn):
    from pbe_amd import ops
    ops._TIMES = {}
    try:
        out = fn()
        return out, list(ops._TIMES)
    finally:
        ops._TIMES = None


def test_inherited_machinery_is_bit_identical(dev, narrow, golden_dir, monkeypatch):
    """Graphed against eager, the shared guidance prefix on against off, regions with an attribution-map collector against regions without
    (latent), a one-token run with a collector against one without (same launches, same bits), and the number of U-Net calls: S."""
    from ldm.modules.attention import ContextMaps
    unet = narrow.model.diffusion_model
    calls = []
    real = unet.forward_nhwc
    monkeypatch.setattr(unet, "forward_nhwc", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        c3 = _three_tokens(narrow, dev)
        wt, r = torch.tensor([[2.0, 1.0, 0.5], [1.0, 0.0, 3.0]]), rr.soft_regions(2, 3, 16, 16, seed=12)
        kw = dict(_kw(narrow, dev, golden_dir, c3, S=4), conditioning_weights=wt, conditioning_regions=r, order=2)
        z_e, _ = _sampler(narrow).sample(**kw)
        assert len(calls) == 4                                                           # S = 4: four grid points, four calls
        z_u, _ = _sampler(narrow, paired=False).sample(**kw)
        g = _sampler(narrow, graph=True)
        z_g, _ = g.sample(**kw)
        assert g._graphed is not None and g._graphed.replays == 3
        cm = ContextMaps()
        z_m, _ = _sampler(narrow).sample(conditioning_maps=cm, **kw)
        z_plain, _ = _sampler(narrow).sample(**dict(kw, conditioning_regions=None))
        res = cm.result((16, 16))
        k1 = dict(_kw(narrow, dev, golden_dir, c3[:, :1].contiguous(), S=4), order=2)
        cm1 = ContextMaps()
        (z_1m, _), keys_m = _keys(lambda: _sampler(narrow).sample(conditioning_maps=cm1, **k1))
        (z_10, _), keys_0 = _keys(lambda: _sampler(narrow).sample(**k1))
    assert torch.equal(z_e, z_g), "graphed vs eager"
    assert torch.equal(z_e, z_u), "shared guidance prefix on vs off"
    assert torch.equal(z_e, z_m), "regions with a collector vs without"
    assert not torch.equal(z_e, z_plain)
    assert tuple(res.shape) == (2, 3, 16, 16) and bool(torch.isfinite(res).all()) and bool((res[1, 1] == 0).all())
    assert all(n > 0 and n % 4 == 0 for n in cm.counts().values()), cm.counts()
    assert keys_m == keys_0 and not any(k.startswith("xa") for k in keys_m) and torch.equal(z_1m, z_10)
    assert torch.equal(cm1.result((16, 16)), torch.ones(2, 1, 16, 16, device=dev))


# ---- 11. the public surface -----------------------------------------------------------------------------------------------------------
def test_pipeline_sampler_dpm_and_the_other_samplers_unchanged(dev, narrow):
    """pipeline.inpaint(sampler="dpm") is the direct DPMSolverSampler call bit for bit; "plms" and "ddim" (and any other string: DDIM)
    give, after the new module is loaded and used, the bits they gave while it was absent from sys.modules - they never import it."""
    from pbe_amd import pipeline
    name = "ldm.models.diffusion.dpm_solver"
    inp = {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("image", "mask", "ref", "x_T", "post_eps")}
    run = lambda s: pipeline.inpaint(narrow, inp["image"], inp["mask"], inp["ref"], steps=4, scale=5.0, x_T=inp["x_T"], post_eps=inp["post_eps"], sampler=s)      # noqa: E731
    saved = sys.modules.pop(name, None)
    try:
        with torch.no_grad():
            before = {s: run(s)["latent"].clone() for s in ("plms", "ddim", "euler")}
        assert name not in sys.modules
    finally:
        if saved is not None:
            sys.modules[name] = saved
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    with torch.no_grad():
        out = run("dpm")
        direct, _ = DPMSolverSampler(narrow).sample(S=4, batch_size=2, shape=[4, 16, 16], conditioning=out["c"], verbose=False, unconditional_guidance_scale=5.0,
                                                    unconditional_conditioning=narrow.learnable_vector, eta=0.0, x_T=inp["x_T"],
                                                    test_model_kwargs={"inpaint_image": out["z_inpaint"], "inpaint_mask": out["mask_lat"]})
        after = {s: run(s)["latent"] for s in ("plms", "ddim", "euler")}
    assert torch.equal(out["latent"], direct)
    assert all(torch.equal(before[s], after[s]) for s in before) and torch.equal(before["ddim"], before["euler"])
    assert not torch.equal(out["latent"], before["ddim"]) and not torch.equal(out["latent"], before["plms"])


def test_inference_cli_dpm_solver(dev, golden_dir, tmp_path):
    """scripts/inference.py --dpm_solver on a bundled triple: the dumped tensors and the result PNG are those of
    pipeline.inpaint(sampler="dpm") on the same tensors, byte for byte; the run differs from the one without the flag (DDIM)."""
    import yaml
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    spec = importlib.util.spec_from_file_location("pbe_inference_cli_dpm", os.path.join(ROOT, "scripts", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    d = os.path.join(golden_dir, "examples")
    paths = (os.path.join(d, "image_example_1.png"), os.path.join(d, "mask_example_1.png"), os.path.join(d, "reference_example_1.jpg"))
    cfg, steps, seed = str(tmp_path / "narrow.yaml"), 4, 321
    with open(cfg, "w") as f:
        yaml.safe_dump({"model": build.narrow_config()}, f)

    def run(tag, extra):
        out, dump = str(tmp_path / tag), str(tmp_path / f"{tag}.npz")
        x = cli.main(extra + ["--outdir", out, "--config", cfg, "--ddim_steps", str(steps), "--image_path", paths[0], "--mask_path", paths[1],
                              "--reference_path", paths[2], "--seed", str(seed), "--scale", "5", "--fixed_code", "--random_weights", "--dump_tensors", dump])
        return x, np.load(dump), out
    out, t, outdir = run("dpm", ["--dpm_solver"])
    _, t0, _ = run("ddim", [])
    trip = preprocess.load_triple_device(*paths, dev)
    with torch.no_grad():
        model = build.narrow_model(dev)
        direct = pipeline.inpaint(model, trip["image"], trip["mask"], trip["ref"], steps=steps, scale=5.0, x_T=torch.from_numpy(t["x_T"]).to(dev),
                                  post_eps=torch.from_numpy(t["post_eps"]).to(dev), sampler="dpm")
    assert torch.equal(direct["latent"].float().cpu(), torch.from_numpy(t["latent"]))
    assert torch.equal(direct["image"].float().cpu(), out)
    host = preprocess.save_outputs(str(tmp_path / "host"), "image_example_1", seed, preprocess.load_triple(*paths), direct["image"].float().cpu()[0], 512, 512)
    a, b = np.asarray(Image.open(os.path.join(outdir, "results", f"image_example_1_{seed}.png"))), np.asarray(Image.open(host["result"]))
    assert a.shape == (512, 512, 3) and np.array_equal(a, b)
    assert np.array_equal(t["x_T"], t0["x_T"]) and not np.array_equal(t["latent"], t0["latent"])
