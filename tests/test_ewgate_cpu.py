"""tests/ewref.py on the CPU: every emulation of an element-wise kernel passes its own gate (pbe_plms_update fused and unfused), every
planted fault is rejected on the same inputs, the fp32 restatements of the exact kernels equal the reference's own expressions on the
exhaustive inputs the GPU tests use, and the coefficient rows the GPU test launches are the sampler's own: PLMSSampler._coef on the v1
schedule (configs/v1.yaml: linear 0.00085 .. 0.0120, 1000 steps, 50 PLMS steps) equals what the oracle builds from ddim_parameters.

Every planted fault is a test case of its own, so the rejections are listed by name (pytest -v); -s prints the measured ratios."""
import math
import os
import types

import numpy as np
import pytest
import torch

import ewref as ew
import windowref
from oracle_loader import O

F = np.float32


# ---- the sampler's coefficient rows -------------------------------------------------------------------------------------------------------
def v1_sampler(steps=50):
    """A PLMSSampler with the v1 schedule made, on a model that is nothing but its schedule buffers (no device, no U-Net)."""
    from ldm.models.diffusion.plms import PLMSSampler
    sb = O.schedule_buffers()
    model = types.SimpleNamespace(num_timesteps=1000, betas=torch.from_numpy(sb["betas"]), alphas_cumprod=torch.from_numpy(sb["alphas_cumprod"]),
                                  alphas_cumprod_prev=torch.from_numpy(sb["alphas_cumprod_prev"]))
    smp = PLMSSampler(model)
    smp.make_schedule(ddim_num_steps=steps, verbose=False)
    return smp


def v1_coef(row, weights, smp=None):
    return (smp or v1_sampler())._coef(row, weights)


def test_coef_rows_are_the_oracle_schedule():
    """All 50 rows, every weight set of the six forms: the eight values of _coef against the oracle's plms_sample arithmetic
    (sqrt(1 - a) in fp32 as the registered buffer, the other three from the fp32 alphas through python floats), bit for bit."""
    from ldm.models.diffusion import plms
    assert plms._AB == ew.AB
    smp = v1_sampler()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "v1.yaml")) as f:
        cfg = f.read()
    for key in ("linear_start: 0.00085", "linear_end: 0.0120", "timesteps: 1000"):
        assert key in cfg, key
    _, a, a_prev = O.ddim_parameters(O.schedule_buffers()["alphas_cumprod"], O.ddim_timesteps_uniform(50))
    sq1m = np.sqrt(1.0 - a)
    assert a.dtype == np.float32 and a.shape == (50,)
    for row in range(50):
        for _, _, w, _, _ in ew.PLMS_FORMS:
            want = list(w) + [0.0] * (4 - len(w)) + [float(sq1m[row]), 1.0 / math.sqrt(float(a[row])), math.sqrt(float(a_prev[row])),
                                                     math.sqrt(1.0 - float(a_prev[row]))]
            assert smp._coef(row, w) == want, (row, w)
    assert 13.0 < smp._coef(49, (1.0,))[5] < 13.5               # 1 / sqrt(a_t) = 13.16 at the first step of a 50-step run (t = 981)


# ---- pbe_plms_update --------------------------------------------------------------------------------------------------------------------
def _plms_case(smp, form, row, dup, cfg, HW=257):
    name, n_hist, w, _, _ = form
    coef = v1_coef(row, w, smp)
    eps, x, hist = ew.plms_operands(2, HW, dup, n_hist, 1000 * row + 10 * n_hist + dup)
    x = ew.plms_cancelling_x(eps, dup, cfg, x, hist, coef)
    return eps, x, hist, coef


def _plms_cases(smp):
    for form in ew.PLMS_FORMS:
        for row in ew.PLMS_ROWS:
            for dup in (1, 2):
                for cfg in (5.0, 1.5):
                    yield (f"{form[0]} row {row} dup {dup} cfg {cfg}", dup, cfg) + _plms_case(smp, form, row, dup, cfg)


def test_plms_emulation_passes():
    """The six forms x rows {49, 48, 47, 25, 1, 0} x dup {1, 2} x cfg {5, 1.5}, a quarter of x cancelling against c4 e': the fused and the
    unfused emulation meet R u S on all three outputs."""
    worst = [0.0, 0.0, 0.0]
    for what, dup, cfg, eps, x, hist, coef in _plms_cases(v1_sampler()):
        ref = ew.plms_reference(eps, dup, cfg, x, hist, coef)
        for fused in (False, True):
            w = ew.plms_gate(*ew.plms_emulated(eps, dup, cfg, x, hist, coef, fused=fused), ref, f"{what} fused {fused}")
            worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"plms_update emulation: worst e_t {worst[0]:.2f} u Se (3), pred_x0 {worst[1]:.2f} u S0 (up to 13), x_prev {worst[2]:.2f} u Sp (up to 16)")


@pytest.mark.parametrize("fault", ew.PLMS_FAULTS)
def test_plms_fault_is_rejected(fault):
    """Each planted fault misses the gate on every one of the same cases it applies to (swap_h12 needs two history tensors, drop_hist one,
    swap_halves guidance)."""
    n = 0
    for what, dup, cfg, eps, x, hist, coef in _plms_cases(v1_sampler()):
        if (fault == "swap_h12" and len(hist) < 2) or (fault == "drop_hist" and not hist) or (fault == "swap_halves" and dup == 1):
            continue
        ref = ew.plms_reference(eps, dup, cfg, x, hist, coef)
        with pytest.raises(AssertionError):
            ew.plms_gate(*ew.plms_emulated(eps, dup, cfg, x, hist, coef, fault=fault), ref, what)
        n += 1
    assert n >= 24
    print(f"plms_update fault rejected: {fault} ({n} cases)")


def test_plms_gate_holds_where_pred_x0_cancels():
    """On the cancelling quarter |pred_x0| is far below S_0 - a result-relative tolerance of 1e-5 would fail the correct emulation there,
    the S-relative gate passes it."""
    smp = v1_sampler()
    eps, x, hist, coef = _plms_case(smp, ew.PLMS_FORMS[4], 49, 2, 5.0)
    ref = ew.plms_reference(eps, 2, 5.0, x, hist, coef)
    got = ew.plms_emulated(eps, 2, 5.0, x, hist, coef)
    ew.plms_gate(*got, ref, "cancelling")
    q = np.abs(ref["x0"].reshape(-1)[::4])
    assert (q <= 4 * ew.U * ref["S0"].reshape(-1)[::4]).all()
    rel = np.abs(got[1].astype(np.float64) - ref["x0"]).reshape(-1)[::4] / np.maximum(q, 1e-300)
    assert (rel > 1e-5).mean() > 0.5


# ---- pbe_posterior_sample ---------------------------------------------------------------------------------------------------------------
def posterior_operands(B=2, HW=257, ld=8):
    n = B * HW * 4
    mean, lv, eps = ew.posterior_lanes(n)
    mom = np.full((B, HW, ld), np.nan, np.float16)
    mom[..., :4], mom[..., 4:8] = mean.reshape(B, HW, 4), lv.reshape(B, HW, 4)
    return mom, np.ascontiguousarray(np.swapaxes(eps.reshape(B, HW, 4), 1, 2))


def test_posterior_emulation_passes():
    mom, eps = posterior_operands()
    lv = mom[..., 4:8].astype(np.float64)
    assert np.isinf(lv).any() and (lv == -30).any() and ((lv < -30) & (lv > -30.1)).any() and ((lv > 20) & (lv < 20.1)).any()
    want, bound = ew.posterior_reference(mom, eps, 0.18215)
    print(ew.gate(ew.posterior_emulated(mom, eps, 0.18215), want, bound, "posterior emulation"))


@pytest.mark.parametrize("fault", ew.POSTERIOR_FAULTS)
def test_posterior_fault_is_rejected(fault):
    mom, eps = posterior_operands()
    want, bound = ew.posterior_reference(mom, eps, 0.18215)
    with pytest.raises(AssertionError):
        ew.gate(ew.posterior_emulated(mom, eps, 0.18215, fault=fault), want, bound, fault)
    print(f"posterior_sample fault rejected: {fault}")


def test_expf_expansion_contracted_and_not():
    """The inline expansion of expf over the clamped range [-15, 10]: under 1 ulp as written (the exp2 instruction adds its own 1 ulp),
    more than 7 ulp once its difference is contracted into an fma - what the posterior gate caught on the device."""
    x = np.linspace(-15.0, 10.0, 100001).astype(F)
    t = np.exp(x.astype(np.float64))
    ulp = np.spacing(t.astype(F)).astype(np.float64)
    assert (np.abs(ew.expf_lowered(x, False) - t) / ulp).max() < 1.0
    assert (np.abs(ew.expf_lowered(x, True) - t) / ulp).max() > 7.0


# ---- the exact kernels ------------------------------------------------------------------------------------------------------------------
def test_rne_restatements_agree():
    """numpy's astype(float16), torch's .half() and the integer statement of round-to-nearest-even agree bit for bit on every input the
    GPU conversions are given; the specials land where IEEE puts them."""
    x = ew.rne_inputs()
    a = ew.rne16(x)
    assert np.array_equal(a, ew.rne16_bits(x))
    assert np.array_equal(a, torch.from_numpy(x).half().numpy().view(np.uint16))
    one = lambda v: int(ew.rne16(np.array([v], F))[0])          # noqa: E731
    assert one(65504.0) == 0x7BFF and one(np.nextafter(F(65520.0), F(0.0))) == 0x7BFF and one(65520.0) == 0x7C00 and one(1e30) == 0x7C00
    assert one(-np.inf) == 0xFC00 and one(2.0 ** -25) == 0 and one(np.nextafter(F(2.0 ** -25), F(1.0))) == 1 and one(-1e-40) == 0x8000
    assert one(1.0 + 2.0 ** -11) == 0x3C00 and one(1.0 + 3 * 2.0 ** -11) == 0x3C02                  # ties go to the even pattern


def test_widen_and_image_post_restatements():
    bits = ew.all_f16_bits()
    wide = ew.widen16(bits)
    t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16)
    nan = np.isnan(wide)
    assert int(nan.sum()) == 2 * 1023 and np.array_equal(nan, torch.isnan(t).numpy())
    assert np.array_equal(wide[~nan].view(np.uint32), t.float().numpy()[~nan].view(np.uint32))
    keep = ~nan                                                 # the finite patterns and +-inf
    want = torch.clamp((t.float()[torch.from_numpy(keep)] + 1.0) / 2.0, min=0.0, max=1.0).numpy()          # scripts/inference.py:346
    assert np.array_equal(ew.image_post32(bits[keep].view(np.float16)).view(np.uint32), want.view(np.uint32))


def test_u8_to_planes_restatement():
    from pbe_amd.preprocess import CLIP_MEAN, CLIP_STD
    v = np.stack([(np.arange(256) + 85 * c) % 256 for c in range(3)], -1).astype(np.uint8)          # [256, 3]
    for mean, std in (((0.5,) * 3, (0.5,) * 3), (CLIP_MEAN, CLIP_STD)):
        t = torch.from_numpy(v).to(torch.float32).div(255)                                            # ToTensor
        want = t.sub(torch.tensor(mean, dtype=torch.float32)).div(torch.tensor(std, dtype=torch.float32))      # Normalize
        assert np.array_equal(ew.u8_to_planes32(v, mean, std).view(np.uint32), want.numpy().view(np.uint32))
    m = v[:, :1]
    inv = 1 - torch.from_numpy(m).to(torch.float32).div(255)
    assert np.array_equal(ew.u8_to_planes32(m, mode=2), inv.numpy())
    thr = inv.clone()
    thr[thr < 0.5], thr[thr >= 0.5] = 0, 1                                                            # scripts/inference.py:311-315
    got = ew.u8_to_planes32(m, mode=1)
    assert np.array_equal(got, thr.numpy())
    assert got[m[:, 0] == 127, 0] == 1 and got[m[:, 0] == 128, 0] == 0                              # 1 - 128 / 255 < 0.5 <= 1 - 127 / 255


def test_canvas_restatement():
    from pbe_amd.preprocess import CLIP_MEAN, CLIP_STD
    for a, b in [(1.0, 0.0), (0.5, 0.5)] + list(zip(CLIP_STD, CLIP_MEAN)):
        x = ew.canvas_sources(a, b)
        y = torch.clamp(torch.from_numpy(x) * torch.tensor(a, dtype=torch.float32) + torch.tensor(b, dtype=torch.float32), 0.0, 1.0)
        want = (255. * y.numpy()).astype(np.uint8)
        got = ew.canvas_bytes(x, a, b)
        assert np.array_equal(got, want), (a, b)
        assert got.min() == 0 and got.max() == 255 and len(np.unique(got)) == 256
    # truncation, not rounding: the fp32 below k / 255 gives k - 1
    k = (np.arange(1, 256) / 255.0).astype(F)
    assert (ew.canvas_bytes(np.nextafter(k, F(0.0)), 1.0, 0.0).astype(int) <= np.arange(1, 256)).all()
    assert ew.canvas_bytes(np.array([0.999999], F), 1.0, 0.0)[0] == 254


def test_scale_latent_check_accepts_both_rounding_orders_and_rejects_truncation():
    x = ew.rne_inputs()
    s = F(1 / 0.18215)
    with np.errstate(over="ignore"):
        two = ew.rne16(x * s)                                                                         # fp32 product, then the conversion
        one = ew.rne16((x.astype(np.float64) * float(s)).astype(np.float16).astype(F))               # one rounding of the exact product
    assert ew.scale_latent_check(two, x, 1 / 0.18215, "two roundings").ratio <= 1.0
    assert ew.scale_latent_check(one, x, 1 / 0.18215, "one rounding").ratio <= 1.0
    with np.errstate(over="ignore"):
        trunc = ((x * s).view(np.uint32) & 0xFFFFE000).view(F)                                        # the low 13 bits cut: round toward zero
    finite = np.abs(x) < 1e4                                                                          # (past 65504 truncation fails the inf check instead)
    assert ew.scale_latent_check(ew.rne16(trunc[finite]), x[finite], 1 / 0.18215, "truncated").ratio > 1.0
    print("scale_latent fault rejected: truncation")


# ---- pbe_resize_bilinear_f32 ------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [((512, 512), (64, 64), 1), ((96, 64), (12, 8), 1), ((100, 77), (13, 31), 1), ((9, 7), (31, 17), 1), ((64, 64), (64, 64), 1),
                ((62, 31), (2, 1), 2)]


def resize_source(shape_in, planes, seed):
    """A plane with an edge and texture: uniform [0, 1) on the left part, a 0/1 mask pattern on the rest."""
    r = np.random.RandomState(seed)
    v = r.random_sample((planes,) + tuple(shape_in)).astype(F)
    cut = shape_in[1] // 2
    v[:, :, cut:] = (r.random_sample((planes, shape_in[0], shape_in[1] - cut)) < 0.5).astype(F)
    return v


def test_resize_matrix_is_the_triangle_filter():
    """Where the fp32 scale is exact, the fp64 filter built from it is windowref.aa_matrix (the integer statement of the same filter)."""
    for n_in, n_out in ((512, 64), (96, 12), (64, 64), (62, 2), (31, 1), (9, 31), (64, 8)):
        s = ew.resize_scale(n_in, n_out)
        if s * n_out == n_in:
            assert np.allclose(ew.resize_matrix(n_in, n_out, True)[0], windowref.aa_matrix(n_in, n_out)[0], rtol=0, atol=1e-15), (n_in, n_out)
    for n_in, n_out in ((100, 13), (77, 31), (7, 17)):
        assert np.abs(ew.resize_matrix(n_in, n_out, True)[0] - windowref.aa_matrix(n_in, n_out)[0]).max() < 1e-5
    assert ew.resize_accepts(31, 1) and not ew.resize_accepts(32, 1) and ew.resize_accepts(62, 2) and not ew.resize_accepts(64, 2)


_case_id = lambda c: "%dx%d-%dx%d" % (c[0] + c[1])          # noqa: E731


@pytest.mark.parametrize("case", RESIZE_CASES, ids=_case_id)
def test_resize_emulation_passes(case):
    shape_in, size, planes = case
    src = resize_source(shape_in, planes, 5)
    for aa in (True, False):
        want, bound = ew.resize_reference(src, size, aa)
        got = ew.resize_emulated(src, size, aa)
        print(ew.gate(got, want, bound, f"resize {shape_in} -> {size} aa {aa}"), f"largest bound {bound.max():.2e}")
        if shape_in == size:
            assert np.array_equal(got.view(np.uint32), src.view(np.uint32))


def _fault_applies(fault, shape_in, size):
    down = shape_in[0] > size[0] or shape_in[1] > size[1]
    if fault == "support1":
        return down                                             # otherwise the support is 1 already
    if fault == "unnormalised":
        return shape_in != size                                 # the identity's single weight is 1
    return True


@pytest.mark.parametrize("case,fault", [(c, f) for c in RESIZE_CASES for f in ew.RESIZE_FAULTS if _fault_applies(f, c[0], c[1])],
                         ids=lambda v: v if isinstance(v, str) else _case_id(v))
def test_resize_fault_is_rejected(case, fault):
    shape_in, size, planes = case
    src = resize_source(shape_in, planes, 5)
    want, bound = ew.resize_reference(src, size, True)
    with pytest.raises(AssertionError):
        ew.gate(ew.resize_emulated(src, size, True, fault=fault), want, bound, fault)
    print(f"resize_bilinear fault rejected: {fault} ({shape_in} -> {size})")
