"""The sampler-step and image-boundary kernels (pbe_amd/csrc/elementwise.hip) per element on the GPU, against the fp64 references, bounds
and bit-exact restatements of tests/ewref.py (their derivations stand there; tests/test_ewgate_cpu.py shows each gate rejecting planted
faults and pins the restatements to the reference's own expressions).  Inputs sit between poison (guard.embed), outputs in sentinel
arenas (guard.sentinel_out): nothing outside an output is written, nothing inside is skipped.

Every case appends one line (what, worst |err| / bound, where) to the accuracy report beside the parity report, as
tests/test_accuracy_gpu.py does.  The last section holds the refusals of the ops wrappers: every deliberately wrong operand is a view
into an allocation large enough for the launch an unchecked wrapper would have made."""
import ctypes as C

import numpy as np
import pytest
import torch

import ewref as ew
import guard
from test_accuracy_gpu import report
from test_ewgate_cpu import RESIZE_CASES, posterior_operands, resize_source, v1_sampler

pytestmark = pytest.mark.gpu
F = np.float32
f32, f16, u8 = torch.float32, torch.float16, torch.uint8


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from pbe_amd import lib
    return lib, lib.load()


def _in(dev, a):
    """A host array, contiguous by the entry point's contract, on the device between poison."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return guard.embed(t.reshape(-1), device=dev)[0]


def _out(dev, n, dtype):
    return guard.sentinel_out((int(n),), dtype=dtype, device=dev)


def _done(out, what, written=True):
    view, arena = out
    guard.assert_untouched(arena, view, what)
    if written:
        guard.assert_fully_written(view, what)
    return view


def _bits16(view):
    return view.view(torch.int16).cpu().numpy().view(np.uint16)


def _bits32(view):
    return view.view(torch.int32).cpu().numpy().view(np.uint32)


def _ptr(v):
    return None if v is None else v.data_ptr()


def _line(what, ratio, where, extra=""):
    report(f"{what:64s} err/bound={ratio:.3f} at {where}{extra}")


# ---- pbe_plms_update --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler():
    return v1_sampler()


def _plms_launch(dev, eps, ld, dup, cfg, x, hist, coef, want_e, want_pred):
    """One raw launch: eps [dup*B, HW, 4] with leading dimension ld (channels 4 .. ld-1 NaN), an omitted output passed as NULL.
    -> {name: fp32 [B, 4, HW] device view}."""
    lib, L = _lib()
    B, _, HW = x.shape
    e = np.full((dup * B * HW, ld), np.nan, np.float16)
    e[:, :4] = eps.reshape(-1, 4)
    ev, xv = _in(dev, e), _in(dev, x)
    hv = [_in(dev, h) for h in hist] + [None] * (3 - len(hist))
    outs = {k: _out(dev, B * 4 * HW, f32) for k, on in (("e_t", want_e), ("x_prev", True), ("pred_x0", want_pred)) if on}
    p = {k: v[0].data_ptr() for k, v in outs.items()}
    lib.check(L.pbe_plms_update(ev.data_ptr(), ld, dup, cfg, xv.data_ptr(), _ptr(hv[0]), _ptr(hv[1]), _ptr(hv[2]), (C.c_float * 8)(*coef),
                                p.get("e_t"), p["x_prev"], p.get("pred_x0"), B, HW, _stream()), "pbe_plms_update")
    return {k: _done(v, f"plms_update {k}").view(B, 4, HW) for k, v in outs.items()}


@pytest.mark.parametrize("HW", [1, 257, 4099])
@pytest.mark.parametrize("form", ew.PLMS_FORMS, ids=lambda f: f[0])
def test_plms_update_forms(dev, sampler, form, HW):
    """The six forms the samplers launch (ewref.PLMS_FORMS) on the sampler's own coefficient rows {49, 48, 47, 25, 1, 0} of the 50-step v1
    schedule, B = 2 (the conditional half sits B * HW tokens behind the unconditional one), 1 / 257 / 4099 pixels (one thread of a block, a
    ragged second block, 65 blocks), dup 1 / 2, cfg 5 / 1.5, ld 4 / 8 / 16 with NaN in the channels past 3.  A quarter of x is
    fp32(c4 e'): pred_x0 is all cancellation there and only a bound relative to S_0 can hold.  Gates: R_e / R_0 / R_p u S (ewref).  An
    output the form omits is passed as NULL; the others carry the bits of the launch that writes all three."""
    name, n_hist, weights, want_e, want_pred = form
    B = 2
    worst = [0.0, 0.0, 0.0]
    for row in ew.PLMS_ROWS:
        coef = sampler._coef(row, weights)
        for dup in (1, 2):
            eps, x0, hist = ew.plms_operands(B, HW, dup, n_hist, 7919 * row + 31 * n_hist + dup + HW)
            for cfg in (5.0, 1.5):
                x = ew.plms_cancelling_x(eps, dup, cfg, x0, hist, coef)
                ref = ew.plms_reference(eps, dup, cfg, x, hist, coef)
                for ld in (4, 8, 16):
                    what = f"plms_update {name} HW {HW} row {row} dup {dup} cfg {cfg} ld {ld}"
                    full = _plms_launch(dev, eps, ld, dup, cfg, x, hist, coef, True, True)
                    w = ew.plms_gate(full["e_t"], full["pred_x0"], full["x_prev"], ref, what)
                    worst = [max(a, b / r) if r else a for a, b, r in zip(worst, w, (ref["Re"], ref["R0"], ref["Rp"]))]
                    if not (want_e and want_pred):
                        lean = _plms_launch(dev, eps, ld, dup, cfg, x, hist, coef, want_e, want_pred)
                        assert set(lean) == {k for k, on in (("e_t", want_e), ("x_prev", True), ("pred_x0", want_pred)) if on}
                        for k, v in lean.items():
                            assert torch.equal(guard.bits(v), guard.bits(full[k])), f"{what}: {k} differs when an output is NULL"
    for k, out in enumerate(("e_t", "pred_x0", "x_prev")):
        _line(f"plms_update {name} HW {HW}: {out} against its R u S", worst[k], "-", f" (R = {(3, 7 + 2 * n_hist, 10 + 2 * n_hist)[k]} with dup 2, 3 less with dup 1)")


def test_plms_update_wrapper_same_bits(dev, sampler):
    """ops.plms_update on plain tensors gives the bits of the raw launch, for every form (the wrapper's operand checks accept what the
    samplers pass)."""
    from pbe_amd import ops
    B, H, W, ld = 2, 3, 19, 8
    for name, n_hist, weights, want_e, want_pred in ew.PLMS_FORMS:
        coef = sampler._coef(47, weights)
        eps, x, hist = ew.plms_operands(B, H * W, 2, n_hist, 99 + n_hist)
        raw = _plms_launch(dev, eps, ld, 2, 5.0, x, hist, coef, want_e, want_pred)
        e4 = torch.zeros(2 * B, H, W, ld, dtype=f16)
        e4[..., :4] = torch.from_numpy(eps).view(2 * B, H, W, 4)
        t = lambda a: torch.from_numpy(a).view(B, 4, H, W).to(dev)          # noqa: E731
        xp, pred, e_t = ops.plms_update(e4.to(dev), 2, 5.0, t(x), [t(h) for h in hist], coef, want_e_t=want_e, want_pred=want_pred)
        assert (e_t is None) == (not want_e) and (pred is None) == (not want_pred)
        for k, got in (("x_prev", xp), ("pred_x0", pred), ("e_t", e_t)):
            if got is not None:
                assert torch.equal(guard.bits(got.view(B, 4, H * W)), guard.bits(raw[k].contiguous())), (name, k)


# ---- pbe_posterior_sample ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [8, 16])
def test_posterior_sample_clamp_bounds(dev, ld):
    """257 pixels, B = 2; the log-variance lanes cycle through the fp16 values around both clamp bounds (+-inf, +-65504, +-31, -30 and 20
    with two fp16 neighbours on each side), the means reach +-65504, eps holds 0 and +-4 (ewref.posterior_lanes); channels 8 .. ld-1 are
    NaN.  Bound: u (3 S + 2 E |scale| ex |eps|), E = 2 ulp for expf (ewref)."""
    lib, L = _lib()
    from pbe_amd import ops
    B, HW = 2, 257
    mom, eps = posterior_operands(B, HW, ld)
    out = _out(dev, B * 4 * HW, f32)
    d_mom, d_eps = _in(dev, mom), _in(dev, eps)      # kept alive: the launch reads them
    lib.check(L.pbe_posterior_sample(d_mom.data_ptr(), ld, d_eps.data_ptr(), out[0].data_ptr(), B, HW, 0.18215, _stream()), "posterior")
    z = _done(out, "posterior_sample").view(B, 4, HW)
    want, bound = ew.posterior_reference(mom, eps, 0.18215)
    w = ew.gate(z, want, bound, f"posterior_sample ld {ld}")
    _line(f"posterior_sample clamp lanes HW {HW} ld {ld} (E = {ew.EXPF_ULP:g} ulp)", w.ratio, w.where)
    m4 = torch.from_numpy(mom).view(B, HW, 1, ld).clone()
    m4[..., 8:] = 0
    plain = ops.posterior_sample(m4.to(dev), torch.from_numpy(eps).view(B, 4, HW, 1).to(dev), 0.18215)
    assert torch.equal(guard.bits(plain.view(B, 4, HW)), guard.bits(z.contiguous()))


# ---- exact kernels: every fp16 pattern through the widening kernels -----------------------------------------------------------------------
def _patterns(C_, keep=None):
    """All 65536 fp16 patterns as [2, HW, C_] (65536 split over the C_ read channels, the slots past them 0; batch 1 in reverse order);
    keep: a mask over the patterns, the others are replaced by +0."""
    bits = ew.all_f16_bits()
    if keep is not None:
        bits = np.where(keep, bits, 0).astype(np.uint16)
    HW = -(-65536 // C_)
    a = np.zeros((2, HW * C_), np.uint16)
    a[0, :65536], a[1, :65536] = bits, bits[::-1]
    return a.reshape(2, HW, C_), HW


@pytest.mark.parametrize("C_,ld", [(1, 8), (4, 4), (9, 16)])
def test_nhwc_to_nchw_every_pattern(dev, C_, ld):
    """All 65536 fp16 patterns, subnormals and both infinities among them: exact widening bit for bit; NaN maps to NaN."""
    lib, L = _lib()
    pat, HW = _patterns(C_)
    src = np.full((2, HW, ld), 0x7E00, np.uint16)
    src[..., :C_] = pat
    out = _out(dev, 2 * C_ * HW, f32)
    d_src = _in(dev, src.view(np.float16))      # kept alive: the launch reads them
    lib.check(L.pbe_nhwc_f16_to_nchw_f32(d_src.data_ptr(), out[0].data_ptr(), 2, C_, HW, ld, _stream()), "nhwc_to_nchw")
    got = _bits32(_done(out, "nhwc_to_nchw")).reshape(2, C_, HW).view(F)
    want = np.swapaxes(ew.widen16(pat), 1, 2)
    nan = np.isnan(want)
    assert int(nan.sum()) == 2 * 2046 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    _line(f"nhwc_to_nchw all fp16 patterns C {C_} ld {ld}: exact", 0.0, "-")


def test_image_post_every_pattern(dev):
    """Every finite fp16 pattern and +-inf through clamp((x + 1) * 0.5, 0, 1), bit for bit in IEEE fp32; ld = 8, channels 3 .. 7 NaN."""
    lib, L = _lib()
    from pbe_amd import ops
    pat, HW = _patterns(3, keep=~np.isnan(ew.widen16(ew.all_f16_bits())))
    src = np.full((2, HW, 8), 0x7E00, np.uint16)
    src[..., :3] = pat
    out = _out(dev, 2 * 3 * HW, f32)
    d_src = _in(dev, src.view(np.float16))      # kept alive: the launch reads them
    lib.check(L.pbe_image_post_f32(d_src.data_ptr(), out[0].data_ptr(), 2, HW, 8, _stream()), "image_post")
    view = _done(out, "image_post")
    want = np.swapaxes(ew.image_post32(pat.view(np.float16)), 1, 2)
    assert np.array_equal(_bits32(view).reshape(2, 3, HW), want.view(np.uint32))
    plain = src.copy()
    plain[..., 3:] = 0
    y = ops.image_post(torch.from_numpy(plain.view(np.float16)).view(2, HW, 1, 8).to(dev))
    assert torch.equal(guard.bits(y.view(-1)), guard.bits(view.contiguous()))
    _line("image_post finite fp16 patterns and +-inf, ld 8: exact", 0.0, "-")


# ---- exact kernels: round to nearest even ---------------------------------------------------------------------------------------------
def _rne_planes(C_):
    """ewref.rne_inputs() as fp32 [2, C_, HW] (zeros past the last value; batch 1 in reverse order)."""
    v = ew.rne_inputs()
    HW = -(-v.size // C_)
    a = np.zeros((2, C_ * HW), F)
    a[0, :v.size], a[1, :v.size] = v, v[::-1]
    return a.reshape(2, C_, HW), HW


@pytest.mark.parametrize("C_,Cp", [(9, 16), (4, 8), (1, 8), (8, 8)])
def test_nchw_to_nhwc_rounds_to_nearest_even(dev, C_, Cp):
    """Every fp16 value, every fp32 midpoint between two of them and both fp32 neighbours of each midpoint, both signs, 65504 / 65520 and
    the values around them, 1e30, +-inf, 2^-25 and its neighbour, fp32 subnormals (ewref.rne_inputs): the conversion is RNE bit for bit,
    and channels C .. Cp-1 are +0."""
    lib, L = _lib()
    src, HW = _rne_planes(C_)
    out = _out(dev, 2 * HW * Cp, f16)
    d_src = _in(dev, src)      # kept alive: the launch reads them
    lib.check(L.pbe_nchw_f32_to_nhwc_f16(d_src.data_ptr(), out[0].data_ptr(), 2, C_, HW, Cp, _stream()), "nchw_to_nhwc")
    got = _bits16(_done(out, "nchw_to_nhwc")).reshape(2, HW, Cp)
    assert np.array_equal(got[..., :C_], np.swapaxes(ew.rne16(src), 1, 2)) and (got[..., C_:] == 0).all()
    _line(f"nchw_to_nhwc RNE inputs C {C_} -> {Cp}: exact", 0.0, "-")


@pytest.mark.parametrize("dup", [1, 2])
def test_plms_pack_input_rounds_to_nearest_even(dev, dup):
    """The same inputs through the nine channels pbe_plms_pack_input converts (x, z_inpaint, mask): RNE bit for bit, channels 9 .. 15 +0,
    the second copy (dup 2) equal to the first."""
    lib, L = _lib()
    src, HW = _rne_planes(9)
    x, z, m = src[:, :4], src[:, 4:8], src[:, 8:]
    out = _out(dev, dup * 2 * HW * 16, f16)
    d_x, d_z, d_m = _in(dev, x), _in(dev, z), _in(dev, m)      # kept alive: the launch reads them
    lib.check(L.pbe_plms_pack_input(d_x.data_ptr(), d_z.data_ptr(), d_m.data_ptr(), out[0].data_ptr(), 2, HW, dup, _stream()), "plms_pack")
    got = _bits16(_done(out, "plms_pack_input")).reshape(dup, 2, HW, 16)
    want = np.swapaxes(ew.rne16(src), 1, 2)
    for d in range(dup):
        assert np.array_equal(got[d, ..., :9], want) and (got[d, ..., 9:] == 0).all(), d
    _line(f"plms_pack_input RNE inputs dup {dup}: exact", 0.0, "-")


@pytest.mark.parametrize("C_", [4, 9])
def test_scale_latent_bound_on_rounding_inputs(dev, C_):
    """The same inputs times fp32(1 / 0.18215) into fp16: within half an fp16 ulp plus the fp32 rounding of the exact product (one
    rounding or two - the bound tests/test_edges_gpu.py::test_layout_and_sampler_kernels states), inf past 65520, channels 4 .. 7 +0;
    with C = 9 the channels the kernel must not read are NaN."""
    lib, L = _lib()
    src4, HW = _rne_planes(4)
    src = np.full((2, C_, HW), np.nan, F)
    src[:, :4] = src4
    out = _out(dev, 2 * HW * 8, f16)
    d_src = _in(dev, src)      # kept alive: the launch reads them
    lib.check(L.pbe_scale_latent_f16(d_src.data_ptr(), out[0].data_ptr(), 2, C_, HW, 1 / 0.18215, _stream()), "scale_latent")
    got = _bits16(_done(out, "scale_latent")).reshape(2, HW, 8)
    assert (got[..., 4:] == 0).all()
    w = ew.scale_latent_check(np.swapaxes(got[..., :4], 1, 2), src4, 1 / 0.18215, f"scale_latent C {C_}")
    _line(f"scale_latent RNE inputs C {C_}: (2^-11 + 2^-23) |p| + 2^-25", w.ratio, w.where)
    assert w.ratio <= 1.0, str(w)


# ---- bytes <-> planes -------------------------------------------------------------------------------------------------------------------
def _norms():
    from pbe_amd.preprocess import CLIP_MEAN, CLIP_STD
    return (("half", (0.5,) * 3, (0.5,) * 3), ("clip", CLIP_MEAN, CLIP_STD))


@pytest.mark.parametrize("C_", [3, 1])
def test_u8_to_planes_every_byte(dev, C_):
    """All 256 byte values in every channel (B = 2, 257 pixels), (mean, std) = (0.5, 0.5) and CLIP's: v / 255, - mean, / std as three
    separately rounded fp32 operations, bit for bit; both mask modes, bytes 127 and 128 on either side of the threshold."""
    lib, L = _lib()
    HW = 257
    v = np.stack([(np.arange(2 * HW) * 3 + 85 * c) % 256 for c in range(C_)], -1).astype(np.uint8).reshape(2, HW, C_)
    assert all(len(np.unique(v[..., c])) == 256 for c in range(C_))
    sv = _in(dev, v)
    for name, mean, std in _norms():
        out = _out(dev, 2 * C_ * HW, f32)
        lib.check(L.pbe_u8_to_planes_f32(sv.data_ptr(), out[0].data_ptr(), 2, C_, HW, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), 0, _stream()), "u8_to_planes")
        want = np.swapaxes(ew.u8_to_planes32(v, mean, std), 1, 2)
        assert np.array_equal(_bits32(_done(out, "u8_to_planes")).reshape(2, C_, HW), want.view(np.uint32)), name
    for mode in (1, 2):
        out = _out(dev, 2 * C_ * HW, f32)
        lib.check(L.pbe_u8_to_planes_f32(sv.data_ptr(), out[0].data_ptr(), 2, C_, HW, None, None, mode, _stream()), "u8_to_planes")
        want = np.swapaxes(ew.u8_to_planes32(v, mode=mode), 1, 2)
        got = _bits32(_done(out, "u8_to_planes")).reshape(2, C_, HW)
        assert np.array_equal(got, want.view(np.uint32)), mode
        if mode == 1:
            b = np.swapaxes(v, 1, 2)
            assert (got.view(F)[b == 127] == 1).all() and (got.view(F)[b == 128] == 0).all()
    _line(f"u8_to_planes all bytes C {C_}, two normalisations, both mask modes: exact", 0.0, "-")


@pytest.mark.parametrize("bcast", [0, 1])
@pytest.mark.parametrize("norm", ["unit", "half", "clip"])
def test_planes_to_canvas_exact_bytes(dev, norm, bcast):
    """trunc(255 * clamp(fp32(x * a) + b, 0, 1)) byte for byte, for (a, b) = (1, 0), (0.5, 0.5) and CLIP's un-normalisation (std, mean), three
    channels and the broadcast of channel 0.  Sources (ewref.canvas_sources): (k / 255 - b) / a for every byte k with both fp32 neighbours -
    the edges of the truncation -, values that land below 0 and above 1, exactly 0 and 1.  A 9 x 8 rectangle in a 13 x 11 canvas, by turns
    against the bottom and right edges and against the top and left ones; no canvas byte outside it changes."""
    lib, L = _lib()
    a, b = {"unit": ((1.0,) * 3, (0.0,) * 3), "half": ((0.5,) * 3, (0.5,) * 3), "clip": (_norms()[1][2], _norms()[1][1])}[norm]      # clip: a = std, b = mean
    Hc, Wc, H, W = 13, 11, 9, 8
    per = [ew.canvas_sources(a[c], b[c]) for c in range(3)]
    if bcast:
        vals = [np.concatenate(per) if norm == "clip" else per[0]]
    else:
        vals = per
    n = vals[0].size
    calls = -(-n // (H * W))
    seen = set()
    for i in range(calls):
        idx = np.minimum(np.arange(i * H * W, (i + 1) * H * W), n - 1)
        src = np.stack([v[idx] for v in vals]).reshape(len(vals), H, W)
        y0, x0 = ((Hc - H, Wc - W), (0, 0))[i % 2]
        canvas, arena = guard.sentinel_out((Hc * Wc * 3,), dtype=u8, device=dev)
        canvas.fill_(0x3C)
        d_src = _in(dev, src)      # kept alive: the launch reads them
        lib.check(L.pbe_planes_to_u8_canvas(d_src.data_ptr(), canvas.data_ptr(), H, W, Hc, Wc, y0, x0, (C.c_float * 3)(*a), (C.c_float * 3)(*b), bcast,
                                            _stream()), "planes_to_canvas")
        guard.assert_untouched(arena, canvas, "planes_to_canvas")
        got = canvas.cpu().numpy().reshape(Hc, Wc, 3)
        want = np.full((Hc, Wc, 3), 0x3C, np.uint8)
        for c in range(3):
            want[y0:y0 + H, x0:x0 + W, c] = ew.canvas_bytes(src[0 if bcast else c], a[c], b[c])
        assert np.array_equal(got, want), (norm, bcast, i, np.argwhere(got != want)[:4].tolist())
        seen.update(np.unique(want[y0:y0 + H, x0:x0 + W]).tolist())
    assert len(seen) == 256
    _line(f"planes_to_canvas ({norm}) bcast {bcast}: {calls} rectangles, exact bytes", 0.0, "-")


# ---- pbe_resize_bilinear_f32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_resize_bilinear_per_element(dev, case):
    """Both filters against the fp64 filter built from the kernel's fp32 scale, per element within the bound derived in ewref (weight
    normalisation, the two accumulations over the tap counts, the fp32 centre): the 512 -> 64 mask resize, ragged down-scales, an
    up-scale, the identity (exact, both filters) and the largest horizontal scale an antialiased call accepts (31, two planes)."""
    lib, L = _lib()
    shape_in, size, planes = case
    src = resize_source(shape_in, planes, 5)
    sv = _in(dev, src)
    for aa in (1, 0):
        out = _out(dev, planes * size[0] * size[1], f32)
        lib.check(L.pbe_resize_bilinear_f32(sv.data_ptr(), out[0].data_ptr(), planes, shape_in[0], shape_in[1], size[0], size[1], aa, _stream()), "resize")
        got = _done(out, "resize_bilinear").view(planes, *size)
        want, bound = ew.resize_reference(src, size, bool(aa))
        w = ew.gate(got, want, bound, f"resize {shape_in} -> {size} aa {aa}")
        _line(f"resize_bilinear {shape_in[0]}x{shape_in[1]} -> {size[0]}x{size[1]} planes {planes} aa {aa}", w.ratio, w.where)
        if shape_in == size:
            assert np.array_equal(_bits32(got.contiguous()).reshape(src.shape), src.view(np.uint32)), f"aa {aa}: the identity is not exact"


def test_resize_bilinear_refuses_scale_32(dev):
    """Win = 32 Wout with antialias needs 66 taps: PBE_EINVAL, and not one element of the output arena is written."""
    _, L = _lib()
    assert not ew.resize_accepts(32, 1) and ew.resize_accepts(31, 1)
    src = resize_source((4, 64), 1, 6)
    view, arena = _out(dev, 4 * 2, f32)
    d_src = _in(dev, src)      # kept alive: the launch reads them
    assert L.pbe_resize_bilinear_f32(d_src.data_ptr(), view.data_ptr(), 1, 4, 64, 4, 2, 1, _stream()) == -1          # PBE_EINVAL
    torch.cuda.synchronize()
    assert bool((guard.bits(arena) == guard.SENTINEL_BITS[f32]).all())


# ---- the ops wrappers refuse inconsistent operands --------------------------------------------------------------------------------------
def test_wrappers_refuse_inconsistent_operands(dev):
    """ops.plms_update, ops.posterior_sample, ops.image_post and ops.nhwc_to_nchw refuse operands whose ranks, shapes, contiguity or counts
    do not fit each other - the cases an unchecked wrapper would have read out of bounds or in the wrong layout.  Every wrong operand is a
    view into an allocation that covers what such a launch would read, so the test asserts the refusal and nothing else."""
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    B, H, W, ld = 2, 4, 6, 8
    coef = [1.0, 0.0, 0.0, 0.0, 0.6, 1.25, 0.9, 0.43]
    big16 = torch.zeros(4 * 2 * B * H * W * 2 * ld, dtype=f16, device=dev)
    big32 = torch.zeros(4 * B * 4 * H * W * 2, dtype=f32, device=dev)
    eps = big16[:2 * B * H * W * ld].view(2 * B, H, W, ld)
    x = big32[:B * 4 * H * W].view(B, 4, H, W)
    h = big32[B * 4 * H * W:2 * B * 4 * H * W].view(B, 4, H, W)
    ops.plms_update(eps, 2, 5.0, x, [h], coef)                                                   # the consistent call is accepted
    wide = big32[:B * 4 * H * 2 * W].view(B, 4, H, 2 * W)
    bad_plms = [
        dict(eps=eps[:B]),                                                                       # batch B with dup 2
        dict(eps=big16[:2 * B * H * W * 2 * ld].view(2 * B, H, W, 2 * ld)[..., :ld]),           # not contiguous
        dict(eps=big16[:2 * B * H * W * 2].view(2 * B, H, W, 2)),                               # ld < 4
        dict(eps=big16[:2 * B * H * W * ld].view(2 * B, W, H, ld)),                             # H and W exchanged
        dict(eps=big16[:2 * B * H * W * ld].view(2 * B, H * W, ld)),                            # rank 3
        dict(x=wide[..., ::2]),                                                                  # not contiguous
        dict(x=big32[:B * 3 * H * W].view(B, 3, H, W)),                                         # 3 channels
        dict(x=big32[:B * 4 * H * W].view(B * 4, H, W)),                                        # rank 3
        dict(hist=[big32[:B * 4 * H * (W // 2)].view(B, 4, H, W // 2)]),                        # a history tensor of another shape
        dict(hist=[h, wide[..., ::2]]),                                                          # not contiguous
        dict(hist=[h, h, h, h]),                                                                 # more than three
        dict(dup=3), dict(dup=0),
        dict(coef=coef[:7]), dict(coef=coef + [0.0]),
    ]
    for bad in bad_plms:
        a = dict(eps=eps, dup=2, x=x, hist=[h], coef=coef)
        a.update(bad)
        with pytest.raises(PbeError):
            ops.plms_update(a["eps"], a["dup"], 5.0, a["x"], a["hist"], a["coef"])
    with pytest.raises(PbeError):
        ops.plms_update(eps, 1, 5.0, x, [h], coef)                                               # batch 2 B with dup 1
    # posterior_sample
    mom = big16[:B * H * W * ld].view(B, H, W, ld)
    noise = big32[:B * 4 * H * W].view(B, 4, H, W)
    ops.posterior_sample(mom, noise, 0.18215)
    for m, e in ((mom, big32[:B * 4 * H * (W // 2)].view(B, 4, H, W // 2)), (mom, wide[..., ::2]), (mom, big32[:4 * H * W].view(1, 4, H, W)),
                 (mom, big32[:B * 4 * H * W].view(B * 4, H, W)), (big16[:B * H * W * 4].view(B, H, W, 4), noise),
                 (big16[:B * H * W * 2 * ld].view(B, H, W, 2 * ld)[..., :ld], noise), (big16[:B * H * W * ld].view(B, H * W, ld), noise)):
        with pytest.raises(PbeError):
            ops.posterior_sample(m, e, 0.18215)
    # image_post, nhwc_to_nchw
    img = big16[:B * H * W * ld].view(B, H, W, ld)
    ops.image_post(img)
    ops.nhwc_to_nchw(img, 3)
    sliced = big16[:B * H * W * 2 * ld].view(B, H, W, 2 * ld)[..., :ld]
    for t in (sliced, big16[:B * H * W * ld].view(B, H * W, ld), big16[:B * H * W * 2].view(B, H, W, 2)):
        with pytest.raises(PbeError):
            ops.image_post(t)
    for t, c in ((sliced, 3), (big16[:B * H * W * ld].view(B, H * W, ld), 3), (img, ld + 1), (img, 0)):
        with pytest.raises(PbeError):
            ops.nhwc_to_nchw(t, c)
    torch.cuda.synchronize()
