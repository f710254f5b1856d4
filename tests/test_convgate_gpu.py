"""The conv-side block chains on the device against tests/convref.py: every case of convref.CASES through the product module's run() on
NHWC fp16 tensors, the output through convref.verdict (limits from the fp32 emulation in two summation orders, never from a kernel's
output), and the launches the block must make asserted from recorders around ops.groupnorm / conv3x3 / conv3x3_small / gemm.

Product entries: ResBlock.run(x, emb_out, skip), Upsample.run, Downsample.run, ResnetBlock.run, AttnBlock.run; the VAE heads through
Encoder.run / Decoder.run of a one-level model without blocks whose mid modules are pass-throughs (conv_in -> norm_out + swish ->
conv_out is then all that runs); the U-Net heads through the two statements of UNetModel.forward_nhwc that run them, on the model's own
pack (pk(): w_in, b_in / go, bo, eps_o, w_out, b_out) - the U-Net has no smaller entry.

The printed lines (pytest -s) are the GPU half of the DESIGN.md section; PBE_CONVGATE_REPORT=<file> appends them there.
"""
import os

import pytest
import torch
from torch import nn

import convref as R

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in R.CASES]
FORCED_TILE = 6 | (1 << 8)           # the 64 x 64 tile (dense and conv forms), split-K 1: 64 rows = one 8x8 image, so the conv leaves group statistics
FORCED_CASE = "res-cat-128+64to128-8x8-unit"
FORCED_CASES = (FORCED_CASE, "res-id-64to64-16x16-flat", "res-1x1-128to64-16x16-unit")
CONTROL_CASE = "res-id-64to64-16x16-flat"


def report(line):
    print(line)
    path = os.environ.get("PBE_CONVGATE_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


class _Recorded:
    """Recorders around the four ops the blocks launch through; the originals are back on exit."""
    NAMES = ("groupnorm", "conv3x3", "conv3x3_small", "gemm")

    def __enter__(self):
        from pbe_amd import ops
        self.ops, self.saved, self.calls = ops, {n: getattr(ops, n) for n in self.NAMES}, []

        def wrap(name, fn):
            def rec(*a, **kw):
                y = fn(*a, **kw)
                st = getattr(y, "_pbe_gstats", None) if isinstance(y, torch.Tensor) else None
                self.calls.append(dict(op=name, x2=kw.get("x2") is not None, a2=kw.get("a2") is not None, resid=kw.get("resid") is not None,
                                       rowvec=kw.get("rowvec") is not None, bias_per_row=bool(kw.get("bias_per_row")),
                                       phase=name == "conv3x3" and a[1].dim() == 3, stride=kw.get("stride", 1), pad=kw.get("pad", 1),
                                       in_gstats=name == "groupnorm" and getattr(a[0], "_pbe_gstats", None) is not None,
                                       out_blocks=0 if st is None else st.blocks, eps=a[3] if name == "groupnorm" else None,
                                       a_strided=name == "gemm" and a[0].dim() == 3 and a[0].stride(1) != a[0].shape[2],
                                       a_stride0=name == "gemm" and a[0].dim() == 3 and a[0].stride(0) == 0))
                return y
            return rec
        for n, fn in self.saved.items():
            setattr(ops, n, wrap(n, fn))
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.ops, n, fn)

    def of(self, name):
        return [c for c in self.calls if c["op"] == name]


class _Through(nn.Module):
    def run(self, h):
        return h


def _pad_channels(x, cp):
    return torch.nn.functional.pad(x, (0, cp - x.shape[-1])).contiguous()


def _module(c, sd, dev):
    """The product module of a case with the case's parameters, on the device."""
    from ldm.modules.diffusionmodules import model as vae
    from ldm.modules.diffusionmodules import openaimodel as unet
    kind, C, C2, Co = c["kind"], c["C"], c["C2"], c["Cout"]
    strict = True
    if kind == "res":
        m = unet.ResBlock(C + C2, R.EMB, 0.0, out_channels=Co)
    elif kind == "unet_up":
        m = unet.Upsample(C, True, out_channels=Co)
    elif kind == "unet_down":
        m = unet.Downsample(C, True, out_channels=Co)
    elif kind in ("unet_in", "unet_out"):
        width = Co if kind == "unet_in" else C
        m = unet.UNetModel(image_size=8, in_channels=9, model_channels=width, out_channels=4, num_res_blocks=1, attention_resolutions=(),
                           channel_mult=(1,), num_heads=8, use_spatial_transformer=True, context_dim=64, legacy=False)
        strict = False                                # only the head's parameters are the case's
    elif kind == "vres":
        m = vae.ResnetBlock(in_channels=C, out_channels=Co, dropout=0.0, temb_channels=0)
    elif kind == "vattn":
        m = vae.AttnBlock(C)
    elif kind == "vdown":
        m = vae.Downsample(C, True)
    elif kind == "vup":
        m = vae.Upsample(C, True)
    else:
        cls = vae.Encoder if kind == "venc" else vae.Decoder
        m = cls(ch=C2, out_ch=3, ch_mult=(1,), num_res_blocks=0, attn_resolutions=[], in_channels=3, resolution=16, z_channels=4, double_z=True)
        m.mid.block_1, m.mid.attn_1, m.mid.block_2 = _Through(), _Through(), _Through()
        if kind == "vdec":
            m.up[0].block = nn.ModuleList([])
    res = m.load_state_dict(sd, strict=strict)
    assert not res.unexpected_keys, res.unexpected_keys
    return m.to(dev)


def _run(c, m, inp, dev):
    """The block on the device -> fp16 NHWC on the device."""
    from pbe_amd import ops
    kind = c["kind"]
    x = inp["x"].to(dev)
    if kind == "res":
        return m.run(x, inp["emb_out"].to(dev), None if inp["skip"] is None else inp["skip"].to(dev))
    if kind == "unet_in":                             # UNetModel.forward_nhwc: h = ops.conv3x3_small(x16, p.w_in, p.b_in)
        p = m.pk()
        return ops.conv3x3_small(_pad_channels(x, p.cin_pad), p.w_in, p.b_in)
    if kind == "unet_out":                            # UNetModel.forward_nhwc: groupnorm(h, p.go, p.bo, p.eps_o, True) -> conv3x3(h, p.w_out, p.b_out)
        p = m.pk()
        return ops.conv3x3(ops.groupnorm(x, p.go, p.bo, p.eps_o, True), p.w_out, p.b_out)
    if kind in ("venc", "vdec"):
        return m.run(_pad_channels(x, m.pk().cin_pad))
    return m.run(x)


def _check_launches(c, rec):
    """The launches the block must make; -> (stats, stats_rows) of the U-Net ResBlock's second norm as it ran (else two_pass)."""
    kind, form = c["kind"], c["form"]
    gn, conv, small, gemm = rec.of("groupnorm"), rec.of("conv3x3"), rec.of("conv3x3_small"), rec.of("gemm")
    HW = c["hw"][0] * c["hw"][1]
    if kind in ("res", "vres"):
        assert len(gn) == 2 and len(conv) == 2 and not small, rec.calls
        assert gn[0]["x2"] == (form == "cat") and not gn[1]["x2"]
        assert len(gemm) == (0 if form == "id" else 1)
        assert all(g["a2"] == (form == "cat") for g in gemm)
        assert conv[0]["rowvec"] == (kind == "res") and conv[1]["resid"] and not conv[0]["resid"]
        want_eps = R.EPS_UNET if kind == "res" else R.EPS_VAE
        assert [g["eps"] for g in gn] == [want_eps, want_eps], [g["eps"] for g in gn]
        assert gn[1]["in_gstats"] == (conv[0]["out_blocks"] > 0)      # the second norm took the route the conv's output offered
        if kind == "vres":
            assert conv[0]["out_blocks"] == 0                         # the VAE block asks for no group statistics
        if conv[0]["out_blocks"]:
            assert HW % conv[0]["out_blocks"] == 0
            return "conv", HW // conv[0]["out_blocks"]
    elif kind in ("unet_up", "vup"):
        assert len(conv) == 1 and conv[0]["phase"] and not gn and not gemm
    elif kind == "unet_down":
        assert len(conv) == 1 and (conv[0]["stride"], conv[0]["pad"]) == (2, 1) and not conv[0]["phase"]
    elif kind == "vdown":
        assert len(conv) == 1 and (conv[0]["stride"], conv[0]["pad"]) == (2, 0)
    elif kind == "unet_in":
        assert len(small) == 1 and not conv and not gn
    elif kind == "unet_out":
        assert len(gn) == 1 and gn[0]["eps"] == R.EPS_UNET and len(conv) == 1 and not small
    elif kind == "vattn":
        assert len(gn) == 1 and gn[0]["eps"] == R.EPS_VAE and len(gemm) == 5 and not conv
        assert sum(g["bias_per_row"] for g in gemm) == 1 and sum(g["a_stride0"] for g in gemm) == 1      # V^T: the expanded weight, bias per row
        assert sum(g["a_strided"] for g in gemm) == 1 and gemm[-1]["resid"]                                # the scores read the q | k halves in place
    else:
        assert len(small) == 1 and len(conv) == 1 and len(gn) == 1 and gn[0]["eps"] == R.EPS_VAE
    return "two_pass", None


_RESULTS = {}


def _case_result(dev, cid, tile=None):
    """(output on the CPU, stats, stats_rows) of a case, run once per (case, forced tile)."""
    from pbe_amd import ops
    key = (cid, tile)
    if key not in _RESULTS:
        r = R.refs(cid)
        try:
            if tile is not None:
                ops.tune(1, tile)
            with torch.no_grad(), _Recorded() as rec:
                y = _run(r.c, _module(r.c, r.sd, dev), r.inp, dev)
            torch.cuda.synchronize()
        finally:
            if tile is not None:
                ops.tune(1, -1)
        stats, rows = _check_launches(r.c, rec)
        _RESULTS[key] = (y.cpu(), stats, rows)
    return _RESULTS[key]


def _judge(cid, y, stats, rows, what=""):
    r = R.refs(cid)
    assert tuple(y.shape) == tuple(r.ref64().shape), (cid, tuple(y.shape))
    ok, text = r.verdict(y, stats, rows)
    report(f"convgate gpu  {cid + what:40s} {stats:8s} rows {rows or '-':>4}: {text}")
    return ok, text


@pytest.mark.parametrize("cid", IDS)
def test_case_against_ref64(dev, cid):
    y, stats, rows = _case_result(dev, cid)
    ok, text = _judge(cid, y, stats, rows)
    assert ok, (cid, text)


@pytest.mark.parametrize("cid", FORCED_CASES)
def test_forced_tile_case_takes_the_conv_statistics(dev, cid):
    """U-Net ResBlocks under the forced 64-row tile without split-K: a tile is one 8x8 image or a quarter of a 16x16 one, so conv 1
    leaves the second norm's statistics (one and four partials per sample) and pbe_groupnorm_apply_f16 runs - on the flat case with eps
    deciding rstd.  (At B = 3 the planner splits K on conv 1 of every ResBlock case but res-1x1-64to128-16x16-unit, and a split-K launch
    leaves no statistics.)"""
    y, stats, rows = _case_result(dev, cid, FORCED_TILE)
    assert (stats, rows) == ("conv", 64)
    ok, text = _judge(cid, y, stats, rows, " [tile 6]")
    assert ok, text


def test_both_groupnorm_routes_occur(dev):
    """Across the U-Net ResBlock cases (and the forced-tile ones) the second norm ran on the conv's partials and as the two-pass kernel."""
    routes = {}
    for c in R.CASES:
        if c["kind"] == "res":
            routes[c["id"]] = _case_result(dev, c["id"])[1:]
    for cid in FORCED_CASES:
        routes[cid + " [tile 6]"] = _case_result(dev, cid, FORCED_TILE)[1:]
    for cid, (stats, rows) in routes.items():
        report(f"convgate gpu  route {cid:40s}: {stats} rows {rows or '-'}")
    assert {s for s, _ in routes.values()} == {"conv", "two_pass"}, routes


def test_concat_resblock_is_batch_independent(dev):
    """B = 3 equals the three single-sample runs bit for bit under the same forced tile (no split-K: one summation order)."""
    from pbe_amd import ops
    r = R.refs(FORCED_CASE)
    whole = _case_result(dev, FORCED_CASE, FORCED_TILE)[0]
    m = _module(r.c, r.sd, dev)
    try:
        ops.tune(1, FORCED_TILE)
        with torch.no_grad():
            for b in range(r.c["B"]):
                one = m.run(r.inp["x"][b:b + 1].to(dev), r.inp["emb_out"][b:b + 1].to(dev), r.inp["skip"][b:b + 1].to(dev)).cpu()
                assert torch.equal(one[0], whole[b]), b
    finally:
        ops.tune(1, -1)


def test_positive_control_eps2_on_the_product_module(dev):
    """out_layers.0 of the product ResBlock set to the VAE's eps: the verdict rejects the run on the flat case, and accepts it again once
    the module is restored."""
    r = R.refs(CONTROL_CASE)
    m = _module(r.c, r.sd, dev)
    norm = m.out_layers[0]
    keep = norm.eps
    try:
        norm.eps = R.EPS_VAE
        m.invalidate_packs()
        with torch.no_grad(), _Recorded() as rec:
            bad = _run(r.c, m, r.inp, dev).cpu()
        stats, rows = _check_launches_control(r.c, rec)
    finally:
        norm.eps = keep
        m.invalidate_packs()
    ok, text = _judge(CONTROL_CASE, bad, stats, rows, " [eps2 1e-6]")
    assert not ok, text
    with torch.no_grad():
        good = _run(r.c, m, r.inp, dev).cpu()
    ok, text = _judge(CONTROL_CASE, good, stats, rows, " [restored]")
    assert ok, text


def _check_launches_control(c, rec):
    gn, conv = rec.of("groupnorm"), rec.of("conv3x3")
    assert [g["eps"] for g in gn] == [R.EPS_UNET, R.EPS_VAE]          # the planted eps reached the second launch
    HW = c["hw"][0] * c["hw"][1]
    return ("conv", HW // conv[0]["out_blocks"]) if conv[0]["out_blocks"] else ("two_pass", None)
