"""Gate of the conv-side block chains one level above the kernels: the U-Net ResBlock (identity skip, 1x1 skip, concat input), Upsample,
Downsample, input conv and output head, and the VAE ResnetBlock (with and without nin_shortcut), AttnBlock, Downsample, Upsample and the
encoder / decoder heads.  Helpers imported by test_convgate_cpu.py and test_convgate_gpu.py.  Not a conftest: plain functions only, CPU
tensors, no product code.

Everything works from a state dict with the names of ldm/modules/diffusionmodules/openaimodel.py and model.py (one block per dict, no
prefix) and the inputs as sent: NHWC tensors holding fp16 values (x, the concat partner skip, the embedding rows emb_out [B, Cout]).

plain(c, sd, inp)     the fp64 block, nothing rounded (the upsampling conv literally: nearest 2x, then 3x3).  Pinned on the CPU to
                      oracle/pbe_oracle.py at fp32 accuracy; for the concat ResBlock the oracle takes cat([x, skip], channel).
ref64(c, sd, inp)     the same block in exact fp64 with ONLY the weight roundings the packs perform: conv and linear weights to fp16
                      (ops.pack_conv3x3, ops.pack_linear), the upsampling conv's four phase weight sets summed in fp32 and THEN rounded
                      (ops.pack_conv3x3_up_phases).  round_conv / phase_weights / round_linear hold the values, packed_conv3x3 /
                      packed_up_phases / packed_linear put them in the packers' K order; test_convgate_cpu.py pins each bit for bit.
emulate(c, sd, inp, reverse=, stats=, stats_rows=, fault=)
                      the chain as the GPU runs it in plain fp32 torch (never a kernel's own output): fp32 accumulation and an fp16
                      rounding at every point where the path stores fp16 -
    U-Net ResBlock    GroupNorm+SiLU of x (| skip) -> fp16 (one tensor of C1 + C2 channels); conv 1 + bias + embedding row -> fp16, ONE
                      rounding; GroupNorm+SiLU -> fp16; the 1x1 shortcut GEMM over [x | skip] + bias -> fp16; conv 2 + bias -> fp16 (the
                      tile staged in LDS), + shortcut in fp32 -> fp16 again (the double store tilecheck.py models).
    VAE ResnetBlock   the same without the embedding row; nin_shortcut is a one-source GEMM.
    Upsample / Downsample / U-Net input conv      conv + bias -> fp16.
    U-Net output head GroupNorm+SiLU -> fp16; conv C -> 4 + bias -> fp16.
    VAE heads         conv_in + bias -> fp16; GroupNorm+swish -> fp16; conv_out + bias -> fp16.
    VAE AttnBlock     GroupNorm -> fp16; q | k = hn Wqk^T + b -> fp16; V^T = Wv hn^T + b (per row) -> fp16; raw scores q k^T -> fp16;
                      probabilities (accgate.softmax_emulate, scale C^-1/2) -> fp16; P V -> fp16; proj_out + bias -> fp16, + x -> fp16.
                      reverse=True sums every K in the opposite order (another valid fp32 order, as accgate.attn_emulate's flag); an
                      int sums K in a permutation seeded by it (a third order: the CPU test of the verdict's peak margin).
                      stats: the statistics of the U-Net ResBlock's SECOND GroupNorm - "conv": fp32 (sum, sumsq) of the stored fp16
                      conv output per block of stats_rows rows (the conv tile's rows, HW / blocks), the blocks' partials met in fp64
                      (pbe_groupnorm_apply_f16 on the conv's group_stats partials); "two_pass": the two-pass kernel's blocks
                      (accgate.gn_geometry).  Both through accgate.gn_emulate.  Every other norm is two-pass.
verdict(got, plain64, ref64, emu_fwd, emu_rev, unit_scale)   the gate; PEAK, REL_L2_FACTOR and BLOCK_TOL are its only constants and none
                      is fitted to a run.
CASES                 what both test files run.  Recipes: unit (randn), offset (channel means +-6 over std 1, fp16-exact: the
                      cancellation case), flat (3e-3 randn: a group variance near eps, so eps decides rstd; the parameters that feed a
                      LATER norm of the block - conv 1 with its bias and the embedding rows, the VAE heads' conv_in bias - are scaled by
                      FLAT_W too, or that norm would see a unit-variance map whatever the input), hole (VAE encoder head: a flat picture
                      that is exactly 0 over a rectangle).  flat / hole skip the BLOCK_TOL term (unit_scale=False).
FAULTS                wiring faults planted in the emulation only; test_convgate_cpu.py demands that the verdict rejects each.
"""
from __future__ import annotations

import math
import zlib

import torch
import torch.nn.functional as F

import accgate as ag
from accgate import REL_L2_FACTOR, rel_l2  # noqa: F401  (re-exported)

BLOCK_TOL = 2e-3            # tests/test_model_gpu.py: one fp16 block against its reference module
PEAK = 2.0                  # per-channel peak error against the larger of the two emulated orders (the device's is a third order)
EMB = 32                    # emb_channels of the ResBlock cases
FLAT, FLAT_W = 3e-3, 2.0 ** -7
B = 3
EPS_UNET, EPS_VAE = 1e-5, 1e-6

KINDS = ("res", "unet_up", "unet_down", "unet_out", "unet_in", "vres", "vattn", "vdown", "vup", "venc", "vdec")

# name -> (kinds it applies to, forms or None for every form, what is wired wrongly)
FAULTS = {
    "eps1 1e-6": (("res",), None, "in_layers.0 runs with the VAE's eps"),
    "eps2 1e-6": (("res",), None, "out_layers.0 runs with the VAE's eps"),
    "eps_o 1e-6": (("unet_out",), None, "the output head's norm runs with the VAE's eps"),
    "norm1 eps 1e-5": (("vres",), None, "norm1 runs with the U-Net's eps"),
    "norm2 eps 1e-5": (("vres",), None, "norm2 runs with the U-Net's eps"),
    "norm eps 1e-5": (("vattn",), None, "the AttnBlock's norm runs with the U-Net's eps"),
    "norm_out eps 1e-5": (("venc", "vdec"), None, "norm_out runs with the U-Net's eps"),
    "emb row of the next sample": (("res",), None, "the embedding row of sample b + 1 used for sample b"),
    "emb row after the second SiLU": (("res",), None, "the embedding row added after SiLU(out_layers.0) instead of before the norm"),
    "concat swapped in GroupNorm": (("res",), ("cat",), "GroupNorm reads the pair as skip | x"),
    "concat swapped in conv 1": (("res",), ("cat",), "conv 1 takes the normalised concat as skip | x"),
    "concat swapped in the shortcut": (("res",), ("cat",), "the two-source shortcut GEMM reads skip | x"),
    "shortcut without its second source": (("res",), ("cat",), "the shortcut GEMM runs over x alone (K = C1)"),
    "residual from the normalised input": (("res", "vres"), None, "the residual (or the shortcut's input) is GroupNorm+SiLU(x), not x"),
    "second norm's statistics before the row vector": (("res",), None, "out_layers.0 normalises conv 1 + row vector with the statistics of conv 1 alone"),
    "no SiLU on norm 1": (("res", "vres"), None, "the first norm without SiLU"),
    "no SiLU on norm 2": (("res", "vres"), None, "the second norm without SiLU"),
    "no SiLU on the head norm": (("unet_out", "venc", "vdec"), None, "the head's norm without SiLU"),
    "VAE Downsample padded (1,0,1,0)": (("vdown",), None, "the asymmetric pad on the wrong sides"),
    "U-Net Downsample with the VAE's pad": (("unet_down",), None, "pad (0,1,0,1) instead of 1 all round"),
    "upsampling phases exchanged": (("unet_up", "vup"), None, "the weight sets of phases (0, 1) and (1, 0) exchanged"),
    "nearest-2x shifted by one source pixel": (("unet_up", "vup"), None, "every phase reads one source column to the left"),
    "attn scale (2C)^-1/2": (("vattn",), None, "the softmax scale of the q | k width"),
    "attn softmax over queries": (("vattn",), None, "the probabilities normalised along the query axis"),
    "attn V^T bias per column": (("vattn",), None, "V^T's bias indexed by the token instead of the channel"),
    "attn k from the q columns": (("vattn",), None, "both score operands are the q half of q | k"),
    "attn residual missing": (("vattn",), None, "proj_out without + x"),
    "conv_out bias of the neighbouring channel": (("venc", "vdec"), None, "conv_out's bias shifted by one channel"),
}


def fault_applies(name, c):
    kinds, forms, _ = FAULTS[name]
    return c["kind"] in kinds and (forms is None or c["form"] in forms)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _case(kind, form, C, Cout, hw, recipe, C2=0, qk=1.0):
    cid = f"{kind}-{form}-{C}" + (f"+{C2}" if C2 else "") + f"to{Cout}-{hw[0]}x{hw[1]}-{recipe}" + ("-peaked" if qk != 1.0 else "")
    return dict(id=cid, kind=kind, form=form, C=C, C2=C2, Cout=Cout, hw=hw, B=B, recipe=recipe, qk=qk, seed=zlib.crc32(cid.encode()) & 0x7FFFFFFF)


CASES = [
    _case("res", "id", 64, 64, (8, 8), "unit"), _case("res", "id", 128, 128, (12, 8), "offset"), _case("res", "id", 64, 64, (16, 16), "flat"),
    _case("res", "1x1", 64, 128, (8, 8), "offset"), _case("res", "1x1", 128, 64, (16, 16), "unit"), _case("res", "1x1", 64, 128, (12, 8), "flat"),
    _case("res", "1x1", 64, 128, (16, 16), "unit"),       # conv 1 plans a 256-row tile without split-K here: the conv leaves the second norm's statistics
    _case("res", "cat", 128, 128, (8, 8), "unit", C2=64), _case("res", "cat", 128, 128, (12, 8), "flat", C2=64),
    _case("res", "cat", 128, 128, (16, 16), "offset", C2=64), _case("res", "cat", 128, 128, (8, 8), "flat", C2=64),
    _case("unet_up", "phase", 64, 64, (8, 6), "unit"), _case("unet_up", "phase", 128, 128, (8, 6), "offset"),
    _case("unet_down", "s2p1", 64, 64, (16, 16), "unit"), _case("unet_down", "s2p1", 128, 128, (16, 16), "offset"),
    _case("unet_out", "head", 64, 4, (8, 8), "unit"), _case("unet_out", "head", 128, 4, (12, 8), "flat"), _case("unet_out", "head", 64, 4, (16, 16), "offset"),
    _case("unet_in", "small", 9, 64, (12, 8), "unit"), _case("unet_in", "small", 9, 128, (8, 8), "offset"),
    _case("vres", "id", 64, 64, (8, 8), "unit"), _case("vres", "id", 128, 128, (16, 16), "flat"), _case("vres", "id", 128, 128, (12, 8), "offset"),
    _case("vres", "nin", 64, 128, (12, 8), "flat"), _case("vres", "nin", 128, 64, (16, 16), "unit"),
    _case("vattn", "attn", 64, 64, (12, 8), "unit"), _case("vattn", "attn", 128, 128, (16, 16), "unit"), _case("vattn", "attn", 64, 64, (16, 16), "unit", qk=3.0),
    _case("vattn", "attn", 128, 128, (12, 8), "flat"), _case("vattn", "attn", 64, 64, (12, 8), "offset"),
    _case("vdown", "p0101", 64, 64, (15, 13), "unit"), _case("vdown", "p0101", 128, 128, (15, 13), "offset"),
    _case("vup", "phase", 64, 64, (8, 6), "unit"), _case("vup", "phase", 128, 128, (8, 6), "offset"),
    _case("venc", "head", 3, 8, (16, 16), "hole", C2=64), _case("venc", "head", 3, 8, (12, 8), "unit", C2=128),
    _case("vdec", "head", 4, 3, (8, 8), "unit", C2=64), _case("vdec", "head", 4, 3, (12, 8), "flat", C2=128),
]
# (venc / vdec: C2 is the heads' inner width - conv_in C -> C2, norm_out over C2, conv_out C2 -> Cout)


def case_by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def unit_scale(c):
    return c["recipe"] in ("unit", "offset")


def shapes(c):
    """{parameter name: shape} of the block's state dict (names of openaimodel.py / model.py)."""
    kind, C, C2, Co = c["kind"], c["C"], c["C2"], c["Cout"]
    out = {}

    def conv(n, co, ci, k=3):
        out[n + ".weight"], out[n + ".bias"] = (co, ci, k, k), (co,)

    def norm(n, ch):
        out[n + ".weight"], out[n + ".bias"] = (ch,), (ch,)
    if kind == "res":
        norm("in_layers.0", C + C2); conv("in_layers.2", Co, C + C2)
        out["emb_layers.1.weight"], out["emb_layers.1.bias"] = (Co, EMB), (Co,)
        norm("out_layers.0", Co); conv("out_layers.3", Co, Co)
        if c["form"] != "id":
            conv("skip_connection", Co, C + C2, 1)
    elif kind in ("unet_up", "vup", "vdown"):
        conv("conv", Co, C)
    elif kind == "unet_down":
        conv("op", Co, C)
    elif kind == "unet_out":
        norm("out.0", C); conv("out.2", Co, C)
    elif kind == "unet_in":
        conv("input_blocks.0.0", Co, C)
    elif kind == "vres":
        norm("norm1", C); conv("conv1", Co, C); norm("norm2", Co); conv("conv2", Co, Co)
        if c["form"] == "nin":
            conv("nin_shortcut", Co, C, 1)
    elif kind == "vattn":
        norm("norm", C)
        for n in ("q", "k", "v", "proj_out"):
            conv(n, C, C, 1)
    else:
        conv("conv_in", C2, C); norm("norm_out", C2); conv("conv_out", Co, C2)
    return out


# parameters the flat / hole recipes scale by FLAT_W, so that the norm they feed meets a flat map too (module docstring)
_FLAT_FEEDERS = {"res": ("in_layers.2.", "emb_layers.1."), "vres": ("conv1.",), "venc": ("conv_in.bias",), "vdec": ("conv_in.bias",)}


def state_dict(c):
    """The block's fp32 parameters from a CPU generator seeded by the case: matrices and kernels at 1 / sqrt(fan-in), norm gains 1 + 0.1
    randn, biases 0.1 randn.  Nothing is left at zero (out_layers.3 and out.2 are zero_module in the product)."""
    g = torch.Generator().manual_seed(c["seed"])
    sd = {}
    for name, shape in shapes(c).items():
        r = torch.randn(shape, generator=g)
        if len(shape) > 1:
            sd[name] = r / math.sqrt(r[0].numel())
        elif name.endswith("weight"):
            sd[name] = 1.0 + 0.1 * r
        else:
            sd[name] = 0.1 * r
    if c["qk"] != 1.0:
        sd["q.weight"] *= c["qk"]
        sd["k.weight"] *= c["qk"]
    if c["recipe"] in ("flat", "hole"):
        for name in sd:
            if name.startswith(_FLAT_FEEDERS.get(c["kind"], ())):
                sd[name] = sd[name] * FLAT_W
    return sd


def _draw(recipe, shape, g):
    x = torch.randn(shape, generator=g)
    if recipe == "offset":
        x = x + 6.0 * (torch.randint(0, 2, (shape[-1],), generator=g).float() * 2 - 1)
    elif recipe == "flat":
        x = FLAT * x
    elif recipe == "hole":
        x = FLAT_W * x
        h, w = shape[1], shape[2]
        x[:, h // 8:h - h // 8, w // 8:w - w // 4] = 0.0
    return x.half()


def inputs(c, sd=None):
    """dict(x, skip, emb, emb_out): NHWC fp16 x (and skip for the concat form); emb [B, EMB] fp32 with a distinct row per sample and
    emb_out = fp16(Linear(SiLU(emb))) computed in fp64, the rows ResBlock.run takes."""
    g = torch.Generator().manual_seed(c["seed"] ^ 0x5A5A5A)
    H, W = c["hw"]
    inp = dict(x=_draw(c["recipe"], (c["B"], H, W, c["C"]), g), skip=None, emb=None, emb_out=None)
    if c["kind"] == "res":
        if c["form"] == "cat":
            inp["skip"] = _draw(c["recipe"], (c["B"], H, W, c["C2"]), g)
        inp["emb"] = torch.randn(c["B"], EMB, generator=g)
        inp["emb_out"] = emb_rows64(sd if sd is not None else state_dict(c), inp["emb"]).half()
    return inp


def emb_rows64(sd, emb):
    e = emb.double()
    return (e / (1 + torch.exp(-e))) @ sd["emb_layers.1.weight"].double().t() + sd["emb_layers.1.bias"].double()


# ---- the packs, restated --------------------------------------------------------------------------------------------------------------------
def round_conv(w):
    """The values ops.pack_conv3x3 keeps of an OIHW weight: fp16."""
    return w.detach().float().half()


def round_linear(w):
    """The values ops.pack_linear keeps: [N, K] fp16."""
    return w.detach().float().reshape(w.shape[0], -1).half()


def phase_weights(w):
    """The values ops.pack_conv3x3_up_phases keeps: per output phase py * 2 + px a 2x2 kernel [Cout, Cin, 2, 2] whose taps are the 3x3 taps
    that fall on one source pixel, summed in fp32 (ky outer, kx inner, from 0) and rounded to fp16 once."""
    w32 = w.detach().float()
    sets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    out = []
    for py in (0, 1):
        for px in (0, 1):
            k = torch.zeros(w.shape[0], w.shape[1], 2, 2)
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = 0
                    for ky in sets[py][ty]:
                        for kx in sets[px][tx]:
                            acc = acc + w32[:, :, ky, kx]
                    k[:, :, ty, tx] = acc
            out.append(k.half())
    return out


def packed_conv3x3(w, cin_pad=None):
    """round_conv(w) in ops.pack_conv3x3's K order: k = ((ci // 64) * 9 + tap) * 64 + ci % 64, or with cin_pad (the small-Cin path)
    k = tap * cin_pad + ci, zero-padded channels."""
    r = round_conv(w)
    co, ci = r.shape[:2]
    taps = r.permute(0, 2, 3, 1).reshape(co, 9, ci)
    if cin_pad is not None:
        out = torch.zeros(co, 9, cin_pad, dtype=torch.float16)
        out[:, :, :ci] = taps
        return out.reshape(co, 9 * cin_pad)
    return taps.reshape(co, 9, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, 9 * ci).contiguous()


def packed_up_phases(w):
    """phase_weights(w) in ops.pack_conv3x3_up_phases' layout [4, Cout, 4 Cin]: k = ((ci // 64) * 4 + ty * 2 + tx) * 64 + ci % 64."""
    out = []
    for k in phase_weights(w):
        co, ci = k.shape[:2]
        out.append(k.permute(0, 2, 3, 1).reshape(co, 4, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, 4 * ci))
    return torch.stack(out, 0).contiguous()


def packed_linear(w):
    return round_linear(w).contiguous()


# ---- the arithmetic of one chain in three precisions ----------------------------------------------------------------------------------------
def _silu(x):
    return x / (1 + torch.exp(-x))


class _Arith:
    """mode "plain" (fp64, nothing rounded), "ref64" (fp64, pack roundings only) or "emu" (fp32, every store rounded; reverse, stats,
    fault as in the module docstring)."""

    def __init__(self, mode, reverse=False, stats="two_pass", stats_rows=None, fault=None):
        assert mode in ("plain", "ref64", "emu") and stats in ("conv", "two_pass") and (fault is None or fault in FAULTS)
        self.mode, self.reverse, self.stats, self.stats_rows, self.fault = mode, reverse, stats, stats_rows, fault if mode == "emu" else None
        self.dt = torch.float32 if mode == "emu" else torch.float64

    def t(self, x):
        return x.to(self.dt)

    def w(self, w):                                   # a packed weight's values
        return self.t(w) if self.mode == "plain" else self.t(w.detach().float().half())

    def r(self, x):                                   # an fp16 store
        return x.half().float() if self.mode == "emu" else x

    def mm(self, a, w):
        """a [.., K] @ w [N, K]^T."""
        if self.reverse is True:
            a, w = a.flip(-1), w.flip(-1)
        elif self.reverse is not False:               # an int: K in a seeded permutation (a third order, for the CPU test of the peak margin)
            perm = torch.randperm(a.shape[-1], generator=torch.Generator().manual_seed(int(self.reverse)))
            a, w = a[..., perm], w[..., perm]
        return a @ w.transpose(-1, -2)

    def conv(self, x, w, pad4=(1, 1, 1, 1), stride=1):
        """NHWC x, OIHW w (already in this arithmetic's dtype); pad4 = (left, right, top, bottom)."""
        k = w.shape[-1]
        xn = F.pad(x.permute(0, 3, 1, 2), pad4)
        Ho, Wo = (xn.shape[2] - k) // stride + 1, (xn.shape[3] - k) // stride + 1
        cols = F.unfold(xn, k, stride=stride).transpose(1, 2)             # [B, L, C k k]
        return self.mm(cols, w.reshape(w.shape[0], -1)).reshape(x.shape[0], Ho, Wo, w.shape[0])

    def gn(self, x, sd, name, eps, silu, rows=None, stats_of=None):
        """GroupNorm(32)(+SiLU) of NHWC x -> stored fp16.  rows: rows per fp32 partial (default: the two-pass kernel's); stats_of: the
        tensor the statistics are taken from (a fault)."""
        Bn, H, W, C = x.shape
        g, b = sd[name + ".weight"], sd[name + ".bias"]
        if self.mode != "emu":
            xg = x.reshape(Bn, H * W, 32, C // 32)
            mean = xg.mean((1, 3), keepdim=True)
            d = xg - mean
            y = (d / torch.sqrt((d * d).mean((1, 3), keepdim=True) + eps)).reshape(Bn, H, W, C) * g.double() + b.double()
            return _silu(y) if silu else y
        rows = rows or ag.gn_geometry(H * W, C)[1]
        x16 = x.reshape(Bn, H * W, C).half()
        if stats_of is None:
            return ag.gn_emulate(x16, g, b, eps, silu, rows).float().reshape(Bn, H, W, C)
        return _gn_emulate_stats_of(stats_of.reshape(Bn, H * W, C).half(), x16, g, b, eps, silu, rows).float().reshape(Bn, H, W, C)


def _gn_emulate_stats_of(xs, x, gamma, beta, eps, silu, rows, groups=32):
    """accgate.gn_emulate with the statistics of xs applied to x (the fault "second norm's statistics before the row vector")."""
    Bn, HW, C = x.shape
    cg = C // groups
    sf, xf = xs.float().view(Bn, HW, groups, cg), x.float().view(Bn, HW, groups, cg)
    ta = torch.zeros(Bn, 1, groups, 1, dtype=torch.float64)
    tq = torch.zeros_like(ta)
    for r0 in range(0, HW, rows):
        blk = sf[:, r0:r0 + rows]
        ta += blk.sum((1, 3), keepdim=True, dtype=torch.float32).double()
        tq += (blk * blk).sum((1, 3), keepdim=True, dtype=torch.float32).double()
    n = float(HW * cg)
    mean = ta / n
    var = (tq / n - mean * mean).clamp_min(0.0)
    mu, rstd = mean.float(), (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float()
    sc = rstd * gamma.float().view(1, 1, groups, cg)
    f = xf * sc + (beta.float().view(1, 1, groups, cg) - mu * sc)
    if silu:
        f = f * (1.0 / (1.0 + torch.exp2(-ag.LOG2E * f)))
    return f.half().view(Bn, HW, C)


def _bias(A, sd, name):
    return A.t(sd[name + ".bias"])


def _res(A, c, sd, inp, vae):
    """U-Net ResBlock.run / VAE ResnetBlock.run."""
    f = A.fault
    n1, c1, n2, c2, sk = ("norm1", "conv1", "norm2", "conv2", "nin_shortcut") if vae else \
        ("in_layers.0", "in_layers.2", "out_layers.0", "out_layers.3", "skip_connection")
    e1 = e2 = EPS_VAE if vae else EPS_UNET
    if f in ("eps1 1e-6", "norm1 eps 1e-5"):
        e1 = EPS_UNET if vae else EPS_VAE
    if f in ("eps2 1e-6", "norm2 eps 1e-5"):
        e2 = EPS_UNET if vae else EPS_VAE
    x, skip = A.t(inp["x"]), None if inp["skip"] is None else A.t(inp["skip"])
    C1 = x.shape[-1]
    pair = x if skip is None else torch.cat([x, skip], -1)
    swapped = None if skip is None else torch.cat([skip, x], -1)
    h1 = A.gn(swapped if f == "concat swapped in GroupNorm" else pair, sd, n1, e1, f != "no SiLU on norm 1")
    a1 = torch.cat([h1[..., C1:], h1[..., :C1]], -1) if f == "concat swapped in conv 1" else h1
    acc = A.conv(a1, A.w(sd[c1 + ".weight"])) + _bias(A, sd, c1)
    if vae:
        h = A.r(acc)
        h2 = A.gn(h, sd, n2, e2, f != "no SiLU on norm 2")
    else:
        emb = A.t(inp["emb_out"])
        if f == "emb row of the next sample":
            emb = emb.roll(-1, 0)
        rv = emb[:, None, None, :]
        HW = x.shape[1] * x.shape[2]
        rows = (A.stats_rows or 64) if A.stats == "conv" else None
        assert rows is None or HW % rows == 0, "the conv's statistics come in whole tiles of one sample"
        if f == "emb row after the second SiLU":
            h = A.r(acc)
            h2 = A.r(A.gn(h, sd, n2, e2, True, rows) + rv)
        elif f == "second norm's statistics before the row vector":
            h = A.r(acc + rv)
            h2 = A.gn(h, sd, n2, e2, True, rows, stats_of=A.r(acc))
        else:
            h = A.r(acc + rv)                                              # bias + row vector in the fp32 epilogue: one rounding
            h2 = A.gn(h, sd, n2, e2, f != "no SiLU on norm 2", rows)
    src = pair
    if f == "residual from the normalised input":
        src = h1
    elif f == "concat swapped in the shortcut":
        src = swapped
    if sk + ".weight" in sd:
        ws = A.w(sd[sk + ".weight"]).reshape(sd[sk + ".weight"].shape[0], -1)
        if f == "shortcut without its second source":
            src, ws = src[..., :C1], ws[:, :C1]
        xs = A.r(A.mm(src, ws) + _bias(A, sd, sk))
    else:
        xs = src
    y = A.r(A.conv(h2, A.w(sd[c2 + ".weight"])) + _bias(A, sd, c2))        # the tile as staged in fp16 ...
    return A.r(y + xs)                                                     # ... and stored again after the residual add


def _up(A, c, sd, inp):
    x = A.t(inp["x"])
    w, b = sd["conv.weight"], _bias(A, sd, "conv")
    if A.mode == "plain":
        return A.conv(x.repeat_interleave(2, 1).repeat_interleave(2, 2), A.t(w)) + b
    pw = phase_weights(w)
    if A.fault == "upsampling phases exchanged":
        pw[1], pw[2] = pw[2], pw[1]
    shift = 1 if A.fault == "nearest-2x shifted by one source pixel" else 0
    Bn, H, W, _ = x.shape
    out = x.new_zeros(Bn, 2 * H, 2 * W, w.shape[0])
    for py in (0, 1):
        for px in (0, 1):                             # output (2y + py, 2x + px) reads source rows {y - 1 + py, y + py}, columns {x - 1 + px, x + px}
            out[:, py::2, px::2] = A.conv(x, A.t(pw[py * 2 + px]), (1 - px + shift, px - shift, 1 - py, py))
    return A.r(out + b)


def _conv_block(A, sd, name, x, pad4, stride=1):
    return A.r(A.conv(x, A.w(sd[name + ".weight"]), pad4, stride) + _bias(A, sd, name))


def _head(A, sd, x, norm, conv, eps, fault_eps):
    f = A.fault
    h = A.gn(x, sd, norm, fault_eps if f in ("eps_o 1e-6", "norm_out eps 1e-5") else eps, f != "no SiLU on the head norm")
    b = _bias(A, sd, conv)
    if f == "conv_out bias of the neighbouring channel":
        b = b.roll(1)
    return A.r(A.conv(h, A.w(sd[conv + ".weight"])) + b)


def _vattn(A, c, sd, inp):
    f = A.fault
    x = A.t(inp["x"])
    Bn, H, W, C = x.shape
    N = H * W
    wl = lambda n: A.w(sd[n + ".weight"]).reshape(C, C)      # noqa: E731
    x2 = x.reshape(Bn, N, C)
    hn = A.gn(x, sd, "norm", EPS_UNET if f == "norm eps 1e-5" else EPS_VAE, False).reshape(Bn, N, C)
    q = A.r(A.mm(hn, wl("q")) + _bias(A, sd, "q"))
    k = A.r(A.mm(hn, wl("k")) + _bias(A, sd, "k"))
    bv = _bias(A, sd, "v")
    bv = bv[torch.arange(N) % C][None, None, :] if f == "attn V^T bias per column" else bv[None, :, None]
    vt = A.r(A.mm(wl("v")[None], hn) + bv)                                 # [B, C, N]
    s = A.r(A.mm(q, q if f == "attn k from the q columns" else k))         # raw scores, stored fp16
    scale = float(int(2 * C if f == "attn scale (2C)^-1/2" else C) ** -0.5)
    if f == "attn softmax over queries":
        s = s.transpose(1, 2)
    pr = ag.softmax_emulate(s.half(), scale).float() if A.mode == "emu" else torch.softmax(s * scale, -1)
    if f == "attn softmax over queries":
        pr = pr.transpose(1, 2)
    o = A.r(A.mm(pr, vt))                                                  # [B, N, C]
    y = A.r(A.mm(o, wl("proj_out")) + _bias(A, sd, "proj_out"))
    return (y if f == "attn residual missing" else A.r(y + x2)).reshape(Bn, H, W, C)


def _run(A, c, sd, inp):
    kind = c["kind"]
    if kind in ("res", "vres"):
        return _res(A, c, sd, inp, kind == "vres")
    if kind in ("unet_up", "vup"):
        return _up(A, c, sd, inp)
    if kind == "vattn":
        return _vattn(A, c, sd, inp)
    x = A.t(inp["x"])
    if kind == "unet_down":
        return _conv_block(A, sd, "op", x, (0, 1, 0, 1) if A.fault == "U-Net Downsample with the VAE's pad" else (1, 1, 1, 1), 2)
    if kind == "vdown":
        return _conv_block(A, sd, "conv", x, (1, 0, 1, 0) if A.fault == "VAE Downsample padded (1,0,1,0)" else (0, 1, 0, 1), 2)
    if kind == "unet_in":
        return _conv_block(A, sd, "input_blocks.0.0", x, (1, 1, 1, 1))
    if kind == "unet_out":
        return _head(A, sd, x, "out.0", "out.2", EPS_UNET, EPS_VAE)
    assert kind in ("venc", "vdec"), kind
    return _head(A, sd, _conv_block(A, sd, "conv_in", x, (1, 1, 1, 1)), "norm_out", "conv_out", EPS_VAE, EPS_UNET)


def plain(c, sd, inp):
    """fp64 [B, Ho, Wo, Cout], nothing rounded."""
    return _run(_Arith("plain"), c, sd, inp)


def ref64(c, sd, inp):
    """fp64, only the packs' weight roundings."""
    return _run(_Arith("ref64"), c, sd, inp)


def emulate(c, sd, inp, reverse=False, stats="two_pass", stats_rows=None, fault=None):
    """The chain as the GPU runs it -> fp16 [B, Ho, Wo, Cout] (module docstring)."""
    assert fault is None or fault_applies(fault, c), (fault, c["id"])
    return _run(_Arith("emu", reverse, stats, stats_rows, fault), c, sd, inp).half()


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------
def channel_peaks(got, ref, emu_fwd, emu_rev):
    """(E_c [C], the largest max|got - ref| / E_c of a channel, the largest |got - ref| / (PEAK E_c + 2^-11 |ref| + 2^-25) of an element:
    the peak term holds when the last is <= 1)."""
    C = ref.shape[-1]
    r = ref.reshape(-1, C)
    E = torch.maximum((emu_fwd.double().reshape(-1, C) - r).abs().amax(0), (emu_rev.double().reshape(-1, C) - r).abs().amax(0))
    d = (got.double().reshape(-1, C) - r).abs()
    lim = PEAK * E[None] + 2.0 ** -11 * r.abs() + 2.0 ** -25
    return E, (d.amax(0) / E.clamp_min(2.0 ** -40)).max().item(), (d / lim).max().item()


def verdict(got, plain64, ref, emu_fwd, emu_rev, unit_scale):
    """(accepted, text).  Accepts when got is finite, rel_l2(got, ref64) <= REL_L2_FACTOR x the larger rel_l2 of the two emulated orders,
    every element has |got - ref64| <= PEAK E_c + 2^-11 |ref64| + 2^-25 with E_c the largest |emulation - ref64| of its output channel in
    either order, and for the unit-scale cases rel_l2(got, plain64) <= BLOCK_TOL."""
    if not bool(torch.isfinite(got.float()).all()):
        return False, "non-finite result"
    r_got = rel_l2(got, ref)
    r_emu = max(rel_l2(emu_fwd, ref), rel_l2(emu_rev, ref))
    p_got = rel_l2(got, plain64)
    _, peak, excess = channel_peaks(got, ref, emu_fwd, emu_rev)
    ok_l2, ok_peak = r_got <= REL_L2_FACTOR * r_emu, excess <= 1.0
    text = (f"vs ref64 {r_got:.3e} (emulation {r_emu:.3e}, ratio {r_got / max(r_emu, 1e-300):.2f}, limit x{REL_L2_FACTOR}); "
            f"peak max_c |d| / E_c {peak:.2f}, of its limit {excess:.2f}; vs plain {p_got:.3e}")
    ok = ok_l2 and ok_peak
    if unit_scale:
        ok = ok and p_got <= BLOCK_TOL
        text += f" (BLOCK_TOL {BLOCK_TOL:.0e})"
    return ok, text + ("" if ok else f"  REJECTED:{'' if ok_l2 else ' rel-L2'}{'' if ok_peak else ' peak'}{'' if not unit_scale or p_got <= BLOCK_TOL else ' BLOCK_TOL'}")


def rel_l2_terms_accept(got, plain64, ref, emu_fwd, emu_rev, unit_scale):
    """The verdict without its peak term (what a whole-tensor gate alone would say)."""
    ok = rel_l2(got, ref) <= REL_L2_FACTOR * max(rel_l2(emu_fwd, ref), rel_l2(emu_rev, ref))
    return ok and (not unit_scale or rel_l2(got, plain64) <= BLOCK_TOL)


class Refs:
    """State dict, inputs, plain64, ref64 and the emulations of one case, each computed once and never changed."""

    def __init__(self, c):
        self.c, self.sd = c, state_dict(c)
        self.inp = inputs(c, self.sd)
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def plain(self):
        return self._get("plain", lambda: plain(self.c, self.sd, self.inp))

    def ref64(self):
        return self._get("ref64", lambda: ref64(self.c, self.sd, self.inp))

    def emu(self, reverse=False, stats="two_pass", stats_rows=None, fault=None):
        return self._get(("e", reverse, stats, stats_rows, fault),
                         lambda: emulate(self.c, self.sd, self.inp, reverse=reverse, stats=stats, stats_rows=stats_rows, fault=fault))

    def verdict(self, got, stats="two_pass", stats_rows=None):
        return verdict(got, self.plain(), self.ref64(), self.emu(False, stats, stats_rows), self.emu(True, stats, stats_rows), unit_scale(self.c))

    def rel_l2_terms_accept(self, got, stats="two_pass"):
        return rel_l2_terms_accept(got, self.plain(), self.ref64(), self.emu(False, stats), self.emu(True, stats), unit_scale(self.c))


_REFS = {}


def refs(cid):
    if cid not in _REFS:
        _REFS[cid] = Refs(case_by_id(cid))
    return _REFS[cid]
