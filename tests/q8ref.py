"""Quantisation-aware gate of the two opt-in fp8 switches (pbe_amd.precision: linear_fp8, attn_fp8) one level above the kernels: a whole
SpatialTransformer (GroupNorm, proj_in, its BasicTransformerBlocks, proj_out, residual) with a one-token context.  Helpers imported by
test_q8gate_cpu.py, test_q8gate_gpu.py and oracle/gen_q8_golden.py.  Not a conftest: plain functions only, CPU tensors, no product code.

Everything works from a state dict of a SpatialTransformer (names of ldm/modules/attention.py, an optional prefix) and the inputs as sent:
x [B, Hh, Ww, C] NHWC holding fp16 values, context [B, 1, Dc] holding fp16 values.

plain(...)            the fp64 block, nothing rounded.  Pinned to oracle/pbe_oracle.py's spatial_transformer (fp32) on the CPU.
quantised(mode, ...)  mode in MODES: the same block in exact fp64 arithmetic with ONLY the operand quantisations, each a deterministic
                      function of exact values ("q64"):
    linear     LN(x) / row_scale -> e4m3, row_scale = max|LN(x)| / 448 floored at 2^-100 (1 for a zero row); weights -> e4m3 with one
               scale per output channel (the same rule); round to nearest even, saturating (include/pbe_hip.h pbe_layernorm_f8,
               ops.pack_linear_f8).  Covers what BasicTransformerBlock sends through the fp8 LayerNorm: attn1's q | k and V^T and
               ff.net.0.proj.  attn2, both to_out, ff.net.2 and proj_in / proj_out stay unquantised.
    attention  q scale log2(e), k and V^T -> MX-fp8: e4m3 with the smallest power of two s with amax / s <= 448 per 32 elements, along d
               for q and k, along the tokens for V^T (pbe_quant_mx8_f16).  P is NOT rounded here: the kernel rounds exp2(s - m) against
               its deferred maximum m, which is no function of exact values - that rounding belongs to the emulation.
    both       the two together.
emulate(mode, path, ...)  the chain as the GPU runs it in plain fp32 torch (never a kernel's own output): fp32 accumulation, an fp16
                      rounding at every point where the path stores fp16, and per path (BasicTransformerBlock._mode):
    every path stores fp16:   GroupNorm output; proj_in output h; to_v(context) and attn2's constant to_out(to_v(context)) [B, C];
                      the attention core's output; x1 = x + to_out(a) + constant; the GEGLU product value * gelu(gate); the block's
                      output x1 + ff.net.2(...); proj_out(h) + x.  All weights are fp16 (pack_linear) unless e4m3.
    folded            no LayerNorm output exists: q | k | V^T and the GEGLU input are rstd (x (W gamma)^T - mean colsum) + W beta with
                      (W gamma) rounded to fp16, mean / rstd from the fp32 (sum, sumsq) of the STORED fp16 rows; q leaves as
                      fp16(scale log2(e) q) (alpha in the fp32 epilogue); k, V^T fp16.
    plain             LayerNorm output fp16; q | k, V^T fp16 (q unscaled: the d = 40 attention form rounds q scale log2(e) to fp16).
    f8                LayerNorm output e4m3 codes + fp32 row scale (fp32 LayerNorm, scale = amax fl32(1 / 448)); e4m3 weights (the GEGLU
                      projection's from its fp16 pack); a_scale w_scale acc (+ bias) in fp32; q | k, V^T, GEGLU product fp16.
    attention fp16    accgate.attn_emulate (P rounded to fp16).  attention fp8: the fp16 q (x scale log2(e) in fp32 unless the projection
                      applied it), k, V^T quantised to MX-fp8, fp32 scores, P = exp2(s - rowmax) rounded to e4m3 ONCE and shared by the
                      numerator and the denominator, o / l stored fp16.  The MX copy-out (copy_out=True) quantises the fp16 values the
                      projection would have stored, so it is the same arithmetic: the flag is accepted and changes nothing.
verdict(got, plain64, q64, emu)  the gate; no constant is fitted to a run.
FAULTS                wiring faults planted in the emulation that the verdict must reject (test_q8gate_cpu.py).
"""
from __future__ import annotations

import math

import torch

import accgate as ag
import f8ref
from accgate import LOG2E, REL_L2_FACTOR, rel_l2  # noqa: F401  (re-exported)

MODES = ("linear", "attention", "both")
PATHS = ("folded", "plain", "f8")
BLOCK_TOL = 2e-3                      # tests/test_model_gpu.py: one fp16 block against its reference module
OLD_FWD_TOL = {"linear": 5e-2, "attention": 8.5e-3, "both": 7e-2}      # the whole-tensor limits against the PLAIN reference
E4M3_MAX = f8ref.E4M3_MAX
SCALE_FLOOR = f8ref.SCALE_FLOOR
GN_EPS, LN_EPS = 1e-6, 1e-5
# name -> (modes it applies to, what is wired wrongly)
FAULTS = {
    "one A scale for all rows": (("linear", "both"), "per-tensor instead of per-row activation scale"),
    "weights truncated": (("linear", "both"), "e4m3 weights truncated, not rounded to nearest even"),
    "GEGLU scales swapped": (("linear", "both"), "w_scale of the GEGLU projection applied in un-interleaved order"),
    "MX blocks of 64": (("attention", "both"), "the core reads one power-of-two scale per 64 elements of operands quantised per 32"),
    "V^T blocked along d": (("attention", "both"), "the core reads V^T's scales as if its MX blocks ran along d instead of the tokens"),
    "q scale applied twice": (("attention", "both"), "scale log2(e) on q by the projection and again by the quantiser"),
    "q scale not applied": (("attention", "both"), "scale log2(e) never reaches q"),
    "norm3's pack for norm1": (("linear", "both"), "norm1's fp8 LayerNorm runs with norm3's gain and bias"),
    "w_scale of q|k on V^T": (("linear", "both"), "V^T's product dequantised with q's channel scales"),
}


def _lin(mode):
    return mode in ("linear", "both")


def _att(mode):
    return mode in ("attention", "both")


def blocks_of(sd, p=""):
    """Indices of the transformer blocks under prefix p."""
    pre = p + "transformer_blocks."
    return sorted({int(k[len(pre):].split(".")[0]) for k in sd if k.startswith(pre)})


# ---- the quantisers, restated in fp64 (pinned byte for byte to f8ref / mx8ref by test_q8gate_cpu.py) ------------------------------------
def row_scale(t):
    """max|row| / 448 floored at 2^-100, 1 for a zero row; t [..., K] -> [..., 1]."""
    amax = t.abs().amax(-1, keepdim=True)
    return torch.where(amax > 0, (amax / E4M3_MAX).clamp(min=SCALE_FLOOR), torch.ones_like(amax))


def quant_rows(t, rounding="rne", scale=None):
    """(decoded e4m3 values, scale): t / scale rounded to e4m3, one scale per row of the last dim (fp64 in, fp64 out)."""
    s = row_scale(t) if scale is None else scale
    return f8ref.q_e4m3(t / s, rounding), s


def mx_scale(amax):
    """The smallest power of two s with amax / s <= 448 (E8M0: 2^-126 .. 2^127), 1 for amax == 0 (mx8ref.scale_exp)."""
    m, E = torch.frexp(amax)                                    # amax = m 2^E, m in [0.5, 1);  448 = 0.875 2^9
    e = torch.where(m <= 0.875, E - 9, E - 8).clamp(-126, 127).double()
    return torch.where(amax > 0, torch.exp2(e), torch.ones_like(amax))


def mx_quant(t, block=32):
    """(decoded e4m3 values, scales [..., blocks]) of fp64 t with one power-of-two scale per `block` elements of the LAST dim (a ragged last
    block is zero-padded, which changes no amax)."""
    n = t.shape[-1]
    pad = (-n) % block
    v = torch.cat([t, t.new_zeros(*t.shape[:-1], pad)], -1) if pad else t
    v = v.reshape(*t.shape[:-1], -1, block)
    s = mx_scale(v.abs().amax(-1))
    q = f8ref.q_e4m3(v / s[..., None])
    return q.reshape(*t.shape[:-1], n + pad)[..., :n], s


def mx_dequant(t, block=32):
    q, s = mx_quant(t, block)
    n = t.shape[-1]
    pad = (-n) % block
    qq = torch.cat([q, q.new_zeros(*q.shape[:-1], pad)], -1) if pad else q
    return (qq.reshape(*t.shape[:-1], -1, block) * s[..., None]).reshape(*t.shape[:-1], n + pad)[..., :n]


# ---- fp64 pieces ----------------------------------------------------------------------------------------------------------------------
def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ln(x, g, b, eps=LN_EPS):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def _gn(x, g, b, eps=GN_EPS, groups=32):
    """x [B, N, C] tokens x channels; statistics per (sample, group)."""
    B, N, C = x.shape
    xg = x.reshape(B, N, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    d = xg - mean
    y = d / torch.sqrt((d * d).mean((1, 3), keepdim=True) + eps)
    return y.reshape(B, N, C) * g + b


def _heads(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).permute(0, 2, 1, 3)


def attention64(q, k, v, heads, mx):
    """Per-head softmax(q k^T d^-1/2) v in base 2, fp64, one (sample, head) at a time (N = 4096 fits).  mx: q scale log2(e), k (blocks
    along d) and V^T (blocks along the tokens) go through the MX-fp8 quantiser first; P is not rounded."""
    B, N, C = q.shape
    D = C // heads
    c = D ** -0.5 * LOG2E
    out = torch.empty_like(q)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            qh, kh, vh = q[b, :, sl] * c, k[b, :, sl], v[b, :, sl]
            if mx:
                qh, kh, vh = mx_dequant(qh), mx_dequant(kh), mx_dequant(vh.t().contiguous()).t()
            s = qh @ kh.t()
            w = torch.exp2(s - s.max(-1, keepdim=True).values)
            out[b, :, sl] = (w @ vh) / w.sum(-1, keepdim=True)
    return out


def block64(sd, p, h, context, heads, mode=None):
    """One BasicTransformerBlock (names under prefix p) on h [B, N, C] fp64 with a ONE-token context [B, 1, Dc] -> fp64 [B, N, C].
    mode None: plain; else the operand quantisations of that mode.  attn2 over one key is to_out(to_v(context)) exactly."""
    assert context.shape[1] == 1, "the fp8 paths take a one-token context"
    W = lambda n: sd[p + n].double()      # noqa: E731
    lin = _lin(mode)

    def proj(xn, names):
        if lin:
            a, s = quant_rows(xn)
            xn = a * s
        outs = []
        for n in names:
            w = W(n)
            if lin:
                wq, ws = quant_rows(w)
                w = wq * ws
            outs.append(xn @ w.t())
        return outs

    q, k, v = proj(_ln(h, W("norm1.weight"), W("norm1.bias")), ("attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight"))
    a = attention64(q, k, v, heads, _att(mode))
    x1 = h + a @ W("attn1.to_out.0.weight").t() + W("attn1.to_out.0.bias")
    const = (context.double()[:, 0] @ W("attn2.to_v.weight").t()) @ W("attn2.to_out.0.weight").t() + W("attn2.to_out.0.bias")
    x2 = x1 + const[:, None, :]
    hh = proj(_ln(x2, W("norm3.weight"), W("norm3.bias")), ("ff.net.0.proj.weight",))[0] + W("ff.net.0.proj.bias")
    val, gate = hh.chunk(2, -1)
    return x2 + (val * _gelu(gate)) @ W("ff.net.2.weight").t() + W("ff.net.2.bias")


def _chain64(sd, x, context, heads, mode, p=""):
    W = lambda n: sd[p + n].double()      # noqa: E731
    B, Hh, Ww, C = x.shape
    x2 = x.double().reshape(B, Hh * Ww, C)
    h = _gn(x2, W("norm.weight"), W("norm.bias")) @ W("proj_in.weight").reshape(-1, C).t() + W("proj_in.bias")
    for i in blocks_of(sd, p):
        h = block64(sd, f"{p}transformer_blocks.{i}.", h, context, heads, mode)
    y = h @ W("proj_out.weight").reshape(C, -1).t() + W("proj_out.bias") + x2
    return y.reshape(B, Hh, Ww, C)


def plain(sd, x, context, heads, p=""):
    """The fp64 SpatialTransformer: x [B, Hh, Ww, C] NHWC, context [B, 1, Dc] -> fp64 [B, Hh, Ww, C]."""
    return _chain64(sd, x, context, heads, None, p)


def quantised(mode, sd, x, context, heads, p=""):
    """plain() with only the operand quantisations of `mode` (module docstring)."""
    assert mode in MODES, mode
    return _chain64(sd, x, context, heads, mode, p)


# ---- the emulation: what the GPU path does, in fp32 ---------------------------------------------------------------------------------------
def _r16(t):
    return t.half().float()


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def ln8(x, g, b, eps=LN_EPS, per_tensor=False):
    """pbe_layernorm_f8 in fp32 -> (decoded codes fp32 [.., C], scale fp32 [.., 1]): mean from a row sum, centred variance, rsqrt,
    (x - mean) rstd g + b, scale = max(amax fl32(1 / 448), 2^-100) (1 for amax == 0), codes = e4m3(y (1 / scale)).  The restatement of
    f8ref.ln8_emulate (pinned byte for byte).  per_tensor: the fault - one amax for all rows."""
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    y = d * torch.rsqrt((d * d).sum(-1, keepdim=True) / float(C) + eps) * g + b
    amax = y.abs().amax(-1, keepdim=True)
    if per_tensor:
        amax = amax.amax().expand_as(amax)
    scale = torch.where(amax > 0, (amax * _f32(1.0).div(448.0)).clamp(min=SCALE_FLOOR), torch.ones_like(amax))
    return f8ref.q_e4m3((y * (1.0 / scale)).double()).float(), scale


def pack_f8(w, rounding="rne"):
    """ops.pack_linear_f8 on an fp32 weight [N, K] -> (decoded codes fp32, scale fp32 [N]): fp32 scale and quotient, e4m3 of the quotient."""
    amax = w.abs().amax(1)
    scale = torch.where(amax > 0, (amax / 448.0).clamp(min=SCALE_FLOOR), torch.ones_like(amax))
    return f8ref.q_e4m3((w / scale[:, None]).double(), rounding).float(), scale


def _stats(h, C, eps=LN_EPS):
    """(rstd, -mean rstd) of the LayerNorm fold, from the fp32 (sum, sumsq) of the stored rows."""
    s, ss = h.sum(-1, keepdim=True), (h * h).sum(-1, keepdim=True)
    mean = s / C
    rstd = torch.rsqrt((ss / C - mean * mean).clamp_min(0.0) + eps)
    return rstd, -mean * rstd


def _fold(h, w, gamma, beta, C, alpha=None, bias=None):
    """rstd (x (W gamma)^T - mean colsum) + W beta (+ bias) with (W gamma) fp16 (ops.pack_linear_ln); alpha [n] multiplies product and bias."""
    wg = _r16(w * gamma[None, :])
    c1 = wg.double().sum(1).float()
    c2 = w.double() @ beta.double()
    if bias is not None:
        c2 = c2 + bias.double()
    c2 = c2.float()
    if alpha is not None:
        c1, c2 = c1 * alpha, c2 * alpha
    rstd, nm = _stats(h, C)
    acc = h @ wg.t()
    return acc * (rstd if alpha is None else rstd * alpha) + (nm * c1 + c2)


def _spread(s, n, block=32):
    """Scales [..., blocks] -> one per element [..., n]."""
    return s.repeat_interleave(block, -1)[..., :n]


def attention_mx8_emulate(q, k, v, heads, alpha, block=32, vt_along_d=False, mismatch=None):
    """The MX-fp8 core on fp16-valued q, k, v [B, N, C] fp32: q alpha (fp32), k quantised along d, V^T along the tokens; fp32 scores; P =
    exp2(s - rowmax) rounded to e4m3 once, shared by the numerator and the denominator; o / l -> fp16-valued [B, N, C] fp32.
    block / vt_along_d: another block geometry, used CONSISTENTLY by producer and consumer (value-neutral short of the subnormal range: a
    power-of-two scale only moves the e4m3 exponent).  mismatch: the faults - the operands are quantised as above and the consumer reads the
    scales in another geometry: "pair64" one scale per 64 elements (the first 32-block's for both), "vt_axis" V^T's scales as if its
    blocks ran along d."""
    def deq(t, fault_pair):
        qq, s = mx_quant(t.double(), block)
        if fault_pair:
            s = s[..., torch.arange(s.shape[-1]) // 2 * 2]
        return (qq * _spread(s, t.shape[-1], block)).float()
    pair = mismatch == "pair64"
    qh = deq(_heads((q * _f32(alpha)), heads), pair)
    kh = deq(_heads(k, heads), pair)
    vh = _heads(v, heads)
    if vt_along_d:
        vh = deq(vh, pair)
    elif mismatch == "vt_axis":
        codes = mx_quant(vh.double().transpose(-1, -2).contiguous(), block)[0].transpose(-1, -2)       # [B, H, N, D], blocks along the tokens
        vh = (codes * _spread(mx_quant(vh.double(), block)[1], vh.shape[-1], block)).float()          # scales of blocks along d
    else:
        vh = deq(vh.transpose(-1, -2).contiguous(), pair).transpose(-1, -2)
    s = qh @ kh.transpose(-1, -2)
    pr = f8ref.q_e4m3(torch.exp2(s - s.max(-1, keepdim=True).values).double()).float()
    o = (pr @ vh) * (1.0 / pr.sum(-1, keepdim=True))
    B, H, N, D = o.shape
    return _r16(o.permute(0, 2, 1, 3).reshape(B, N, H * D))


def _emu_block(sd, p, h, context, heads, mode, path, fault, reblock=None):
    F = lambda n: sd[p + n].float()      # noqa: E731
    B, N, C = h.shape
    D = C // heads
    c = D ** -0.5 * LOG2E
    wq, wk, wv = F("attn1.to_q.weight"), F("attn1.to_k.weight"), F("attn1.to_v.weight")
    g1, b1, g3, b3 = F("norm1.weight"), F("norm1.bias"), F("norm3.weight"), F("norm3.bias")
    wp, bp = F("ff.net.0.proj.weight"), F("ff.net.0.proj.bias")
    rounding = "trunc" if fault == "weights truncated" else "rne"
    prescaled = False
    # ---- attn1's projections
    if path == "folded":
        inner = wq.shape[0]
        qa = 1.0 if fault == "q scale not applied" else c
        alpha = torch.cat([torch.full((inner,), qa), torch.ones(2 * inner)]).float()
        qkv = _r16(_fold(h, torch.cat([wq, wk, wv], 0), g1, b1, C, alpha=alpha))
        q, k, v = qkv.split(inner, -1)
        prescaled = True
    elif path == "plain":
        xn = _r16(_ln(h, g1, b1))
        q, k, v = (_r16(xn @ _r16(w).t()) for w in (wq, wk, wv))
    else:
        gg, bb = (g3, b3) if fault == "norm3's pack for norm1" else (g1, b1)
        x8, sx = ln8(h, gg, bb, per_tensor=fault == "one A scale for all rows")
        outs = []
        for i, w in enumerate((wq, wk, wv)):
            w8, sw = pack_f8(w, rounding)
            if i == 2 and fault == "w_scale of q|k on V^T":
                sw = pack_f8(wq, rounding)[1]
            outs.append(_r16((x8 @ w8.t()) * sx * sw[None, :]))
        q, k, v = outs
    # ---- the attention core
    if _att(mode):
        alpha = 1.0 if prescaled or fault == "q scale not applied" else c
        if fault == "q scale applied twice":
            alpha = alpha * c
        a = attention_mx8_emulate(q, k, v, heads, alpha, mismatch={"MX blocks of 64": "pair64", "V^T blocked along d": "vt_axis"}.get(fault),
                                  **(reblock or {}))
    else:
        dp, mpad, ones = ag.form_of(ag.instantiation(B, heads, N, N, D))
        a = ag.attn_emulate(_heads(q, heads).half(), _heads(k, heads).half(), _heads(v, heads).half(), c, mpad=mpad, q_prescaled=prescaled,
                            ones=ones).float()
    # ---- to_out + attn2's constant + residual
    cv = _r16(context.float()[:, 0] @ _r16(F("attn2.to_v.weight")).t())
    const = _r16(cv @ _r16(F("attn2.to_out.0.weight")).t() + F("attn2.to_out.0.bias"))
    x1 = _r16(a @ _r16(F("attn1.to_out.0.weight")).t() + F("attn1.to_out.0.bias") + const[:, None, :] + h)
    # ---- feed-forward
    if path == "folded":
        hh = _fold(x1, wp, g3, b3, C, bias=bp)
    elif path == "plain":
        hh = _r16(_ln(x1, g3, b3)) @ _r16(wp).t() + bp
    else:
        x8, sx = ln8(x1, g3, b3, per_tensor=fault == "one A scale for all rows")
        w8, sw = pack_f8(_r16(wp), rounding)                        # (GEGLU.run_f8 packs from its fp16 pack)
        if fault == "GEGLU scales swapped":                         # the kernel's rows are (value_0, gate_0, value_1, ...): row j takes scale j
            Fh = wp.shape[0] // 2                                   # of the UN-interleaved order
            j = torch.arange(2 * Fh)
            inter = torch.where(j < Fh, 2 * j, 2 * (j - Fh) + 1)    # position of original row j in the interleaved order
            sw = sw[inter]
        hh = (x8 @ w8.t()) * sx * sw[None, :] + bp
    val, gate = hh.chunk(2, -1)
    gl = _r16(val * _gelu(gate))
    return _r16(gl @ _r16(F("ff.net.2.weight")).t() + F("ff.net.2.bias") + x1)


def path_of(mode, N, fold_layernorm=True):
    """The LayerNorm mode BasicTransformerBlock._mode takes for the 320-wide fixture at N tokens."""
    if _lin(mode):
        return "f8"
    return "folded" if fold_layernorm and N % 8 == 0 else "plain"


def emulate(mode, path, sd, x, context, heads, p="", copy_out=False, fault=None, reblock=None):
    """The chain as the GPU runs it (module docstring) -> fp16 [B, Hh, Ww, C].  mode None or in MODES; path in PATHS ("f8" exactly when
    the mode quantises the linears); copy_out: accepted, the same arithmetic; fault: a key of FAULTS; reblock: dict(block=64) or
    dict(vt_along_d=True) - another MX geometry used consistently (attention_mx8_emulate)."""
    assert mode is None or mode in MODES, mode
    assert path in PATHS and (path == "f8") == _lin(mode), (mode, path)
    assert fault is None or (fault in FAULTS and mode in FAULTS[fault][0]), (fault, mode)
    F = lambda n: sd[p + n].float()      # noqa: E731
    B, Hh, Ww, C = x.shape
    x2 = x.float().reshape(B, Hh * Ww, C)
    h = _r16(_gn(x2, F("norm.weight"), F("norm.bias")))
    h = _r16(h @ _r16(F("proj_in.weight").reshape(-1, C)).t() + F("proj_in.bias"))
    for i in blocks_of(sd, p):
        h = _emu_block(sd, f"{p}transformer_blocks.{i}.", h, context, heads, mode, path, fault, reblock)
    y = _r16(h @ _r16(F("proj_out.weight").reshape(C, -1)).t() + F("proj_out.bias") + x2)
    return y.half().reshape(B, Hh, Ww, C)


# ---- the block cases of test_q8gate_cpu.py / test_q8gate_gpu.py ---------------------------------------------------------------------------
GRIDS = (8, 5, 16)        # N = 64: the fold, with attn_fp8 the MX copy-out; N = 25: N % 8 != 0, the plain chain, V^T padded, the quantiser
                          # path; N = 256: four key tiles and several row tiles - the deferred maximum and the tile seams inside the block
CASES = (                 # (name, switches for block_cases.set_switches, mode)
    ("default", {}, None),
    ("nofold", dict(fold_layernorm=False), None),
    ("linf8", dict(linear_fp8=True), "linear"),
    ("attnf8-proj", dict(attn_fp8=True, mx8_from_projection=True), "attention"),
    ("attnf8-quant", dict(attn_fp8=True, mx8_from_projection=False), "attention"),
    ("linf8-attnf8", dict(linear_fp8=True, attn_fp8=True), "both"),
)


def case_spec(grid):
    """The block_cases spec whose id seeds the inputs of a grid (one set of inputs per grid: the references are shared by its cases)."""
    return dict(id=f"q8gate-{grid}x{grid}", grid=grid, tokens=1, weights=None, regions=False, maps=False, switches={})


class Refs:
    """plain64, q64 per mode and the emulation per (mode, path) of one grid of the block_cases fixture, each computed once."""

    def __init__(self, sd, x, context, heads):
        self.sd, self.x, self.context, self.heads, self._c = sd, x, context, heads, {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def plain(self):
        return self._get("plain", lambda: plain(self.sd, self.x, self.context, self.heads))

    def q64(self, mode):
        return self.plain() if mode is None else self._get(("q", mode), lambda: quantised(mode, self.sd, self.x, self.context, self.heads))

    def emu(self, mode, path, fault=None):
        return self._get(("e", mode, path, fault), lambda: emulate(mode, path, self.sd, self.x, self.context, self.heads, fault=fault))

    def verdict(self, got, mode, path):
        return verdict(got, self.plain(), self.q64(mode), self.emu(mode, path), fp16_case=mode is None)


_REFS = {}


def refs(grid):
    """Refs of a grid on the seeded fixture of tests/block_cases.py (CPU), for st.run on cat([x, x]) - and st.run_paired on x - with the
    2B contexts."""
    if grid not in _REFS:
        import block_cases as bc
        st = bc.transformer("cpu")
        sd = {k: v.detach().float() for k, v in st.state_dict().items()}
        x, ctx, _, _ = bc.inputs(case_spec(grid), "cpu")
        _REFS[grid] = Refs(sd, torch.cat([x, x], 0), ctx, bc.HEADS)
    return _REFS[grid]


# ---- the gate -----------------------------------------------------------------------------------------------------------------------------
def verdict(got, plain64, q64, emu, fp16_case=False):
    """(accepted, text).  Accepts when got is finite, rel_l2(got, q64) <= REL_L2_FACTOR x rel_l2(emu, q64), for a quantising mode
    rel_l2(got, plain64) <= REL_L2_FACTOR x rel_l2(q64, plain64) (nearer to the plain block than 1.5 x the quantisation error itself), and
    for the fp16 cases (q64 is plain64) rel_l2(got, plain64) <= BLOCK_TOL."""
    if not bool(torch.isfinite(got.float()).all()):
        return False, "non-finite result"
    r_got, r_emu = rel_l2(got, q64), rel_l2(emu, q64)
    p_got = rel_l2(got, plain64)
    ok = r_got <= REL_L2_FACTOR * r_emu
    text = f"vs q64 {r_got:.3e} (emulation {r_emu:.3e}, limit x{REL_L2_FACTOR}); vs plain {p_got:.3e}"
    if fp16_case:
        ok = ok and p_got <= BLOCK_TOL
        text += f" (BLOCK_TOL {BLOCK_TOL:.0e})"
    else:
        p_q = rel_l2(q64, plain64)
        ok = ok and p_got <= REL_L2_FACTOR * p_q
        text += f" (q64 vs plain {p_q:.3e}, limit x{REL_L2_FACTOR})"
    return ok, text
