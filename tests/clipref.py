"""Gate of the exemplar-conditioning chain one level above the kernels: one CLIP encoder layer, the vision tower on pixels (patch
embedding, CLS and position rows, pre_layrnorm, the layers, post_layernorm of CLS), the one-token mapper with final_ln, and the whole
embedder followed by proj_out.  Helpers imported by test_clipgate_cpu.py and test_clipgate_gpu.py.  Not a conftest: plain functions only,
CPU tensors, no product code.

Everything works from a state dict with the names of ldm/modules/encoders/modules.py and xf.py (layer: one _EncoderLayer, no prefix;
tower: one _VisionTransformer, no prefix; mapper: `mapper.resblocks.N.*` and `final_ln.*`; cond: `cond_stage_model.*` and `proj_out.*`)
and the inputs as sent: x [B*N, d] fp16 (layer), CLIP-normalised fp32 pixels [B, 3, S, S] (tower, cond), z [B, width] fp16 (mapper).

plain(c, sd, inp)     the stage in fp64, nothing rounded.  Pinned on the CPU to oracle/pbe_oracle.py at fp32 accuracy.
ref64(c, sd, inp)     the same stage in exact fp64 with ONLY the roundings the packs perform: linear weights to fp16 (ops.pack_linear), the
                      patch weight to fp16 as [hidden, kp] with k = 3 P^2 zero-padded to kp, class_embedding and position_embedding to
                      fp16, norm gains and biases fp32.  packed_linear / packed_patch / packed_embedding / packed_norm hold the values;
                      test_clipgate_cpu.py pins each bit for bit against the modules' _pack().
emulate(c, sd, inp, reverse=, fault=)
                      the chain as the GPU runs it in plain fp32 torch (never a kernel's own output): fp32 accumulation and an fp16
                      rounding at every point where the path stores fp16 -
    tower embedding   the patches (pixels in (c, py, px) order) -> fp16; patch GEMM -> fp16 (the tile staged in LDS), + pos[1:] in fp32
                      -> fp16 again (the residual epilogue's double store, which tilecheck.py and actref.py model); fp16(cls + pos[0]);
                      pre_layrnorm -> fp16 (accgate.ln_emulate, as every LayerNorm here).
    encoder layer     layer_norm1 -> fp16; q | k = h Wqk^T + b -> fp16; V^T = Wv h^T + b (per row) -> fp16; attention
                      (accgate.attn_emulate in the form accgate.instantiation picks: "64,1" for D = 64, "32,1" for D = 32) -> fp16;
                      out_proj + bias -> fp16, + x -> fp16; layer_norm2 -> fp16; fc1 + bias, quick-GELU (actref.silu_f32 at 1.702) -> fp16;
                      fc2 + bias -> fp16, + x -> fp16.
    pooled            post_layernorm of the CLS rows -> fp16.
    mapper block      ln_1 -> fp16; V = h Wv^T + b (the last third of c_qkv) -> fp16; c_proj + bias -> fp16, + x -> fp16; ln_2 -> fp16;
                      c_fc + bias, erf-GELU (actref.gelu_erf_f32) -> fp16; c_proj + bias -> fp16, + x -> fp16.  Then final_ln -> fp16.
    proj_out          z W^T + b -> fp16.
                      reverse=True sums every K and the keys of every attention tile in the opposite order (another valid fp32 order);
                      an int sums every K and every key tile in a permutation seeded by it (a third order: the CPU test of the
                      verdict's peak margin).
verdict               convref.verdict with its constants unchanged (PEAK, REL_L2_FACTOR; neither is fitted to a run).  Token-stream
                      outputs [B*N, d] take the per-channel peak term E_c as there.  Outputs with one row per sample (pooled, mapper,
                      conditioning) have only B values per channel - too few for a per-channel maximum of the emulation's error to
                      bound a third order - so E is the largest |emulation - ref64| of the whole tensor in either order (the tensor is
                      judged as one channel).  The unit-scale term: rel_l2 against plain <= BLOCK_TOL (2e-3) for the single layer,
                      FWD_TOL (4e-3, tests/test_model_gpu.py) for the multi-layer chains; `flat` skips it.
CASES                 B = 3 throughout.  Recipes: unit; outlier (two channels of the residual stream - of the position rows for the tower -
                      carry fp16-exact means of +-32 over std 1, like CLIP's massive activations); peaked (q and k weights x 3: a few keys
                      hold the softmax); flat (layer and mapper: rows of 3e-3 randn, so eps decides rstd; the projections that write the
                      residual stream are scaled by FLAT_W so that the later norms meet a flat row too).  Pixels are seeded bytes through
                      (v / 255 - mean) / std with CLIP's constants.
FAULTS                wiring faults planted in the emulation only; test_clipgate_cpu.py demands that the verdict rejects each on every
                      case it applies to.  GAP_FAULTS are wrong at ONE site (one key of one query in one head, one bias element on one
                      row, one row's q bias): the verdict rejects them while its rel-L2 terms alone accept them.
"""
from __future__ import annotations

import math
import zlib

import torch
import torch.nn.functional as F

import accgate as ag
import actref
import convref
from convref import BLOCK_TOL, PEAK, REL_L2_FACTOR, rel_l2  # noqa: F401  (re-exported, unchanged)

FWD_TOL = 4e-3              # tests/test_model_gpu.py: one network forward (test_clipgate_cpu.py holds the two equal)
B = 3
EPS = 1e-5                  # layer_norm_eps of the tower; nn.LayerNorm's default in xf.py
FLAT, FLAT_W = 3e-3, 2.0 ** -7
OUTLIER = 32.0
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
KP = 592                    # 3 * 14^2 = 588 rounded up to a multiple of 8
PROJ = 96

KINDS = ("layer", "tower", "mapper", "cond")
_ENC, _EMB, _POOL, _MAP = ("layer", "tower", "cond"), ("tower", "cond"), ("tower", "cond"), ("mapper", "cond")

# name -> (kinds it applies to, recipes or None for every recipe, what is wired wrongly)
FAULTS = {
    "position rows shifted by one token": (_EMB, None, "patch token n takes the position row of token n - 1"),
    "CLS row without pos[0]": (_EMB, None, "the class row is the class embedding alone"),
    "position residual at a per-sample offset": (_EMB, None, "sample b reads the position rows b tokens on, as if they were not batch-shared"),
    "patch K order (py, px, c)": (_EMB, None, "the patches are gathered pixel-major against a channel-major weight"),
    "pre_layrnorm missing": (_EMB, None, "the layers read the raw embeddings"),
    "k from the q columns": (_ENC, None, "both score operands are the q half of q | k"),
    "softmax scale hidden^-1/2": (_ENC, None, "the scale of the hidden width instead of the head width"),
    "softmax scale (2d)^-1/2": (_ENC, None, "the scale of the q | k row width"),
    "heads split at the wrong width": (_ENC, None, "2 H heads of D / 2 channels"),
    "the last key missing from the numerator": (_ENC, None, "token N - 1 (the ragged tile) counts in the denominator only"),
    "V^T bias per column": (_ENC, None, "V^T's bias indexed by the token instead of the channel"),
    "attention residual from layer_norm1(x)": (_ENC, None, "out_proj adds the normalised input"),
    "MLP residual from the layer's input": (_ENC, None, "fc2 adds x instead of x + attention"),
    "erf-GELU in the tower": (_ENC, None, "fc1 runs the mapper's activation"),
    "quick-GELU in the mapper": (_MAP, None, "c_fc runs the tower's activation"),
    "layer_norm2's gain in layer_norm1": (_ENC, None, "layer_norm1 multiplies by layer_norm2.weight"),
    "pooled from token 1": (_POOL, None, "post_layernorm reads the first patch token instead of CLS"),
    "post_layernorm missing": (_POOL, None, "the pooled output is the raw CLS row"),
    "mapper V from rows w:2w of c_qkv": (_MAP, None, "the k third of c_qkv"),
    "mapper attention residual missing": (_MAP, None, "attn.c_proj without + x"),
    "final_ln eps 1e-6": (("mapper",), ("flat",), "final_ln runs with eps 1e-6"),
    "proj_out bias of the neighbouring column": (("cond",), None, "proj_out's bias shifted by one column"),
    "the row of sample b + 1": (_MAP, None, "the mapper (cond: proj_out) reads the row of the next sample"),
}

# Faults wrong at one site only: the LAST row of the token stream (token N - 1 of sample B - 1, the ragged row of every tile), and there one
# head (head 0) or one column (column 5).  name -> (ids of the cases it is planted on, what is wired wrongly).  On these cases the verdict
# rejects each while its rel-L2 terms alone accept it (test_clipgate_cpu.py asserts both); on other cases some of them move the output by
# less than two summation orders differ, where no gate can see them, or sit within a tenth of either limit, where the draw of a summation
# order would decide (the pairs kept are at most 1.34 of the emulation's rel-L2 against the limit of 1.5, and at least 2.3 x the peak limit).
_L = "layer-256h4-"
GAP_FAULTS = {
    "one key: the last key missing from one query's numerator in one head":
        ((_L + "N65-unit", _L + "N65-outlier", "layer-128h4-N65-outlier"), "head 0 of the last row sums P V without key N - 1"),
    "one key: the last key twice in one query's denominator in one head":
        ((_L + "N65-outlier", _L + "N65-flat", "layer-128h4-N65-outlier"), "head 0 of the last row divides by l + P[N - 1]"),
    "one bias: out_proj's bias of the neighbouring column on one row":
        ((_L + "N17-unit", _L + "N65-outlier"), "column 5 of the last row takes bias 6"),
    "one bias: fc2's bias of the neighbouring column on one row":
        ((_L + "N65-outlier", "layer-128h4-N65-peaked"), "column 5 of the last row takes bias 6"),
    "one bias: V^T bias per column for one key of one query":
        ((_L + "N65-flat",), "head 0 of the last row reads key N - 1's value row with the bias indexed by the token"),
    "one row: the last row's q without its bias":
        ((_L + "N17-outlier",), "q of the last row is h Wq^T alone"),
}


def fault_applies(name, c):
    if name in GAP_FAULTS:
        return c["id"] in GAP_FAULTS[name][0]
    kinds, recipes, _ = FAULTS[name]
    return c["kind"] in kinds and (recipes is None or c["recipe"] in recipes)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _case(kind, recipe, hidden=256, heads=4, N=0, image=0, layers=1):
    shape = {"layer": f"{hidden}h{heads}-N{N}", "tower": f"{hidden}h{heads}-img{image}x{layers}", "mapper": f"{hidden}x{layers}",
             "cond": f"{hidden}h{heads}-img{image}x{layers}to{PROJ}"}[kind]
    cid = f"{kind}-{shape}-{recipe}"
    if image:
        N = (image // 14) ** 2 + 1
    return dict(id=cid, kind=kind, recipe=recipe, hidden=hidden, heads=heads, mlp=4 * hidden, N=N, image=image, patch=14, layers=layers, B=B,
                qk=3.0 if recipe == "peaked" else 1.0, seed=zlib.crc32(cid.encode()) & 0x7FFFFFFF)


CASES = [_case("layer", r, N=n) for n in (17, 65) for r in ("unit", "outlier", "peaked", "flat")]
CASES += [_case("layer", r, hidden=128, N=65) for r in ("unit", "outlier", "peaked")]                 # D = 32, the narrow model's head
CASES += [_case("tower", r, image=56, layers=2) for r in ("unit", "outlier", "peaked")]
CASES += [_case("tower", r, image=112, layers=2) for r in ("unit", "outlier")]
CASES += [_case("mapper", r, layers=2) for r in ("unit", "outlier", "flat")]
CASES += [_case("cond", r, image=56, layers=2) for r in ("unit", "outlier")]
# (no `peaked` on the 112-pixel tower or on cond: with score std 9 in two chained layers the packs' fp16 weights alone move the pooled output
#  by 1.8e-3 and 1.0e-3 rel-L2 against plain, and the emulation's own orders then land at 3.4e-3 .. 4.05e-3 - on FWD_TOL itself, where the
#  unit-scale term would tell a correct run from a wrong one by the draw of a summation order.  The 56-pixel tower keeps it at 2.5e-3.)


def case_by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def unit_tol(c):
    """The unit-scale limit of a case against plain: None for `flat`."""
    if c["recipe"] == "flat":
        return None
    return BLOCK_TOL if c["kind"] == "layer" else FWD_TOL


def rowwise(c, name):
    """True for an output with one row per sample (E over the whole tensor), False for a token stream (E per channel)."""
    return not (c["kind"] == "layer" or name.startswith("stream"))


def oracle_cfgs(c):
    """(clip cfg, mapper cfg) for oracle/pbe_oracle.py."""
    return (dict(hidden=c["hidden"], heads=c["heads"], layers=c["layers"], mlp=c["mlp"], patch=c["patch"], image=c["image"], eps=EPS),
            dict(width=c["hidden"], layers=c["layers"]))


def _layer_shapes(out, p, d, mlp):
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        out[f"{p}self_attn.{n}.weight"], out[f"{p}self_attn.{n}.bias"] = (d, d), (d,)
    for n in ("layer_norm1", "layer_norm2"):
        out[f"{p}{n}.weight"], out[f"{p}{n}.bias"] = (d,), (d,)
    out[f"{p}mlp.fc1.weight"], out[f"{p}mlp.fc1.bias"] = (mlp, d), (mlp,)
    out[f"{p}mlp.fc2.weight"], out[f"{p}mlp.fc2.bias"] = (d, mlp), (d,)


def _tower_shapes(out, p, c):
    d = c["hidden"]
    out[p + "embeddings.class_embedding"] = (d,)
    out[p + "embeddings.patch_embedding.weight"] = (d, 3, c["patch"], c["patch"])
    out[p + "embeddings.position_embedding.weight"] = (c["N"], d)
    for n in ("pre_layrnorm", "post_layernorm"):
        out[f"{p}{n}.weight"], out[f"{p}{n}.bias"] = (d,), (d,)
    for i in range(c["layers"]):
        _layer_shapes(out, f"{p}encoder.layers.{i}.", d, c["mlp"])


def _mapper_shapes(out, p, w, layers):
    for i in range(layers):
        q = f"{p}mapper.resblocks.{i}."
        out[q + "attn.c_qkv.weight"], out[q + "attn.c_qkv.bias"] = (3 * w, w), (3 * w,)
        out[q + "attn.c_proj.weight"], out[q + "attn.c_proj.bias"] = (w, w), (w,)
        out[q + "mlp.c_fc.weight"], out[q + "mlp.c_fc.bias"] = (4 * w, w), (4 * w,)
        out[q + "mlp.c_proj.weight"], out[q + "mlp.c_proj.bias"] = (w, 4 * w), (w,)
        for n in ("ln_1", "ln_2"):
            out[f"{q}{n}.weight"], out[f"{q}{n}.bias"] = (w,), (w,)
    out[p + "final_ln.weight"], out[p + "final_ln.bias"] = (w,), (w,)


def shapes(c):
    """{parameter name: shape} of the case's state dict."""
    out = {}
    if c["kind"] == "layer":
        _layer_shapes(out, "", c["hidden"], c["mlp"])
    elif c["kind"] == "tower":
        _tower_shapes(out, "", c)
    elif c["kind"] == "mapper":
        _mapper_shapes(out, "", c["hidden"], c["layers"])
    else:
        _tower_shapes(out, "cond_stage_model.transformer.vision_model.", c)
        _mapper_shapes(out, "cond_stage_model.", c["hidden"], c["layers"])
        out["proj_out.weight"], out["proj_out.bias"] = (PROJ, c["hidden"]), (PROJ,)
    return out


def outlier_channels(c):
    """The two channels that carry +OUTLIER and -OUTLIER in the `outlier` recipe."""
    g = torch.Generator().manual_seed(c["seed"] ^ 0x0C0C0C)
    a, b = torch.randperm(c["hidden"], generator=g)[:2].tolist()
    return a, b


_FLAT_FEEDERS = ("self_attn.out_proj.", "mlp.fc2.", "attn.c_proj.", "mlp.c_proj.")


def state_dict(c):
    """The stage's fp32 parameters from a CPU generator seeded by the case: matrices and the patch kernel at 1 / sqrt(fan-in), norm gains
    1 + 0.1 randn, biases 0.1 randn, class and position embeddings randn."""
    g = torch.Generator().manual_seed(c["seed"])
    sd = {}
    for name, shape in shapes(c).items():
        r = torch.randn(shape, generator=g)
        if name.endswith("embedding") or name.endswith("position_embedding.weight"):
            sd[name] = r
        elif len(shape) > 1:
            sd[name] = r / math.sqrt(r[0].numel())
        elif name.endswith("weight"):
            sd[name] = 1.0 + 0.1 * r
        else:
            sd[name] = 0.1 * r
    for name in sd:
        if c["qk"] != 1.0 and (name.endswith("q_proj.weight") or name.endswith("k_proj.weight")):
            sd[name] = sd[name] * c["qk"]
        if c["recipe"] == "flat" and any(f in name for f in _FLAT_FEEDERS):
            sd[name] = sd[name] * FLAT_W
        if c["recipe"] == "outlier" and name.endswith("position_embedding.weight"):
            a, b = outlier_channels(c)
            sd[name][:, a] += OUTLIER
            sd[name][:, b] -= OUTLIER
    return sd


def pixels_from_bytes(v):
    """uint8 [B, 3, S, S] -> the fp32 pixels preprocessing sends: (v / 255 - mean) / std in fp32."""
    m, s = torch.tensor(CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    return (v.float() / 255.0 - m) / s


def inputs(c):
    """dict(x) for the layer ([B*N, d] fp16), dict(z) for the mapper ([B, width] fp16), dict(pixels) for tower and cond (fp32)."""
    g = torch.Generator().manual_seed(c["seed"] ^ 0x5A5A5A)
    if c["kind"] in ("tower", "cond"):
        S = c["image"]
        return dict(pixels=pixels_from_bytes(torch.randint(0, 256, (c["B"], 3, S, S), generator=g, dtype=torch.uint8)))
    rows = c["B"] * c["N"] if c["kind"] == "layer" else c["B"]
    x = torch.randn(rows, c["hidden"], generator=g)
    if c["recipe"] == "flat":
        x = FLAT * x
    elif c["recipe"] == "outlier":
        a, b = outlier_channels(c)
        x[:, a] += OUTLIER
        x[:, b] -= OUTLIER
    return {"x" if c["kind"] == "layer" else "z": x.half()}


# ---- the packs, restated --------------------------------------------------------------------------------------------------------------------
def packed_linear(w):
    """The values ops.pack_linear keeps: [N, K] fp16."""
    return w.detach().float().reshape(w.shape[0], -1).half().contiguous()


def packed_patch(w, kp=KP):
    """_VisionTransformer._pack's wpatch: the conv kernel [hidden, 3, P, P] as [hidden, kp] fp16 in (c, py, px) order, zeros from 3 P^2 on."""
    k = w[0].numel()
    out = torch.zeros(w.shape[0], kp, dtype=torch.float16)
    out[:, :k] = w.detach().float().reshape(w.shape[0], k).half()
    return out


def packed_embedding(e):
    """class_embedding / position_embedding.weight as packed: fp16."""
    return e.detach().float().half().contiguous()


def packed_norm(p):
    """A norm's gain or bias as packed: fp32, untouched."""
    return p.detach().float().contiguous()


# ---- the arithmetic of the chain in three precisions ----------------------------------------------------------------------------------------
class _Arith:
    """mode "plain" (fp64, nothing rounded), "ref64" (fp64, pack roundings only) or "emu" (fp32, every store rounded; reverse and fault
    as in the module docstring)."""

    def __init__(self, mode, reverse=False, fault=None):
        assert mode in ("plain", "ref64", "emu") and (fault is None or fault in FAULTS or fault in GAP_FAULTS)
        self.mode, self.reverse, self.fault = mode, reverse, fault if mode == "emu" else None
        self.dt = torch.float32 if mode == "emu" else torch.float64

    def t(self, x):
        return x.to(self.dt)

    def w(self, w):                                   # a packed fp16 operand's values (weights, embeddings)
        return self.t(w) if self.mode == "plain" else self.t(w.detach().float().half())

    def r(self, x):                                   # an fp16 store
        return x.half().float() if self.mode == "emu" else x

    def order(self, n):
        """The index order a sum over n terms runs in: None (ascending), reversed, or a seeded permutation."""
        if self.reverse is False:
            return None
        if self.reverse is True:
            return torch.arange(n - 1, -1, -1)
        return torch.randperm(n, generator=torch.Generator().manual_seed(int(self.reverse) * 7919 + n))

    def mm(self, a, w):
        """a [.., K] @ w [N, K]^T."""
        o = self.order(a.shape[-1])
        if o is not None:
            a, w = a[..., o], w[..., o]
        return a @ w.transpose(-1, -2)

    def ln(self, x, g, b, eps=EPS):
        """LayerNorm over the last dim -> stored fp16."""
        if self.mode == "emu":
            return ag.ln_emulate(x.half(), g, b, eps).float()
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g.double() + b.double()

    def act(self, v, act):
        if self.mode == "emu":
            return actref.act_f32(v, act)
        return actref.act64(v, act)

    def attention(self, q, k, v, Bn, N, H, D, scale):
        """softmax(q k^T scale) v over [Bn * N, H * D] operands -> [Bn * N, H * D] (stored fp16 in emu)."""
        if self.mode != "emu":
            q4, k4, v4 = (ag.heads(t, Bn, N, H, D) for t in (q, k, v))
            w = torch.softmax(q4 @ k4.transpose(-1, -2) * scale, -1)
            return (w @ v4).permute(0, 2, 1, 3).reshape(Bn * N, H * D)
        _, mpad, ones = ag.form_of(ag.instantiation(Bn, H, N, N, D))
        q4, k4, v4 = (ag.heads(t.half(), Bn, N, H, D) for t in (q, k, v))
        rev = self.reverse is True
        if self.reverse is not False and not rev:      # a seeded permutation of the keys inside every 64-key tile
            idx = torch.cat([t0 + self.order(min(ag.KT, N - t0)) for t0 in range(0, N, ag.KT)])
            k4, v4 = k4[:, :, idx], v4[:, :, idx]
        o = ag.attn_emulate(q4, k4, v4, scale * ag.LOG2E, mpad=mpad, q_prescaled=False, ones=ones, reverse=rev)
        return o.float().reshape(Bn * N, H * D)


def _p(A, sd, name):
    return A.t(sd[name])


def _last_row_only(clean, bad, cols=None):
    """clean with its LAST row (columns `cols`, default all) taken from bad: a fault at one site."""
    out = clean.clone()
    if cols is None:
        out[-1] = bad[-1]
    else:
        out[-1, cols] = bad[-1, cols]
    return out


def _layer(A, sd, p, x, Bn, N, H):
    """_EncoderLayer.run on the residual stream x [Bn * N, d]."""
    f = A.fault
    d = x.shape[1]
    D = d // H
    W = lambda n: A.w(sd[p + n + ".weight"])          # noqa: E731
    bias = lambda n: _p(A, sd, p + n + ".bias")       # noqa: E731
    h = A.ln(x, sd[p + ("layer_norm2" if f == "layer_norm2's gain in layer_norm1" else "layer_norm1") + ".weight"], sd[p + "layer_norm1.bias"])
    q = A.r(A.mm(h, W("self_attn.q_proj")) + bias("self_attn.q_proj"))
    if f == "one row: the last row's q without its bias":
        q = _last_row_only(q, A.r(A.mm(h, W("self_attn.q_proj"))))
    k = q if f == "k from the q columns" else A.r(A.mm(h, W("self_attn.k_proj")) + bias("self_attn.k_proj"))
    bv = bias("self_attn.v_proj")
    acc_v = A.mm(h, W("self_attn.v_proj")).reshape(Bn, N, d)                  # V^T [d, N] per sample, held here as [N, d]
    v = A.r(acc_v + bv[None, None, :]).reshape(Bn * N, d)
    v_tok = A.r(acc_v + bv[torch.arange(N) % d][None, :, None]).reshape(Bn * N, d)      # the bias indexed by the token
    if f == "V^T bias per column":
        v = v_tok
    scale = {"softmax scale hidden^-1/2": d ** -0.5, "softmax scale (2d)^-1/2": (2 * d) ** -0.5}.get(f, D ** -0.5)
    Hh, Dh = (2 * H, D // 2) if f == "heads split at the wrong width" else (H, D)
    o = A.attention(q, k, v, Bn, N, Hh, Dh, scale)
    if f is not None and ("the last key" in f or "for one key of one query" in f):
        last = torch.arange(Bn * N) % N == N - 1
        if "numerator" in f:                                                  # the key's value row is absent from P V, its P stays in the sum
            bad = A.attention(q, k, torch.where(last[:, None], torch.zeros_like(v), v), Bn, N, H, D, scale)
        elif "denominator" in f:                                              # l + P_last: o l / (l + P_last), P_last / l recovered from two runs
            wl = _last_key_weight(A, q, k, Bn, N, H, D, scale)
            bad = A.r(o / (1.0 + wl))
        else:                                                                 # the last key's value row with the token-indexed bias
            bad = A.attention(q, k, torch.where(last[:, None], v_tok, v), Bn, N, H, D, scale)
        o = bad if f == "the last key missing from the numerator" else _last_row_only(o, bad, slice(0, D))
    bo = bias("self_attn.out_proj")
    y = A.r(A.mm(o, W("self_attn.out_proj")) + bo)                           # the tile as staged in fp16 ...
    if f == "one bias: out_proj's bias of the neighbouring column on one row":
        y = _last_row_only(y, A.r(A.mm(o, W("self_attn.out_proj")) + bo.roll(-1)), [5])
    x1 = A.r(y + (h if f == "attention residual from layer_norm1(x)" else x))        # ... and stored again after the residual add
    h2 = A.ln(x1, sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"])
    c1 = bias("mlp.fc1")
    a = A.r(A.act(A.mm(h2, W("mlp.fc1")) + c1, 2 if f == "erf-GELU in the tower" else 3))
    c2 = bias("mlp.fc2")
    y2 = A.r(A.mm(a, W("mlp.fc2")) + c2)
    if f == "one bias: fc2's bias of the neighbouring column on one row":
        y2 = _last_row_only(y2, A.r(A.mm(a, W("mlp.fc2")) + c2.roll(-1)), [5])
    return A.r(y2 + (x if f == "MLP residual from the layer's input" else x1))


def _last_key_weight(A, q, k, Bn, N, H, D, scale):
    """The softmax weight of the last key per (row, head), broadcast to [Bn * N, H * D] (fp32: only the planted fault uses it)."""
    q4, k4 = (ag.heads(t, Bn, N, H, D) for t in (q, k))
    w = torch.softmax(q4 @ k4.transpose(-1, -2) * scale, -1)[..., -1:]                  # [Bn, H, N, 1]
    return w.expand(Bn, H, N, D).permute(0, 2, 1, 3).reshape(Bn * N, H * D)


def _tower(A, c, sd, p, pixels, outs):
    """_VisionTransformer.pooled; the residual stream after each layer goes to outs["stream<i>"]."""
    f = A.fault
    Bn, d, P, N, H = pixels.shape[0], c["hidden"], c["patch"], c["N"], c["heads"]
    k = 3 * P * P
    patches = F.unfold(A.t(pixels), P, stride=P).transpose(1, 2)             # [B, G G, (c, py, px)]
    if f == "patch K order (py, px, c)":
        patches = patches.reshape(Bn, N - 1, 3, P * P).transpose(2, 3).reshape(Bn, N - 1, k)
    patches = A.r(patches)
    wp = A.w(sd[p + "embeddings.patch_embedding.weight"]).reshape(d, k)
    pos, cls = A.w(sd[p + "embeddings.position_embedding.weight"]), A.w(sd[p + "embeddings.class_embedding"])
    res = pos[1:]
    if f == "position rows shifted by one token":
        res = pos[:-1]
    res = res[None].expand(Bn, -1, -1)
    if f == "position residual at a per-sample offset":
        res = torch.stack([pos[1:].roll(-b, 0) for b in range(Bn)])
    tok = A.r(A.r(A.mm(patches, wp)) + res)                                  # the tile staged in fp16, + pos[1:] in fp32, stored again
    row0 = A.r(cls if f == "CLS row without pos[0]" else cls + pos[0])
    x = torch.cat([row0[None, None].expand(Bn, 1, d), tok], 1).reshape(Bn * N, d)
    if f != "pre_layrnorm missing":
        x = A.ln(x, sd[p + "pre_layrnorm.weight"], sd[p + "pre_layrnorm.bias"])
    for i in range(c["layers"]):
        x = _layer(A, sd, f"{p}encoder.layers.{i}.", x, Bn, N, H)
        outs[f"stream{i}"] = x
    row = x.reshape(Bn, N, d)[:, 1 if f == "pooled from token 1" else 0]
    if f == "post_layernorm missing":
        return row
    return A.ln(row, sd[p + "post_layernorm.weight"], sd[p + "post_layernorm.bias"])


def _mapper(A, c, sd, p, z):
    """Transformer.run on z [B, w], then final_ln."""
    f = A.fault
    w = c["hidden"]
    for i in range(c["layers"]):
        q = f"{p}mapper.resblocks.{i}."
        h = A.ln(z, sd[q + "ln_1.weight"], sd[q + "ln_1.bias"])
        rows = slice(w, 2 * w) if f == "mapper V from rows w:2w of c_qkv" else slice(2 * w, 3 * w)
        v = A.r(A.mm(h, A.w(sd[q + "attn.c_qkv.weight"][rows])) + _p(A, sd, q + "attn.c_qkv.bias")[rows])
        y = A.r(A.mm(v, A.w(sd[q + "attn.c_proj.weight"])) + _p(A, sd, q + "attn.c_proj.bias"))
        z1 = y if f == "mapper attention residual missing" else A.r(y + z)
        h2 = A.ln(z1, sd[q + "ln_2.weight"], sd[q + "ln_2.bias"])
        a = A.r(A.act(A.mm(h2, A.w(sd[q + "mlp.c_fc.weight"])) + _p(A, sd, q + "mlp.c_fc.bias"), 3 if f == "quick-GELU in the mapper" else 2))
        z = A.r(A.r(A.mm(a, A.w(sd[q + "mlp.c_proj.weight"])) + _p(A, sd, q + "mlp.c_proj.bias")) + z1)
    return A.ln(z, sd[p + "final_ln.weight"], sd[p + "final_ln.bias"], 1e-6 if f == "final_ln eps 1e-6" else EPS)


def _run(A, c, sd, inp):
    """{output name: tensor}; "out" is the stage's output, "stream<i>" the tower's residual stream after layer i."""
    kind, f = c["kind"], A.fault
    outs = {}
    if kind == "layer":
        outs["out"] = _layer(A, sd, "", A.t(inp["x"]), c["B"], c["N"], c["heads"])
    elif kind == "tower":
        outs["out"] = _tower(A, c, sd, "", inp["pixels"], outs)
    elif kind == "mapper":
        z = A.t(inp["z"])
        outs["out"] = _mapper(A, c, sd, "", z.roll(-1, 0) if f == "the row of sample b + 1" else z)
    else:
        assert kind == "cond", kind
        z = _tower(A, c, sd, "cond_stage_model.transformer.vision_model.", inp["pixels"], outs)
        outs["pooled"] = z
        z = _mapper(A, c, sd, "cond_stage_model.", z)
        if f == "the row of sample b + 1":
            z = z.roll(-1, 0)
        b = _p(A, sd, "proj_out.bias")
        y = A.r(A.mm(z, A.w(sd["proj_out.weight"])) + (b.roll(1) if f == "proj_out bias of the neighbouring column" else b))
        outs["out"] = y[:, None, :]
        outs = {k: v for k, v in outs.items() if not k.startswith("stream")}          # the tower cases gate the streams
    return outs


def plain(c, sd, inp, outputs=False):
    """fp64, nothing rounded: the stage's output, or with outputs=True the dict of every gated output."""
    o = _run(_Arith("plain"), c, sd, inp)
    return o if outputs else o["out"]


def ref64(c, sd, inp, outputs=False):
    """fp64, only the packs' roundings."""
    o = _run(_Arith("ref64"), c, sd, inp)
    return o if outputs else o["out"]


def emulate(c, sd, inp, reverse=False, fault=None, outputs=False):
    """The chain as the GPU runs it -> fp16 (module docstring)."""
    assert fault is None or fault_applies(fault, c), (fault, c["id"])
    o = {k: v.half() for k, v in _run(_Arith("emu", reverse, fault), c, sd, inp).items()}
    return o if outputs else o["out"]


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------
def _one_channel(t):
    return t.reshape(-1, 1)


def verdict(got, plain64, ref, emu_fwd, emu_rev, tol, whole_tensor_peak):
    """(accepted, text): convref.verdict's rel-L2 and peak terms (whole_tensor_peak: E over the whole tensor, for outputs with one row
    per sample), and for tol not None rel_l2(got, plain64) <= tol."""
    ts = (got, plain64, ref, emu_fwd, emu_rev)
    assert len({tuple(t.shape) for t in ts}) == 1, [tuple(t.shape) for t in ts]
    if whole_tensor_peak:
        ts = tuple(_one_channel(t) for t in ts)
    ok, text = convref.verdict(*ts, False)
    text += f"; emulated orders vs ref64 {rel_l2(emu_fwd, ref):.3e} / {rel_l2(emu_rev, ref):.3e}"
    if tol is not None and bool(torch.isfinite(got.float()).all()):
        p = rel_l2(got, plain64)
        text += f" (unit-scale limit {tol:.0e})" + ("" if p <= tol else "  REJECTED: unit-scale")
        ok = ok and p <= tol
    return ok, text


def rel_l2_terms_accept(got, plain64, ref, emu_fwd, emu_rev, tol):
    """The verdict without its peak term (what a whole-tensor gate alone would say)."""
    return convref.rel_l2_terms_accept(got, plain64, ref, emu_fwd, emu_rev, False) and (tol is None or rel_l2(got, plain64) <= tol)


class Refs:
    """State dict, inputs, plain64, ref64 and the emulations of one case (dicts of every gated output), each computed once and never
    changed."""

    def __init__(self, c):
        self.c, self.sd, self.inp = c, state_dict(c), inputs(c)
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def plain(self):
        return self._get("plain", lambda: plain(self.c, self.sd, self.inp, outputs=True))

    def ref64(self):
        return self._get("ref64", lambda: ref64(self.c, self.sd, self.inp, outputs=True))

    def emu(self, reverse=False, fault=None):
        return self._get(("e", reverse, fault), lambda: emulate(self.c, self.sd, self.inp, reverse=reverse, fault=fault, outputs=True))

    def names(self):
        return list(self.ref64())

    def verdict_of(self, name, got):
        return verdict(got, self.plain()[name], self.ref64()[name], self.emu(False)[name], self.emu(True)[name], unit_tol(self.c), rowwise(self.c, name))

    def verdict(self, got):
        """got: {output name: tensor} -> (every output accepted, one line per output)."""
        res = [(n,) + self.verdict_of(n, got[n]) for n in self.names()]
        return all(r[1] for r in res), "\n".join(f"[{n}] {t}" for n, _, t in res)

    def rel_l2_terms_accept(self, got):
        return all(rel_l2_terms_accept(got[n], self.plain()[n], self.ref64()[n], self.emu(False)[n], self.emu(True)[n], unit_tol(self.c))
                   for n in self.names())


_REFS = {}


def refs(cid):
    if cid not in _REFS:
        _REFS[cid] = Refs(case_by_id(cid))
    return _REFS[cid]
