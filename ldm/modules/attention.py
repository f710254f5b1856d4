"""Transformer pieces of the U-Net, same class names / constructor arguments / parameter names as
ldm/modules/attention.py in zhanwenchen/pbe (GEGLU :38-45, FeedForward :48-65, CrossAttention
:189-230, BasicTransformerBlock :233-252, SpatialTransformer :255-298), executed by HIP kernels:

  * activations stay ``[B, N, C]`` fp16 (tokens x channels == NHWC, so the reference's two
    rearranges per block are free),
  * to_q | to_k run as ONE GEMM, to_v as a second GEMM with swapped operands that emits V^T
    (what the fused attention kernel consumes), softmax(QK^T)V never touches HBM,
  * a BasicTransformerBlock is ONE chain of three stages, whatever the context and the precision (BasicTransformerBlock._block):
    attn1 ``x1 = x + to_out(attn1(norm1 x))``, attn2 ``x2 = x1 + attn2(norm2 x1, ctx)``, ff ``x2 + ff(norm3 x2)``.  Each stage is
    written once and evaluates its LayerNorm in one of three modes (_mode): folded into the GEMM that reads it, a separate launch, or
    emitted as fp8.  A guidance pair shares everything upstream of the first launch that depends on the context and parts there,
  * the Paint-by-Example context is ONE token per sample, so attn2's softmax over a single key is exactly 1 and
    ``attn2(x, ctx) = to_out(to_v(ctx))`` for every query (attention.py:207-230): it is computed once per context as a
    [B, C] vector and rides in the epilogue of attn1's output projection - the attn2 stage launches nothing.  norm2 / attn2.to_q /
    attn2.to_k keep their parameters (checkpoint compatibility) but are dead arithmetic with such a context,
  * a context of SEVERAL tokens (several exemplars) keeps that structure: everything that depends on the context alone is folded once
    per context into two skinny operands, and the attn2 stage is ONE launch over the residual stream (pbe_ctx_attention_f16, DESIGN.md
    section 4.11); contexts longer than that kernel takes run q / attention / to_out,
  * exemplar tokens may carry a weight per sample (``context_weights``) and a map of where each applies (``context_regions``: regional
    exemplars, a weight per query row - pbe_ctx_attention_rw_f16 on the same folded operands),
  * the softmax weights of that launch can be collected as attribution maps (``ContextMaps``: which exemplar each position attended
    to - pbe_ctx_attention_map_f16, the same launch with a side output),
  * bias, residual and the row-broadcast adds are GEMM epilogues.
"""
from contextlib import nullcontext
from types import SimpleNamespace

import torch
from torch import nn

from pbe_amd import ops
from pbe_amd.hipmodule import HipModule, f32, require_gpu
from pbe_amd.lib import PbeError

LOG2E = 1.4426950408889634      # the attention kernels run exp2: scale log2(e) goes onto q


def exists(val):
    return val is not None


def default(val, d):
    return val if val is not None else (d() if callable(d) else d)


def zero_module(module):
    for p in module.parameters():
        p.detach().zero_()
    return module


def Normalize(in_channels):
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)


def _tokens(x):
    """[B, N, C] any float dtype -> contiguous fp16 on the GPU."""
    require_gpu(x, "attention")
    return x.to(torch.float16).contiguous()


class GEGLU(HipModule):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)

    def _pack(self):
        wi, bi = ops.pack_geglu(self.proj.weight.detach(), self.proj.bias.detach())
        return SimpleNamespace(w=wi, b=bi, f8=None)          # (value, gate) rows interleaved: gating fused in the GEMM epilogue

    def run(self, x2d):
        p = self.pk()
        return ops.gemm(x2d, p.w, p.b, act=ops.ACT_GEGLU)

    def run_f8(self, x8, sx):
        """x8 / sx: the fp8 LayerNorm output and its row scales -> same result shape as run(); weights e4m3 with a scale per (interleaved) row."""
        p = self.pk()
        if p.f8 is None:
            p.f8 = ops.pack_linear_f8(p.w.float())
        return ops.gemm_f8(x8, sx, p.f8[0], p.f8[1], p.b, act=ops.ACT_GEGLU)

    def forward(self, x):
        x = _tokens(x)
        return self.run(x.view(-1, x.shape[-1])).view(*x.shape[:-1], -1)


class FeedForward(HipModule):
    def __init__(self, dim, dim_out=None, mult=4, glu=False, dropout=0.):
        super().__init__()
        inner = int(dim * mult)
        dim_out = default(dim_out, dim)
        if not glu:
            raise PbeError("FeedForward(glu=False) is not on the Paint-by-Example path (BasicTransformerBlock uses gated_ff=True)")
        self.net = nn.Sequential(GEGLU(dim, inner), nn.Dropout(dropout), nn.Linear(inner, dim_out))

    def _pack(self):
        return SimpleNamespace(w2=ops.pack_linear(self.net[2].weight), b2=f32(self.net[2].bias))

    def run(self, x2d, resid=None):
        """x2d [M, C] fp16 -> Linear(GEGLU(x)) (+ resid)."""
        p = self.pk()
        return ops.gemm(self.net[0].run(x2d), p.w2, p.b2, resid=resid)

    def run_f8(self, x8, sx, resid=None):
        """fp8 operands for the GEGLU projection (its input comes from the fp8 LayerNorm); the output projection stays fp16: its input
        is the GEGLU product, whose per-row scale would need a pass over all 4C columns of a row."""
        p = self.pk()
        return ops.gemm(self.net[0].run_f8(x8, sx), p.w2, p.b2, resid=resid)

    def forward(self, x):
        x = _tokens(x)
        return self.run(x.view(-1, x.shape[-1])).view(x.shape[0], x.shape[1], -1)


class CrossAttention(HipModule):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        inner = dim_head * heads
        self.is_self = context_dim is None
        context_dim = default(context_dim, query_dim)
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.dim_head = dim_head
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))

    def _pack(self):
        ns = SimpleNamespace(wv=ops.pack_linear(self.to_v.weight), wo=ops.pack_linear(self.to_out[0].weight), bo=f32(self.to_out[0].bias))
        if self.to_q.weight.shape[1] == self.to_k.weight.shape[1]:
            ns.wqk = ops.pack_linear(torch.cat([self.to_q.weight, self.to_k.weight], 0))
        ns.wq, ns.wk = ops.pack_linear(self.to_q.weight), ops.pack_linear(self.to_k.weight)
        ns.f8 = None
        return ns

    def self_attention_f8(self, x8, sx, B, N):
        """self_attention with fp8 (e4m3) operands for the q|k and V^T projections: x8 [B*N, C] uint8 + row scales sx [B*N] from
        pbe_layernorm_f8, weights e4m3 with one scale per output channel.  The attention core itself stays fp16 (fp32 softmax)."""
        p = self.pk()
        if p.f8 is None:
            p.f8 = (ops.pack_linear_f8(torch.cat([self.to_q.weight, self.to_k.weight], 0)), ops.pack_linear_f8(self.to_v.weight))
        (wqk8, sqk), (wv8, sv) = p.f8
        inner = self.heads * self.dim_head
        if self._mx8_out(N):                     # both projections write the MX-fp8 operands directly (no fp16 q | k / V^T)
            q8, k8, v8 = ops.qkv_mx8_f8(x8, sx, wqk8, sqk, wv8, sv, B=B, H=self.heads, N=N, D=self.dim_head, q_alpha=self.scale * LOG2E)
            return ops.attention_mx8(q8, k8, v8, 1.0).view(B * N, inner)
        qk = ops.gemm_f8(x8, sx, wqk8, sqk)
        npad = (N + 7) // 8 * 8
        vt = torch.empty((B, inner, npad), dtype=torch.float16, device=x8.device)
        ops.gemm_f8(wv8.unsqueeze(0).expand(B, -1, -1), sv, x8.view(B, N, -1), sx.view(B, N), out=vt[:, :, :N] if npad != N else vt)
        return self.attention_core(qk, vt, B, N, npad)

    attn_fp8 = False            # pbe_amd.precision.set_attention_precision(model, "fp8"): the self-attention core runs on MX-fp8 operands
    mx8_from_projection = True  # with attn_fp8: the folded / fp8 q|k|v^T projections write the MX-fp8 operands (pbe_gemm_mx8out_f16);
                                # False: fp16 projection + pbe_quant_mx8_f16 (A/B runs, tests) - the same bytes

    def _mx8_out(self, N):
        """The projection emits the MX-fp8 operands: attention fp8 on, the switch on, and a shape the MX copy-out takes (whole samples
        of 64 tokens, head dims of pbe_attention_mx8); other shapes keep the quantiser path."""
        return self.attn_fp8 and self.mx8_from_projection and N % 64 == 0 and self.dim_head in (40, 80, 160)

    def attention_core(self, qk, vt, B, N, vt_rs, q_prescaled=False):
        """softmax(q k^T scale) v of every self-attention path: qk [B*N, 2*inner] holds q | k, vt [B, inner, vt_rs] holds V^T;
        returns [B*N, inner].  fp16 core (pbe_attention_f16), or with attn_fp8 the MX-fp8 core: q, k and V^T are quantised to e4m3
        with a power-of-two scale per 32 elements (scale log2(e) goes onto q there unless the projection already applied it)."""
        inner, H, D = self.heads * self.dim_head, self.heads, self.dim_head
        if self.attn_fp8:
            c = self.scale * LOG2E
            q8 = ops.quant_mx8(qk, B, H, N, D, rs=2 * inner, alpha=1.0 if q_prescaled else c)
            k8 = ops.quant_mx8(qk[:, inner:], B, H, N, D, rs=2 * inner)
            v8 = ops.quant_mx8(vt, B, H, N, D, rs=vt_rs, vt=True)
            return ops.attention_mx8(q8, k8, v8, 1.0).view(B * N, inner)
        o = ops.attention(qk, qk[:, inner:], vt, B, H, N, N, D, self.scale, q_strides=(N * 2 * inner, 2 * inner),
                          k_strides=(N * 2 * inner, 2 * inner), vt_strides=(inner * vt_rs, vt_rs), q_prescaled=q_prescaled)
        return o.view(B * N, inner)

    # ---- fast paths used by BasicTransformerBlock -------------------------------------------
    def self_attention(self, xn, B, N):
        """xn [B*N, C] (already normed) -> per-head softmax(QK^T)V as [B*N, inner] (before to_out)."""
        p = self.pk()
        inner = self.heads * self.dim_head
        qk = ops.gemm(xn, p.wqk)                                              # [M, 2*inner]
        npad = (N + 7) // 8 * 8
        vt = torch.empty((B, inner, npad), dtype=torch.float16, device=xn.device)
        ops.gemm(p.wv.unsqueeze(0).expand(B, -1, -1), xn.view(B, N, -1), out=vt[:, :, :N] if npad != N else vt)
        return self.attention_core(qk, vt, B, N, npad)

    def self_attention_fused(self, x2d, stats, bp, B, N):
        """LayerNorm + to_q | to_k | to_v + attention core with ONE projection launch: x2d [B*N, C] is the RAW residual stream, `stats` its
        row statistics (from the producer's epilogue), bp the block's pack (weights pre-multiplied by norm1's gain, attention.py:248).
        The GEMM folds the LayerNorm into its epilogue, multiplies the q columns by scale log2(e) in fp32 (the attention kernel then
        runs exp2 on the MFMA output directly) and stores the v columns transposed (V^T, what the attention kernel streams)."""
        inner = self.heads * self.dim_head
        if self._mx8_out(N):                     # MX-fp8 copy-out: q | k | V^T leave the epilogue as the attention core's operands
            q8, k8, v8 = ops.qkv_mx8(x2d, bp.wqkv, bp.c2qkv, ln=(stats, bp.c1qkv, bp.eps1), B=B, H=self.heads, N=N, D=self.dim_head,
                                     alpha=bp.qscale, alpha_cols=inner)
            return ops.attention_mx8(q8, k8, v8, 1.0).view(B * N, inner)
        qk = torch.empty((B * N, 2 * inner), dtype=torch.float16, device=x2d.device)
        vt = torch.empty((B, inner, N), dtype=torch.float16, device=x2d.device)
        ops.gemm(x2d, bp.wqkv, bp.c2qkv, ln=(stats, bp.c1qkv, bp.eps1), alpha=bp.qscale, alpha_cols=inner, out=qk, vt=vt, vt_col0=2 * inner, vt_tokens=N)
        return self.attention_core(qk, vt, B, N, N, q_prescaled=True)

    def single_token_context(self, context):
        """context [B, 1, Dc] -> to_out(to_v(context)) as [B, C] fp16 (softmax over one key == 1)."""
        p = self.pk()
        c = _tokens(context)
        if c.shape[1] != 1:
            raise PbeError(f"CrossAttention: Paint-by-Example conditions on ONE exemplar token, got {c.shape[1]}")
        v = ops.gemm(c.view(c.shape[0], -1), p.wv)
        return ops.gemm(v, p.wo, p.bo)

    # ---- reference-shaped entry point ------------------------------------------------------------
    def forward(self, x, context=None, mask=None):
        if exists(mask):
            raise PbeError("CrossAttention: masks are not used on the Paint-by-Example path")
        x = _tokens(x)
        B, N, _ = x.shape
        p = self.pk()
        if context is None:
            o = self.self_attention(x.view(B * N, -1), B, N)
            return ops.gemm(o, p.wo, p.bo).view(B, N, -1)
        c = _tokens(context)
        if c.shape[1] == 1:
            return self.single_token_context(c)[:, None, :].expand(B, N, -1).contiguous()
        # general context length (not on the hot path): separate q / k / v projections
        inner, Nk = self.heads * self.dim_head, c.shape[1]
        q = ops.gemm(x.view(B * N, -1), p.wq)
        k = ops.gemm(c.view(B * Nk, -1), p.wk)
        npad = (Nk + 7) // 8 * 8
        vt = torch.zeros((B, inner, npad), dtype=torch.float16, device=x.device)
        ops.gemm(p.wv.unsqueeze(0).expand(B, -1, -1), c, out=vt[:, :, :Nk] if npad != Nk else vt)
        o = ops.attention(q, k, vt, B, self.heads, N, Nk, self.dim_head, self.scale, q_strides=(N * inner, inner),
                          k_strides=(Nk * inner, inner), vt_strides=(inner * npad, npad))
        return ops.gemm(o.view(B * N, inner), p.wo, p.bo).view(B, N, -1)


class ContextKV:
    """What the existing-kernel route of a multi-token attn2 keeps per context: k = to_k(context) [B*Nk, inner] and
    vt = to_v(context)^T [B, inner, npad] (npad = Nk rounded up to 8, zeros past Nk); log2w [B, Nk] fp32 = log2 of the exemplar
    weights (the key bias of pbe_attention_kbias_f16) or None."""
    __slots__ = ("k", "vt", "B", "Nk", "log2w")

    def __init__(self, k, vt, B, Nk, log2w=None):
        self.k, self.vt, self.B, self.Nk, self.log2w = k, vt, B, Nk, log2w

    def rows(self, b0, b1):
        return ContextKV(self.k[b0 * self.Nk:b1 * self.Nk], self.vt[b0:b1], b1 - b0, self.Nk, None if self.log2w is None else self.log2w[b0:b1])


class ContextWeights:
    """Validated exemplar weights of one context, as the kernels take them: log2w fp32 [B, K] on the context's device, log2 of the
    weight of token j of sample b, -inf for weight 0.  Built ONCE per context by prepare_context_weights() (set-up, like the schedule tables)."""
    __slots__ = ("log2w", "w")

    def __init__(self, log2w, w=None):
        self.log2w, self.w = log2w, w           # w: the validated fp64 host copy (prepare_context_regions multiplies the maps by it)


def prepare_context_weights(context, weights):
    """Exemplar weights [B, K] (tensor or nested sequence, any device) for context [B, K, Dc] -> ContextWeights, or None for None.
    Token j of sample b takes the softmax weight w[b, j] exp(s_j) / sum_i w[b, i] exp(s_i) (attention.py:207-230 with the token counted
    w times): weight 0 removes it (a padded ragged batch), integer weights equal repeating it, uniform weights change nothing.  Raises
    PbeError unless the weights are [B, K], finite, >= 0 and every sample's sum is > 0.  log2 is taken in fp64 on the host."""
    if weights is None or isinstance(weights, ContextWeights):
        return weights
    if context.dim() != 3:
        raise PbeError(f"context weights: context must be [B, K, Dc], got {tuple(context.shape)}")
    B, K = context.shape[0], context.shape[1]
    w = torch.as_tensor(weights).detach().to("cpu", torch.float64)
    if tuple(w.shape) != (B, K):
        raise PbeError(f"context weights: weights must be [{B}, {K}] (one per context token), got {tuple(w.shape)}")
    if not bool(torch.isfinite(w).all()):
        raise PbeError("context weights: weights must be finite")
    if bool((w < 0).any()):
        raise PbeError("context weights: weights must be >= 0")
    if not bool((w.sum(1) > 0).all()):
        raise PbeError("context weights: every sample needs a positive weight sum (at least one exemplar token present)")
    return ContextWeights(torch.log2(w).to(torch.float32).to(context.device).contiguous(), w)


class ContextRegions:
    """Validated regional exemplar maps of one context: maps fp64 [B, K, Hr, Wr] and weights fp64 [B, K] on the host.  level(h, w) is
    the table pbe_ctx_attention_rw_f16 takes at a transformer level with an h x w grid: fp32 [B, h*w, K] on the context's device,
    log2 of the effective weight e[b, t, j] = w[b, j] * (area average of maps[b, j] over grid cell t = y*w + x, the NHWC row order);
    a row that no token of positive weight covers takes e[b, t, :] = w[b, :] (outside every region the exemplars blend as they do
    without regions), so every row keeps a token of positive weight.  Built once per (context, level), uploaded once, cached here."""
    __slots__ = ("maps", "weights", "device", "_levels")

    def __init__(self, maps, weights, device):
        self.maps, self.weights, self.device, self._levels = maps, weights, device, {}

    def level_weights(self, h, w):
        """fp64 host [B, h*w, K]: the effective weights e of the h x w level (fallback rows included)."""
        B, K, Hr, Wr = self.maps.shape
        h, w = int(h), int(w)
        if h < 1 or w < 1 or Hr % h or Wr % w:
            raise PbeError(f"context regions: the {Hr} x {Wr} region maps do not divide into the {h} x {w} grid of this transformer level "
                           f"(both sides must be whole multiples)")
        r = self.maps.view(B, K, h, Hr // h, w, Wr // w).mean((3, 5))                 # area average, fp64
        e = (r.reshape(B, K, h * w) * self.weights[:, :, None]).permute(0, 2, 1)
        bare = e.sum(-1, keepdim=True) <= 0
        return torch.where(bare, self.weights[:, None, :].expand_as(e), e).contiguous()

    def level(self, h, w):
        t = self._levels.get((int(h), int(w)))
        if t is None:
            t = torch.log2(self.level_weights(h, w)).to(torch.float32).to(self.device).contiguous()
            self._levels[(int(h), int(w))] = t
        return t


def prepare_context_regions(context, regions, weights=None):
    """Region maps [B, K, Hr, Wr] (>= 0; 1 = token j counts fully at that position, 0 = absent there; any resolution that every
    transformer level's grid divides) for context [B, K, Dc] -> ContextRegions, or None for None.  weights: the exemplar weights
    [B, K] (or a ContextWeights) that multiply the maps, None = ones; they are checked by prepare_context_weights.  Raises PbeError
    unless the maps are [B, K, Hr, Wr], finite and >= 0."""
    if regions is None or isinstance(regions, ContextRegions):
        return regions
    if context.dim() != 3:
        raise PbeError(f"context regions: context must be [B, K, Dc], got {tuple(context.shape)}")
    B, K = context.shape[0], context.shape[1]
    r = torch.as_tensor(regions).detach().to("cpu", torch.float64)
    if r.dim() != 4 or tuple(r.shape[:2]) != (B, K) or r.shape[2] < 1 or r.shape[3] < 1:
        raise PbeError(f"context regions: regions must be [{B}, {K}, Hr, Wr] (one map per context token), got {tuple(r.shape)}")
    if not bool(torch.isfinite(r).all()):
        raise PbeError("context regions: regions must be finite")
    if bool((r < 0).any()):
        raise PbeError("context regions: regions must be >= 0")
    cw = prepare_context_weights(context, weights)
    if cw is None:
        w = torch.ones((B, K), dtype=torch.float64)
    else:
        w = cw.w if cw.w is not None else torch.exp2(cw.log2w.detach().to("cpu", torch.float64))
    return ContextRegions(r.contiguous(), w, context.device)


def prepare_row_weights(x_shape, context, row_weights):
    """Already-levelled effective weights e [B, N, K] (>= 0, finite, a positive sum on every row) -> the kernel's table fp32
    [B, N, K] = log2 e on the context's device (log2 in fp64 on the host)."""
    B, N, K = x_shape[0], x_shape[1], context.shape[1]
    e = torch.as_tensor(row_weights).detach().to("cpu", torch.float64)
    if tuple(e.shape) != (B, N, K):
        raise PbeError(f"context row weights: must be [{B}, {N}, {K}] (sample, query token, context token), got {tuple(e.shape)}")
    if not bool(torch.isfinite(e).all()) or bool((e < 0).any()):
        raise PbeError("context row weights: must be finite and >= 0")
    if not bool((e.sum(-1) > 0).all()):
        raise PbeError("context row weights: every row needs a positive weight sum")
    return torch.log2(e).to(torch.float32).to(context.device).contiguous()


class ContextMaps:
    """Collector of exemplar ATTRIBUTION MAPS: per sample and context token, the share of cross-attention that token received at each
    position - the softmax weights of attention.py:207-230, averaged over the heads (in the kernel: pbe_ctx_attention_map_f16), the
    transformer blocks of a level, the U-Net calls of a run and the levels.  One zero-initialised fp32 accumulator [B, h*w, K] per level
    grid, into which every multi-token cross-attention launch of that level adds its head-mean weights, and a launch count per level.

    level(h, w) allocates the accumulator at the first (eager) call, so a graph capture finds it in place; launches captured into a graph
    are counted when the graph is replayed (begin_tape / end_tape / replayed - pbe_amd.graph.GraphedUNet).  The collector covers the
    LAST B samples of the batch it is handed with: all of it, or the conditional half of a guidance batch cat([uc, c]).  A one-token
    context launches nothing: its maps are identically 1 (the softmax over one key).

    With a collector a K > 1 context always takes the fused kernel (as regional exemplars do), so WITHOUT regions the levels wider than
    BasicTransformerBlock.ctx_fused_max_width change route: the result then equals, bit for bit, the collector-less run with
    ctx_fused_max_width = 1280, and the default collector-less run within the samplers' tolerance.  With regions the route is the
    same with and without a collector, and so are the bits."""

    def __init__(self):
        self.B = self.K = self.device = None
        self._levels, self._counts, self._tape = {}, {}, None

    def bind(self, B, K, device):
        """Fix the collector's shape (the first user does; a second user must agree)."""
        B, K, device = int(B), int(K), torch.device(device)
        if self.B is None:
            self.B, self.K, self.device = B, K, device
        elif (self.B, self.K, self.device) != (B, K, device):
            raise PbeError(f"ContextMaps: collecting for {self.B} samples x {self.K} tokens on {self.device}, handed {B} x {K} on {device}")
        return self

    def level(self, h, w):
        """The accumulator fp32 [B, h*w, K] of the h x w level (zeros at first use)."""
        if self.B is None:
            raise PbeError("ContextMaps: not bound to a batch yet (bind(B, K, device))")
        k = (int(h), int(w))
        t = self._levels.get(k)
        if t is None and self.K > 1:
            t = self._levels[k] = torch.zeros((self.B, k[0] * k[1], self.K), dtype=torch.float32, device=self.device)
            self._counts.setdefault(k, 0)
        return t

    def note(self, h, w, launches):
        """`launches` launches were issued (or, inside begin_tape / end_tape, captured) that add to level (h, w)."""
        k = (int(h), int(w))
        tgt = self._counts if self._tape is None else self._tape
        tgt[k] = tgt.get(k, 0) + int(launches)
        self._counts.setdefault(k, 0)

    def begin_tape(self):
        self._tape = {}

    def end_tape(self):
        t, self._tape = self._tape, None
        return t

    def replayed(self, tape):
        for k, n in tape.items():
            self._counts[k] = self._counts.get(k, 0) + n

    def counts(self):
        """{(h, w): launches that have added to the level}."""
        return dict(self._counts)

    def grids(self):
        return sorted(self._counts, reverse=True)

    def per_level(self):
        """{(h, w): fp32 [B, K, h, w]}: each level's accumulator divided by its launch count, unmerged (K = 1: ones)."""
        out = {}
        for k in self.grids():
            if self.K == 1:
                out[k] = torch.ones((self.B, 1, *k), dtype=torch.float32, device=self.device)
            elif self._counts[k] > 0:
                out[k] = ops.ctx_map_gather(self._levels[k], k, div=float(self._counts[k]))
        return out

    def result(self, grid):
        """fp32 [B, K, Hl, Wl] on grid = (Hl, Wl) (the latent grid: every level's grid must divide it): each level's accumulator divided
        by its launch count, gathered to the grid (nearest; pbe_ctx_map_gather_f32) and the levels averaged with equal weight.  K = 1: ones."""
        if self.B is None:
            raise PbeError("ContextMaps.result: nothing was collected")
        Hl, Wl = int(grid[0]), int(grid[1])
        if self.K == 1:
            return torch.ones((self.B, 1, Hl, Wl), dtype=torch.float32, device=self.device)
        live = [k for k in self.grids() if self._counts[k] > 0]
        if not live:
            raise PbeError("ContextMaps.result: nothing was collected")
        for h, w in live:
            if Hl % h or Wl % w:
                raise PbeError(f"ContextMaps.result: the {Hl} x {Wl} grid is not a whole multiple of the {h} x {w} level")
        out = torch.empty((self.B, self.K, Hl, Wl), dtype=torch.float32, device=self.device)
        for i, k in enumerate(live):
            ops.ctx_map_gather(self._levels[k], k, 1.0 / len(live), out=out, accumulate=i > 0, div=float(self._counts[k]))
        return out


class Conditioning:
    """The cross-attention conditioning of one U-Net call or sampler run, carried as one value: context [B, K, Dc], weights (exemplar
    weights [B, K]), regions (region maps [B, K, Hr, Wr]) and maps (a ContextMaps collector); any of the last three may be None.  The
    public entry points build it from their context_weights= / context_regions= / context_maps= keywords; below them it is handed
    on whole.  It validates nothing: prepare_context_weights / prepare_context_regions do, where the operands are built."""
    __slots__ = ("context", "weights", "regions", "maps")

    def __init__(self, context, weights=None, regions=None, maps=None):
        self.context, self.weights, self.regions, self.maps = context, weights, regions, maps

    def key(self):
        """The identity both per-conditioning caches compare (UNetModel.context_vectors, pbe_amd.graph.GraphedUNet): per tensor its
        pointer, version, shape, dtype and device, per non-tensor its repr, for the collector its id.  It is the union of the two
        keys those caches used to build for themselves and changes exactly when either of them did - a tensor of another dtype or
        device is another storage, so its pointer differs too - hence neither cache hits or misses differently, with one exception
        that computes the same values: the U-Net's cache, which knew only WHETHER a collector is present, now also rebuilds when
        the same tensors come with another collector.  A cache that stores the key keeps the tensors alive beside it, so that a
        pointer cannot be recycled."""
        def one(v):
            if isinstance(v, torch.Tensor):
                return (v.data_ptr(), v._version, tuple(v.shape), v.dtype, str(v.device))
            return None if v is None else ("values", repr(v))
        return (one(self.context), one(self.weights), one(self.regions), None if self.maps is None else ("maps", id(self.maps)))

    def kwargs(self):
        """The keywords of forward_nhwc / forward for what is present: a plain context passes none."""
        kw = {"context_weights": self.weights, "context_regions": self.regions, "context_maps": self.maps}
        return {k: v for k, v in kw.items() if v is not None}


class RegionalVectors:
    """What SpatialTransformer.context_vectors returns for a context WITH regions: the per-block list and the context's
    ContextRegions.  The level is known only where the grid is: run / run_paired resolve it there (SpatialTransformer._levelled)."""
    __slots__ = ("vecs", "regions")

    def __init__(self, vecs, regions):
        self.vecs, self.regions = vecs, regions


class BasicTransformerBlock(HipModule):
    def __init__(self, dim, n_heads, d_head, dropout=0., context_dim=None, gated_ff=True, checkpoint=True):
        super().__init__()
        self.attn1 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)
        self.checkpoint = checkpoint

    def _pack(self):
        """Both LayerNorms are FOLDED into the GEMMs that read them (pbe_gemm_desc.ln_stats): norm1 into ONE q | k | v projection, norm3 into
        the GEGLU projection - the weights carry the gain, the bias carries W beta, the row statistics come from the producer's epilogue."""
        a, n1, n3 = self.attn1, self.norm1, self.norm3
        ns = SimpleNamespace(g1=f32(n1.weight), b1=f32(n1.bias), g3=f32(n3.weight), b3=f32(n3.bias), eps1=n1.eps, eps3=n3.eps, wqkv=None)
        inner = a.heads * a.dim_head
        if a.to_q.weight.shape[1] == a.to_k.weight.shape[1] == a.to_v.weight.shape[1]:
            ns.qscale = a.scale * LOG2E                           # q leaves the projection as scale log2(e) q (fp32 epilogue)
            ns.wqkv, ns.c2qkv, ns.c1qkv = ops.pack_linear_ln(torch.cat([a.to_q.weight, a.to_k.weight, a.to_v.weight], 0), None, n1.weight, n1.bias)
            ns.c2qkv[:inner] *= ns.qscale                         # (alpha multiplies the product, the bias is added after it)
        proj = self.ff.net[0].proj                       # (value, gate) rows interleaved, in fp32: pack_linear_ln folds the gain before it rounds
        ns.wg, ns.c2g, ns.c1g = ops.pack_linear_ln(*ops.interleave_geglu(proj.weight.detach().float(), proj.bias.detach().float()), n3.weight, n3.bias)
        ns.m2 = None                                     # the multi-token attn2 pack, built on first use (_pack_multi)
        return ns

    def _pack_multi(self):
        """The pack of attn2 with a multi-token context (kept on pk(), built on first use: the one-token path never pays for it)."""
        ns = self.pk()
        if ns.m2 is not None:
            return ns.m2
        m = SimpleNamespace()
        with torch.no_grad():
            # attn2 with a multi-token context (context_operands): norm2 folded into to_q - for the existing-kernel route as a LayerNorm-
            # folded q projection, for pbe_ctx_attention_f16 as per-head [C + 8, D] blocks whose rows are (Wq gamma2)[hD + d, c] for c < C
            # and (Wq beta2)[hD + d] at c = C, so ONE batched GEMM with to_k(context) gives Kq and the Kq . beta term; Wo per head likewise
            a2, n2 = self.attn2, self.norm2
            H, D, Cq = a2.heads, a2.dim_head, a2.to_q.weight.shape[1]
            m.g2, m.b2, m.eps2 = f32(n2.weight), f32(n2.bias), n2.eps
            m.qscale2 = a2.scale * LOG2E
            m.wq2, m.c2q2, m.c1q2 = ops.pack_linear_ln(a2.to_q.weight, None, n2.weight, n2.bias)
            wq32 = a2.to_q.weight.detach().float()
            ext = torch.zeros((H, Cq + 8, D), dtype=torch.float32, device=wq32.device)
            ext[:, :Cq] = (wq32 * n2.weight.detach().float()[None, :]).view(H, D, Cq).permute(0, 2, 1)
            ext[:, Cq] = (wq32.double() @ n2.bias.detach().double()).float().view(H, D)
            m.wq2h = ext.to(torch.float16).contiguous()
            m.wo2h = a2.to_out[0].weight.detach().float().view(-1, H, D).permute(1, 0, 2).to(torch.float16).contiguous()      # [H, C, D]
        ns.m2 = m
        return m

    linear_fp8 = False          # pbe_amd.precision.set_linear_precision(model, "fp8") turns the LayerNorm-fed projections to e4m3 operands
    fold_layernorm = True       # False: the separate LayerNorm launches of rounds 1-2 (A/B runs, tools/)

    def _folded(self, p, N):
        """The LayerNorm-folded chain, which starts with the fused q | k | V^T projection: only where the library can run that projection
        (N % 8 == 0 and an inner width whose V^T columns start on a column tile, ops.qkv_fusable); other blocks take the unfused launches."""
        return self.fold_layernorm and not self.linear_fp8 and p.wqkv is not None and N % 8 == 0 and \
            ops.qkv_fusable(self.attn1.heads * self.attn1.dim_head, N)

    # The dispatch bound of pbe_ctx_attention_f16, from profiles/ctx_attention_timing.txt: at C = 320 and 640 the fused kernel takes 0.41 ..
    # 0.95 of the faster composition for 2 .. 16 tokens; at C = 1280 (M = 2048 / 512 rows at the headline batch: 32 / 8 workgroups, each
    # walking 20 k-tiles and 20 column tiles behind exposed load latency) it takes 1.10 .. 1.70, so those levels run the existing kernels.
    # ctx_fused_max_width is a SPEED bound, measured against a composition (q projection / pbe_attention_kbias_f16 / to_out) that has no
    # per-row form: it does not apply to regional exemplars, which take the fused kernel at every width it accepts (_ctx_regional).
    ctx_fused_max_tokens = ops.CTX_MAX_TOKENS
    ctx_fused_max_width = 640

    def _ctx_fused(self, K):
        """A K-token context runs in the fused kernel: within the measured dispatch bound and the kernel's shape limits."""
        a2, Cq = self.attn2, self.attn2.to_q.weight.shape[1]
        return K <= min(self.ctx_fused_max_tokens, ops.CTX_MAX_TOKENS) and a2.heads * K <= ops.CTX_MAX_HJ and Cq % 64 == 0 and \
            64 <= Cq <= min(self.ctx_fused_max_width, ops.CTX_MAX_C)

    def _ctx_regional(self, K, what="regional exemplars"):
        """Regions (and attribution maps: `what`) need the fused kernel - the only per-row form, and the only one whose softmax weights
        can be brought out: raise PbeError naming the limit a K-token context breaks."""
        a2, Cq = self.attn2, self.attn2.to_q.weight.shape[1]
        if K > ops.CTX_MAX_TOKENS:
            raise PbeError(f"BasicTransformerBlock: {what} take at most {ops.CTX_MAX_TOKENS} context tokens, got {K}")
        if a2.heads * K > ops.CTX_MAX_HJ:
            raise PbeError(f"BasicTransformerBlock: {what} need heads * tokens <= {ops.CTX_MAX_HJ}, got {a2.heads} * {K}")
        if Cq % 64 or not 64 <= Cq <= ops.CTX_MAX_C:
            raise PbeError(f"BasicTransformerBlock: {what} need a width that is a multiple of 64 in 64..{ops.CTX_MAX_C}, got {Cq}")

    def _refuse_multi_f8(self):
        if self.linear_fp8:
            raise PbeError("BasicTransformerBlock: a multi-token context is not available with linear_fp8 (the fp8 path folds attn2's "
                           "constant into the out-projection epilogue; the multi-token kernels take fp16 operands only)")

    def context_operands(self, context, weights=None, regional=False, maps=False):
        """What run() needs of a context, computed once per context.  weights: exemplar weights [B, K] or a ContextWeights
        (prepare_context_weights: validated there), None = every token counts once; their log2 rides beside the operands (CtxOperands.log2w /
        ContextKV.log2w), which do not depend on it.  [B, 1, Dc]: attn2's constant to_out(to_v(context)) as [B, C]
        (single_token_context: the softmax over one key is 1).  [B, K > 1, Dc]: the operands of pbe_ctx_attention_f16 (ops.CtxOperands:
        with k = to_k(context), v = to_v(context), per head Kq = scale log2(e) k_h (Wq gamma2)_h, kbias = scale log2(e) k_h (Wq beta2)_h,
        Vo = Wo_h v_h, colsum = row sums of the fp16 Kq) - or, beyond that kernel's dispatch bound (K > 16, heads * K > 128, C > 640), a ContextKV
        for the q projection / pbe_attention_f16 / to_out route.  All products are pbe_gemm_f16 launches.  regional: the caller will hand
        the operands a per-row table (CtxOperands.with_row_weights), so K > 1 always takes the fused kernel, at every width it accepts,
        and a context beyond its limits is refused.  maps: the caller will hand the operands an attribution-map target
        (CtxOperands.with_map; ContextMaps) - the same route as regional, for the same reason: only the fused kernel has the form."""
        c = _tokens(context)
        if c.dim() != 3:
            raise PbeError(f"BasicTransformerBlock: context must be [B, K, Dc], got {tuple(c.shape)}")
        B, K, _ = c.shape
        cw = prepare_context_weights(c, weights)
        if K == 1:                                # (any positive weight on a single token is exact: the softmax over one key is 1)
            return self.attn2.single_token_context(c)
        self._refuse_multi_f8()
        a2, p2 = self.attn2, self.attn2.pk()
        inner = a2.heads * a2.dim_head
        if regional:
            self._ctx_regional(K)
        elif maps:
            self._ctx_regional(K, "attribution maps")
        k = ops.gemm(c.view(B * K, -1), p2.wk)                                    # [B*K, inner]
        if not (regional or maps) and not self._ctx_fused(K):
            npad = (K + 7) // 8 * 8
            vt = torch.zeros((B, inner, npad), dtype=torch.float16, device=c.device)
            ops.gemm(p2.wv.unsqueeze(0).expand(B, -1, -1), c, out=vt[:, :, :K] if npad != K else vt)
            return ContextKV(k, vt, B, K, None if cw is None else cw.log2w)
        o = self._fused_operands(c, k)
        o.log2w = None if cw is None else cw.log2w
        return o

    def _fused_operands(self, c, k=None):
        """ops.CtxOperands of context c [B, K, Dc] fp16 (K >= 1 within the kernel's limits; k = to_k(c) when the caller has it)."""
        a2, p2, bp = self.attn2, self.attn2.pk(), self._pack_multi()
        H, D = a2.heads, a2.dim_head
        B, K, _ = c.shape
        Cq = a2.to_q.weight.shape[1]
        c2d = c.view(B * K, -1)
        if k is None:
            k = ops.gemm(c2d, p2.wk)
        v = ops.gemm(c2d, p2.wv)
        heads = lambda t: t.view(B * K, H, D).permute(1, 0, 2)                    # [H, B*K, D] view: batch = head
        kq_h = ops.gemm(heads(k), bp.wq2h, alpha=bp.qscale2)                      # [H, B*K, C + 8]: Kq | Kq . beta
        vo_h = ops.gemm(heads(v), bp.wo2h)                                        # [H, B*K, C]
        HJ = H * K
        kq = kq_h[:, :, :Cq].reshape(H, B, K, Cq).permute(1, 0, 2, 3).reshape(B, HJ, Cq).contiguous()
        kbias = kq_h[:, :, Cq].reshape(H, B, K).permute(1, 0, 2).reshape(B, HJ).float().contiguous()
        colsum = ops.row_stats(kq.view(B * HJ, Cq)).buf[0, :, 0].reshape(B, HJ).contiguous()
        vo = torch.zeros((B, Cq, (HJ + 7) // 8 * 8), dtype=torch.float16, device=c.device)
        vo[:, :, :HJ] = vo_h.view(H, B, K, Cq).permute(1, 3, 0, 2).reshape(B, Cq, HJ)
        return ops.CtxOperands(kq, colsum, kbias, vo, p2.bo, H, K)

    def _attn2(self, x1, st2, ctx, B, N, folded, out=None, stats_out=None):
        """x2 = x1 + attn2(norm2(x1), ctx) for a multi-token context -> (x2, RowStats of x2 or None when not folded).  st2: RowStats of
        x1 (None: computed here).  out / stats_out: targets inside shared buffers (a guidance pair)."""
        p, a2, p2 = self._pack_multi(), self.attn2, self.attn2.pk()
        want = False if not folded else (stats_out if stats_out is not None else True)
        if isinstance(ctx, ops.CtxOperands):
            st = st2 if st2 is not None else ops.row_stats(x1)
            ranges = ctx.map_ranges()
            if len(ranges) == 1:
                return ops.ctx_attention(x1, ctx, st, p.eps2, tokens=N, out=out, row_stats=want)
            # an attribution map for SOME of the samples (the conditional half of a guidance batch): one launch per range.  Row tiles never
            # straddle samples and a workgroup sees its own sample only, so Y and the statistics are those of the one launch, bit for bit.
            M = x1.shape[0]
            y = out if out is not None else torch.empty_like(x1)
            rs = None
            if want is not False:
                rs = want if isinstance(want, ops.RowStats) else ops.RowStats(torch.empty((1, M, 2), dtype=torch.float32, device=x1.device), 1, M)
            for b0, b1 in ranges:
                r0, r1 = b0 * N, b1 * N
                ops.ctx_attention(x1[r0:r1], ctx.rows(b0, b1), ops.RowStats(st.buf, st.parts, st.ld, st.row0 + r0), p.eps2, tokens=N, out=y[r0:r1],
                                  row_stats=False if rs is None else ops.RowStats(rs.buf, 1, rs.ld, rs.row0 + r0))
            return y, (None if rs is None else ops.RowStats(rs.buf, 1, rs.ld, rs.row0))
        inner = a2.heads * a2.dim_head
        if folded:
            q = ops.gemm(x1, p.wq2, p.c2q2, ln=(st2 if st2 is not None else ops.row_stats(x1), p.c1q2, p.eps2))
        else:
            q = ops.gemm(ops.layernorm(x1, p.g2, p.b2, p.eps2), p2.wq)
        npad = ctx.vt.shape[2]
        o = ops.attention(q, ctx.k, ctx.vt, B, a2.heads, N, ctx.Nk, a2.dim_head, a2.scale, q_strides=(N * inner, inner),
                          k_strides=(ctx.Nk * inner, inner), vt_strides=(inner * npad, npad), key_bias=ctx.log2w)
        r = ops.gemm(o.view(B * N, inner), p2.wo, p2.bo, resid=x1, out=out, row_stats=want)
        return r if folded else (r, None)

    def _mode(self, N):
        """How the block's LayerNorms are evaluated at N tokens: "f8" (linear_fp8: emitted as e4m3 + a scale per token, BASELINE
        configs[4]), "folded" (into the GEMMs that read them, _folded) or "plain" (separate launches)."""
        return "f8" if self.linear_fp8 else "folded" if self._folded(self.pk(), N) else "plain"

    def _attn1_core(self, x2d, B, N, stats, mode):
        """attn1(norm1(x)) before to_out, [B*N, inner].  It does not depend on the context: a guidance pair runs it once."""
        p = self.pk()
        if mode == "folded":
            return self.attn1.self_attention_fused(x2d, stats if stats is not None else ops.row_stats(x2d), p, B, N)
        if mode == "f8":
            return self.attn1.self_attention_f8(*ops.layernorm_f8(x2d, p.g1, p.b1, p.eps1), B, N)
        return self.attn1.self_attention(ops.layernorm(x2d, p.g1, p.b1, p.eps1), B, N)

    def _attn1_out(self, a, x2d, N, mode, rowvec=None, out=None, stats_out=None):
        """x1 = x + to_out(a) (+ rowvec [B, C] on the rows of each sample: attn2's constant of a one-token context) -> (x1, RowStats of
        x1 or None when not folded).  out / stats_out: targets inside shared buffers (a guidance pair)."""
        a1 = self.attn1.pk()
        want = False if mode != "folded" else (stats_out if stats_out is not None else True)
        r = ops.gemm(a, a1.wo, a1.bo, rowvec=rowvec, group_rows=0 if rowvec is None else N, resid=x2d, out=out, row_stats=want)
        return r if mode == "folded" else (r, None)

    def _ff(self, x, st, mode, tail=None, paired=False):
        """x + ff(norm3(x)); st: RowStats of x (folded).  tail (folded only; SpatialTransformer._tail): the transformer's proj_out composed
        into this projection - resid + [h | x] w^T + b in ONE launch over the two-source K loop; a guidance pair (x holds both halves, the
        residual serves both) launches once per half under the pair's pinned plan, as the separate proj_out does."""
        p = self.pk()
        if mode == "folded":
            h = ops.gemm(x, p.wg, p.c2g, act=ops.ACT_GEGLU, ln=(st, p.c1g, p.eps3))
            if tail is not None:
                if not paired:
                    return ops.gemm(h, tail.w, tail.b, a2=x, resid=tail.resid)
                M = x.shape[0] // 2
                y = torch.empty((2 * M, tail.w.shape[0]), dtype=torch.float16, device=x.device)
                with ops.pinned_batch_scale(2):
                    for half in (0, 1):
                        ops.gemm(h[half * M:(half + 1) * M], tail.w, tail.b, a2=x[half * M:(half + 1) * M], resid=tail.resid, out=y[half * M:(half + 1) * M])
                return y
            fp = self.ff.pk()
            return ops.gemm(h, fp.w2, fp.b2, resid=x)
        if mode == "f8":
            return self.ff.run_f8(*ops.layernorm_f8(x, p.g3, p.b3, p.eps3), resid=x)
        return self.ff.run(ops.layernorm(x, p.g3, p.b3, p.eps3), resid=x)

    def _block(self, x2d, B, N, ctx, stats, paired, tail=None):
        """The stage chain of run (ctx for B samples) and run_paired (x2d serves both halves, ctx holds 2B samples).  What does not depend
        on the context runs once; the halves of a pair part at the first launch that does - attn1's out-projection for a one-token
        constant, attn2 for multi-token operands - each writing its half of one 2B buffer and of its row statistics."""
        mode, one, fused = self._mode(N), isinstance(ctx, torch.Tensor), isinstance(ctx, ops.CtxOperands)
        if not one:
            self._refuse_multi_f8()
        folded = mode == "folded"
        M, Cc = x2d.shape
        halves = [(ctx, None, None)]
        if paired:
            planes = 1 if fused else (Cc + 63) // 64             # (the fused cross-attention kernel writes one partial)
            x = torch.empty((2 * M, Cc), dtype=torch.float16, device=x2d.device)
            buf = torch.empty((planes, 2 * M, 2), dtype=torch.float32, device=x2d.device) if folded else None
            halves = [(ctx[h * B:(h + 1) * B] if one else ctx.rows(h * B, (h + 1) * B), x[h * M:(h + 1) * M],
                       ops.RowStats(buf, planes, 2 * M, h * M) if folded else None) for h in (0, 1)]
        # a pair's batch-B launches take the tile, split-K factor and statistics partials of the batch-2B layer: same bits.  A single run
        # enters no scale of its own: that would undo its caller's
        with ops.pinned_batch_scale(2) if paired else nullcontext():
            a = self._attn1_core(x2d, B, N, stats, mode)
            if one:
                for c, out, tgt in halves:
                    y, st = self._attn1_out(a, x2d, N, mode, c, out, tgt)
            else:
                x1, st1 = self._attn1_out(a, x2d, N, mode)
                if st1 is None and fused:
                    st1 = ops.row_stats(x1)
                for c, out, tgt in halves:
                    y, st = self._attn2(x1, st1, c, B, N, folded, out, tgt)
        if paired:                                               # the joined buffer, with the partial count the last launch reported
            y, st = x, ops.RowStats(buf, st.parts, 2 * M) if folded else None
        return self._ff(y, st, mode, tail, paired)

    def run(self, x2d, B, N, ctx_vec, stats=None, tail=None):
        """x2d [B*N, C] fp16 residual stream -> the block's output, same shape.  ctx_vec = context_operands(context) for the B samples:
        [B, C] = attn2's constant for a one-token context, or the multi-token operands (ops.CtxOperands / ContextKV); stats =
        ops.RowStats of x2d's rows when its producer emitted them (SpatialTransformer's proj_in does), else the folded chain computes
        them.  tail: _ff.  Stages and modes: _block."""
        return self._block(x2d, B, N, ctx_vec, stats, False, tail)

    def run_paired(self, x2d, B, N, ctx_vec, stats=None, tail=None):
        """Guidance pair with a SHARED input: x2d [B*N, C] serves both halves, ctx_vec holds the 2B contexts -> [2B*N, C], the bits of
        run on the duplicated input.  Everything upstream of the first launch that depends on the context runs once at batch B (_block)."""
        return self._block(x2d, B, N, ctx_vec, stats, True, tail)

    def forward(self, x, context=None, context_weights=None, context_row_weights=None, attn_map=None):
        """x [B, N, C], context [B, K, Dc] with K >= 1 tokens per sample (context_weights [B, K] or None) -> [B, N, C].
        attn_map: (fp32 [B, N, K], accumulate) - the block's head-mean cross-attention weights are stored / added there (K > 1).
        context_row_weights: the already-levelled regional form, effective weights e [B, N, K] >= 0 of token j at query row t (they
        hold the exemplar weights already, so context_weights must be None with them)."""
        x = _tokens(x)
        B, N, Cc = x.shape
        if context is None or context.dim() != 3 or context.shape[0] != B:
            raise PbeError("BasicTransformerBlock: the HIP path expects a context [B, K, D] with one row of K >= 1 tokens per sample")
        if context_row_weights is not None:
            if context_weights is not None:
                raise PbeError("BasicTransformerBlock: context_row_weights hold the exemplar weights already: give one of the two")
            table = prepare_row_weights(x.shape, context, context_row_weights)
            o = self.context_operands(context, None, regional=True)
            if isinstance(o, ops.CtxOperands):               # (K = 1: validated, otherwise ignored - the softmax over one key is 1)
                o = o.with_row_weights(table)
        else:
            o = self.context_operands(context, context_weights, maps=attn_map is not None)
        if attn_map is not None and isinstance(o, ops.CtxOperands):
            o = o.with_map(attn_map[0], attn_map[1])
        return self.run(x.view(B * N, Cc), B, N, o).view(B, N, Cc)


def compose_tail(wpo, bpo, wff, bff):
    """proj_out after ff-out as ONE linear map of [h | x2]: ([Wpo Wff | Wpo] fp16 [Cin, Kff + inner], Wpo bff + bpo fp32 [Cin]); the products in
    fp64 from the masters, rounded once."""
    with torch.no_grad():
        po = wpo.detach().double().reshape(wpo.shape[0], -1)
        w = torch.cat([po @ wff.detach().double(), po], 1)
        b = po @ bff.detach().double() + bpo.detach().double()
        return w.to(torch.float16).contiguous(), b.to(torch.float32).contiguous()


class SpatialTransformer(HipModule):
    """GroupNorm(eps 1e-6) -> 1x1 proj_in -> transformer block(s) -> 1x1 proj_out -> + input."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0., context_dim=None):
        super().__init__()
        self.in_channels = in_channels
        inner = n_heads * d_head
        self.norm = Normalize(in_channels)
        self.proj_in = nn.Conv2d(in_channels, inner, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, n_heads, d_head, dropout=dropout, context_dim=context_dim) for _ in range(depth)])
        self.proj_out = zero_module(nn.Conv2d(inner, in_channels, kernel_size=1, stride=1, padding=0))

    fold_groupnorm = True       # the GroupNorm rides on proj_in's A operand where x carries its producer's statistics (ops.gemm gn=); False: the separate pass (A/B runs)
    # The fold's dispatch bound, from profiles/stfold_shape_profile.txt: at C = 320 norm + proj_in take 15.7 + 22.4 us against 6.5 + 22.2 folded;
    # at C = 640 the table's 5 KB of LDS cost the tuned 64x128 tile its third workgroup per CU, 640 workgroups then run in two rounds and
    # the pair takes 7.3 + 30.4 us against 14.1 + 19.3: wider levels keep the separate pass (the kernel itself takes K <= 1280)
    fold_groupnorm_max_width = 320
    # proj_out composed into the last block's ff-out projection (_tail).  It changes low-order bits, so a stand-alone module keeps the two
    # launches and their bits (tests/golden/block_parent.npz pins them launch for launch); the U-Net switches it on for its transformers
    fold_tail = False

    def _pack(self):
        """proj_out composed into the last block's ff-out (both linear, both constant): with x3 = x2 + h Wff^T + bff,
        x + x3 Wpo^T + bpo = x + [h | x2] [Wpo Wff | Wpo]^T + (Wpo bff + bpo).  The products are formed in fp64 from the fp32 masters and
        rounded to fp16 once."""
        ns = SimpleNamespace(g=f32(self.norm.weight), b=f32(self.norm.bias), eps=self.norm.eps,
                             wi=ops.pack_linear(self.proj_in.weight), bi=f32(self.proj_in.bias),
                             wo=ops.pack_linear(self.proj_out.weight), bo=f32(self.proj_out.bias))
        ns.wt, ns.bt = compose_tail(self.proj_out.weight, self.proj_out.bias, self.transformer_blocks[-1].ff.net[2].weight,
                                    self.transformer_blocks[-1].ff.net[2].bias)
        return ns

    def _tail(self, p, x2d, N, cv):
        """The composed ff-out + proj_out operands for the LAST block, where it runs the LayerNorm-folded chain on a one-token constant
        (the fp8 and plain modes and the multi-token attn2 routes keep the two launches), else None."""
        blk = self.transformer_blocks[-1]
        if not (self.fold_tail and isinstance(cv, torch.Tensor) and blk._mode(N) == "folded"):
            return None
        return SimpleNamespace(w=p.wt, b=p.bt, resid=x2d)

    def context_vectors(self, context, context_weights=None, context_regions=None, maps=False):
        """Per block, what its run() needs of context [B, K, Dc]: the [B, C] constant for K = 1, the multi-token operands for K > 1
        (BasicTransformerBlock.context_operands).  context_weights: exemplar weights [B, K] (or a ContextWeights), validated once here.
        context_regions: region maps [B, K, Hr, Wr] (or a ContextRegions), validated once here; with them the result is a
        RegionalVectors (the list and the regions), which run() / run_paired() resolve at their grid.  maps: run() / run_paired() will
        be handed a ContextMaps, so a K > 1 context takes the fused kernel at every width (BasicTransformerBlock.context_operands)."""
        cw = prepare_context_weights(context, context_weights)
        cr = prepare_context_regions(context, context_regions, cw)
        vecs = [blk.context_operands(context, cw, regional=cr is not None, maps=bool(maps)) for blk in self.transformer_blocks]
        return vecs if cr is None else RegionalVectors(vecs, cr)

    @staticmethod
    def _levelled(ctx_vecs, H, W, maps=None):
        """The per-block list of ctx_vecs; a RegionalVectors gets the regions' table of the H x W grid on every multi-token block's
        operands (one-token constants: unchanged).  maps (a ContextMaps): every multi-token block's operands also get the level's
        accumulator as their attribution-map target, in accumulate mode, for the LAST maps.B samples of the operands' batch."""
        vecs = ctx_vecs
        if isinstance(ctx_vecs, RegionalVectors):
            vecs = ctx_vecs.vecs
            if any(isinstance(cv, ops.CtxOperands) for cv in vecs):      # (K = 1: validated, otherwise ignored)
                table = ctx_vecs.regions.level(H, W)
                vecs = [cv.with_row_weights(table) if isinstance(cv, ops.CtxOperands) else cv for cv in vecs]
        if maps is None:
            return vecs
        if any(isinstance(cv, ContextKV) for cv in vecs):
            raise PbeError("SpatialTransformer: attribution maps need the fused cross-attention kernel: build the context's operands with "
                           "context_vectors(..., maps=True)")
        multi = [cv for cv in vecs if isinstance(cv, ops.CtxOperands)]
        for cv in multi:
            if cv.Nk != maps.K or cv.B < maps.B:
                raise PbeError(f"SpatialTransformer: the ContextMaps collects {maps.B} samples x {maps.K} tokens, the context has {cv.B} x {cv.Nk}")
        acc = maps.level(H, W)
        maps.note(H, W, len(multi))                                      # (K = 1: the level is known, nothing is launched)
        return [cv.with_map(acc, True, cv.B - maps.B) if isinstance(cv, ops.CtxOperands) else cv for cv in vecs]

    def run(self, x, ctx_vecs, maps=None):
        """x [B, H, W, C] fp16 NHWC -> same shape; ctx_vecs = context_vectors(context); maps: a ContextMaps that collects the blocks'
        cross-attention weights at this grid (context_vectors(..., maps=True)), or None."""
        p = self.pk()
        B, H, W, Cc = x.shape
        N = H * W
        ctx_vecs = self._levelled(ctx_vecs, H, W, maps)
        x2d = x.view(B * N, Cc)
        h, st = self._proj_in(p, x, B, N)                                    # statistics for the first block's norm1
        tail = self._tail(p, x2d, N, ctx_vecs[-1])
        last = len(self.transformer_blocks) - 1
        for i, (blk, cv) in enumerate(zip(self.transformer_blocks, ctx_vecs)):
            h, st = blk.run(h, B, N, cv, stats=st, tail=tail if i == last else None), None
        if tail is not None:
            return h.view(B, H, W, Cc)
        return ops.gemm(h, p.wo, p.bo, resid=x2d).view(B, H, W, Cc)

    def _proj_in(self, p, x, B, N):
        """proj_in(GroupNorm(x)) -> (h, RowStats of h): the norm folded into the GEMM's A operand where x carries its producing conv's
        statistics (the launch falls back to the separate pass where no tile's rows divide N), else the norm's own launch(es)."""
        st = ops.group_stats_of(x, self.norm.num_groups) if self.fold_groupnorm and x.shape[-1] <= self.fold_groupnorm_max_width else None
        if st is not None:
            return ops.gemm(x.view(B * N, -1), p.wi, p.bi, row_stats=True, gn=(st, p.g, p.b, p.eps))
        return ops.gemm(ops.groupnorm(x, p.g, p.b, p.eps, False, groups=self.norm.num_groups).view(B * N, -1), p.wi, p.bi, row_stats=True)

    def run_paired(self, x, ctx_vecs, maps=None):
        """x [B, H, W, C] shared by the two halves of a guidance pair, ctx_vecs = context_vectors of the 2B contexts (one- or multi-token)
        -> [2B, H, W, C].  maps: as run(); a collector for B samples takes the second (conditional) half's own launch."""
        p = self.pk()
        B, H, W, Cc = x.shape
        N = H * W
        ctx_vecs = self._levelled(ctx_vecs, H, W, maps)
        x2d = x.view(B * N, Cc)
        with ops.pinned_batch_scale(2):
            h, st = self._proj_in(p, x, B, N)
        last = len(self.transformer_blocks) - 1
        # (depth > 1: the last block runs at batch 2B, where the shared residual has no row per sample of the second half: two launches)
        tail = self._tail(p, x2d, N, ctx_vecs[0]) if last == 0 else None
        h = self.transformer_blocks[0].run_paired(h, B, N, ctx_vecs[0], stats=st, tail=tail)
        if tail is not None:
            return h.view(2 * B, H, W, Cc)
        for blk, cv in zip(list(self.transformer_blocks)[1:], ctx_vecs[1:]):
            h = blk.run(h, 2 * B, N, cv)
        y = torch.empty((2 * B * N, Cc), dtype=torch.float16, device=x.device)
        with ops.pinned_batch_scale(2):
            for half in (0, 1):
                ops.gemm(h[half * B * N:(half + 1) * B * N], p.wo, p.bo, resid=x2d, out=y[half * B * N:(half + 1) * B * N])
        return y.view(2 * B, H, W, Cc)

    def forward(self, x, context=None, context_weights=None, context_regions=None, context_maps=None):
        """Reference layout: x [B, C, H, W], context [B, K, Dc] (K >= 1 tokens), context_weights [B, K] or None, context_regions
        [B, K, Hr, Wr] or None (H | Hr and W | Wr) -> [B, C, H, W].  context_maps: a ContextMaps that collects the attribution maps."""
        require_gpu(x, "SpatialTransformer")
        if context is None:
            raise PbeError("SpatialTransformer: context is required on the Paint-by-Example path")
        if context_maps is not None and context_maps.B is None:
            context_maps.bind(context.shape[0], context.shape[1], x.device)
        vecs = self.context_vectors(context, context_weights, context_regions, maps=context_maps is not None)
        return ops.nhwc_to_nchw(self.run(ops.nchw_to_nhwc(x.float()), vecs, context_maps)).to(x.dtype)
