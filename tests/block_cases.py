"""Every path of BasicTransformerBlock on one small transformer: helpers shared by tests/test_block_paths_gpu.py and
tools/record_block_golden.py (which wrote tests/golden/block_parent.npz with the tree BEFORE the block's paths were merged into one stage
chain).  Plain functions.

The fixture is SpatialTransformer(320, 8, 40, depth=2, context_dim=768) with EVERY parameter drawn from a seeded CPU generator (proj_out
too: zero_module leaves it at zero, which would hide everything) at B = 2, so a guidance pair is 4 samples.  Two blocks, because in a pair
the second block takes the single path at batch 2B, on statistics it has to compute itself.  Two grids: 8 x 8 (N = 64: the LayerNorm fold,
and with attn_fp8 the MX copy-out) and 5 x 5 (N = 25, N % 8 != 0: the fold is refused, the plain chain runs, V^T is padded to 32).

Every case runs as st.run(cat([x, x]), vecs) and as st.run_paired(x, vecs).  Of each run the golden file keeps the output's digest
(prologue_cases.digest), the ordered GEMM launches (ops._PLANS: key, tile, split-K, BM, BN, workgroups) and the launch count of every
kernel class (ops.prof_collect), and whether the two runs were equal.
"""
from __future__ import annotations

import json
import math
import zlib

import numpy as np
import torch

from prologue_cases import digest  # noqa: F401  (re-exported: the recorder and the test digest with it)

B, C, HEADS, DHEAD, DEPTH, CTX_DIM, K = 2, 320, 8, 40, 2, 768, 4
BLOCK_SWITCHES = ("linear_fp8", "fold_layernorm", "ctx_fused_max_width")     # set on each BasicTransformerBlock
ATTN_SWITCHES = ("attn_fp8", "mx8_from_projection")                          # set on each block's attn1


def specs():
    out = []

    def add(name, grid, **kw):
        out.append(dict(id=f"{name}-{grid}x{grid}", grid=grid, tokens=kw.pop("tokens", 1), weights=kw.pop("weights", None),
                        regions=kw.pop("regions", False), maps=kw.pop("maps", False), switches=kw))

    for g in (8, 5):
        add("one", g)                                                       # 8x8: folded; 5x5: plain
    add("one-nofold", 8, fold_layernorm=False)
    for g in (8, 5):
        add("one-linf8", g, linear_fp8=True)
    add("one-attnf8-proj", 8, attn_fp8=True, mx8_from_projection=True)
    add("one-attnf8-quant", 8, attn_fp8=True, mx8_from_projection=False)
    add("one-linf8-attnf8", 8, linear_fp8=True, attn_fp8=True)
    for g in (8, 5):                                                        # the fused cross-attention kernel; 5x5: the block computes the statistics
        add("k4-fused", g, tokens=K)
        add("k4-fused-w0", g, tokens=K, weights="zero")
    for g in (8, 5):                                                        # ContextKV route (q projection / key-bias attention / to_out) at a 320-wide block
        add("k4-kv-w", g, tokens=K, weights="positive", ctx_fused_max_width=64)
    add("k4-regions", 8, tokens=K, regions=True)
    add("k4-maps", 8, tokens=K, maps=True)                                  # collector bound to B: the conditional half, per-range launches
    return out


def _seed(text):
    return zlib.crc32(text.encode()) & 0x7FFFFFFF


def transformer(dev):
    """The seeded fixture on `dev` (default switches)."""
    from ldm.modules.attention import SpatialTransformer
    st = SpatialTransformer(C, HEADS, DHEAD, depth=DEPTH, context_dim=CTX_DIM)
    g = torch.Generator().manual_seed(_seed("block-paths-parameters"))
    with torch.no_grad():
        for name, p in st.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if p.dim() > 1:
                p.copy_(r / math.sqrt(p[0].numel()))
            elif name.endswith("weight"):                                   # norm gains
                p.copy_(1.0 + 0.1 * r)
            else:
                p.copy_(0.1 * r)
    return st.to(dev)


def set_switches(st, switches):
    """Every switch of the fixture's blocks: the case's value, or the class default."""
    for blk in st.transformer_blocks:
        for n in BLOCK_SWITCHES:
            setattr(blk, n, switches.get(n, getattr(type(blk), n)))
        for n in ATTN_SWITCHES:
            setattr(blk.attn1, n, switches.get(n, getattr(type(blk.attn1), n)))


def inputs(spec, dev):
    """(x [B, g, g, C] fp16 NHWC, context [2B, tokens, CTX_DIM] fp16, exemplar weights [2B, tokens] or None, region maps
    [2B, tokens, 8, 8] or None), from a CPU generator seeded by the case id."""
    g = torch.Generator().manual_seed(_seed(spec["id"]))
    n, k = spec["grid"], spec["tokens"]
    x = torch.randn(B, n, n, C, generator=g).half().to(dev)
    ctx = torch.randn(2 * B, k, CTX_DIM, generator=g).half().to(dev)
    w = None
    if spec["weights"] is not None:
        w = 0.25 + 2.0 * torch.rand(2 * B, k, generator=g)
        if spec["weights"] == "zero":
            w[0, 1] = 0.0                                                   # one exemplar absent in one sample
    r = None
    if spec["regions"]:
        r = torch.rand(2 * B, k, 8, 8, generator=g)
        r[:, 0, :4] = 0.0                                                   # token 0 absent from the upper half
        r[:, 1:, 6:, 6:] = 0.0                                              # a corner only token 0 covers
    return x, ctx, w, r


def _recorded(fn):
    """fn() -> (result, ordered GEMM plans, {kernel class: launches})."""
    from pbe_amd import ops
    torch.cuda.synchronize()
    try:
        ops.prof_reset()
        ops.prof_enable(True)
        ops._PLANS = []
        y = fn()
        plans = ops._PLANS
    finally:
        ops._PLANS = None
        ops.prof_enable(False)
    torch.cuda.synchronize()
    counts = {k: v["launches"] for k, v in ops.prof_collect().items() if v["launches"]}
    ops.prof_reset()
    return y, [list(p) for p in plans], counts


def run(spec, st, dev):
    """Both runs of a case -> {"run" | "paired": dict(out=[tensors], plans=[..], counts={..})}.  With maps each run has a collector of
    its own and its accumulator is the second output."""
    from ldm.modules.attention import ContextMaps
    set_switches(st, spec["switches"])
    x, ctx, w, r = inputs(spec, dev)
    n = spec["grid"]
    res = {}
    for which in ("run", "paired"):
        cm = ContextMaps().bind(B, spec["tokens"], dev) if spec["maps"] else None
        vecs = st.context_vectors(ctx, w, r, maps=cm is not None)
        if which == "run":
            xx = torch.cat([x, x], 0)
            y, plans, counts = _recorded(lambda: st.run(xx, vecs, cm))
        else:
            y, plans, counts = _recorded(lambda: st.run_paired(x, vecs, cm))
        res[which] = dict(out=[y] + ([cm.level(n, n)] if cm is not None else []), plans=plans, counts=counts)
    return res


def launch_record(r):
    """The launch record of one run as the golden file keeps it: a JSON string."""
    return json.dumps(dict(plans=r["plans"], counts=r["counts"]), sort_keys=True)


def as_array(text):
    return np.frombuffer(text.encode(), dtype=np.uint8).copy()
