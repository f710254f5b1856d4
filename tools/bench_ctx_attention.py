#!/usr/bin/env python3
"""pbe_ctx_attention_f16 against the composition of kernels it replaces, on the U-Net's token shapes at the headline batch (2B = 8).

    python tools/bench_ctx_attention.py [--out profiles/ctx_attention_timing.txt] [--reps 25] [--inner 10]

Per (M, C) in (8*4096, 320), (8*1024, 640), (8*256, 1280), (8*64, 1280) and Nk in {2, 4, 16} context tokens (8 heads), one launch of
  fused        ops.ctx_attention: x + attn2(LayerNorm(x), ctx) and the row statistics of the result
  composition  ops.layernorm, ops.gemm (q projection), ops.attention over the Nk keys, ops.gemm (out projection, resid, row_stats)
  folded       the same with the LayerNorm folded into the q projection (what BasicTransformerBlock runs beyond the fused kernel's limits)
is timed with device events around `inner` back-to-back launches; the three variants alternate inside every repetition, the input rotates
over enough buffers that no launch re-reads what the previous one left in the caches (>= 512 MB in rotation, at most 16 buffers), and the
table gives the median and the 10 % / 90 % quantiles over the repetitions, per launch, in microseconds.  "spread" is (p90 - p10) / median
of the composition.  The variants' results are compared first (rel-L2 of fused against composition on the same operands).

    python tools/bench_ctx_attention.py --weights [--out profiles/ctx_weights_timing.txt]

times the exemplar-weight forms against their unweighted ones instead, arms alternating the same way: pbe_ctx_attention_w_f16 against
pbe_ctx_attention_f16 at the shapes above, and pbe_attention_kbias_f16 against pbe_attention_f16 at the cross-attention shapes the
existing-kernel route launches (a:8:8:256:4:160, a:8:8:64:4:160, a:8:8:4096:20:40).  Weights: exp2(randn), the last token of every
second sample absent.  "spread" is (p90 - p10) / median of the unweighted arm.

    python tools/bench_ctx_attention.py --regions [--out profiles/ctx_regions_timing.txt]

times the row-weight form (pbe_ctx_attention_rw_f16, launch key xar) against the weighted form (pbe_ctx_attention_w_f16, xaw) at the
shapes above, arms alternating the same way.  Table: exp2(randn) weights times uniform regions zeroed below 0.6 (about 60 % of the
entries -inf, rows without a token fall back to the weights), one [B, tokens, Nk] table per shape: it adds 4 Nk bytes per row to the
about 6 C the kernel moves.  "spread" is (p90 - p10) / median of the weighted arm.

    python tools/bench_ctx_attention.py --maps [--out profiles/ctx_maps_timing.txt]

times the map-emitting form (pbe_ctx_attention_map_f16, launch key xawm) against the form without the map (pbe_ctx_attention_w_f16, xaw)
at the shapes above, arms alternating the same way: the map stored, and the map accumulated (what the collector launches: the target is
read as well).  One fp32 [B, tokens, Nk] target per input buffer, rotating with it: 4 Nk bytes per row written (and read) beside the
about 6 C the kernel moves.  "spread" is (p90 - p10) / median of the arm without the map."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pbe_amd import ops  # noqa: E402

SHAPES = [(8 * 4096, 320), (8 * 1024, 640), (8 * 256, 1280), (8 * 64, 1280)]
TOKENS = (2, 4, 16)
B, H = 8, 8
LOG2E = 1.4426950408889634


def build(M, C, Nk, dev, g):
    """Operands of the three variants from one set of random weights: the composition's (g2, b2, wq, k, vt, wo, bo), the folded q pack,
    and the fused kernel's CtxOperands folded from them in fp32."""
    N, D = M // B, C // H
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    g2, b2 = 1.0 + 0.1 * r(C), 0.1 * r(C)
    wq, wo, bo = r(C, C) / C ** 0.5, r(C, C) / C ** 0.5, 0.1 * r(C)
    k, v = r(B, Nk, H, D).half().float(), r(B, Nk, H, D).half().float()
    scale = D ** -0.5
    kq = scale * LOG2E * torch.einsum("bjhd,hdc->bhjc", k, (wq * g2[None, :]).view(H, D, C)).reshape(B, H * Nk, C).half()
    kbias = scale * LOG2E * torch.einsum("bjhd,hd->bhj", k, (wq @ b2).view(H, D)).reshape(B, H * Nk)
    vo = torch.zeros(B, C, (H * Nk + 7) // 8 * 8, dtype=torch.float16)
    vo[:, :, :H * Nk] = torch.einsum("chd,bjhd->bchj", wo.view(C, H, D), v).reshape(B, C, H * Nk).half()
    oc = ops.CtxOperands(kq.to(dev), kq.double().sum(-1).float().to(dev), kbias.to(dev), vo.to(dev), bo.to(dev), H, Nk)
    npad = (Nk + 7) // 8 * 8
    vt = torch.zeros(B, C, npad, dtype=torch.float16)
    vt[:, :, :Nk] = v.permute(0, 2, 3, 1).reshape(B, C, Nk).half()
    wqg, c2, c1 = ops.pack_linear_ln(wq, None, g2, b2)
    comp = dict(g2=g2.to(dev), b2=b2.to(dev), wq=wq.half().to(dev), k=k.reshape(B * Nk, C).half().to(dev), vt=vt.to(dev), wo=wo.half().to(dev),
                bo=bo.to(dev), wqg=wqg.to(dev), c2=c2.to(dev), c1=c1.to(dev), N=N, D=D, Nk=Nk, npad=npad, scale=scale)
    return oc, comp


def composition(x, st, c, folded):
    N, D, Nk, C = c["N"], c["D"], c["Nk"], x.shape[1]
    if folded:
        q = ops.gemm(x, c["wqg"], c["c2"], ln=(st, c["c1"], 1e-5))
    else:
        q = ops.gemm(ops.layernorm(x, c["g2"], c["b2"], 1e-5), c["wq"])
    o = ops.attention(q, c["k"], c["vt"], B, H, N, Nk, D, c["scale"], q_strides=(N * C, C), k_strides=(Nk * C, C), vt_strides=(C * c["npad"], c["npad"]))
    return ops.gemm(o.view(B * N, C), c["wo"], c["bo"], resid=x, row_stats=True)


CROSS = [(256, 4, 160), (64, 4, 160), (4096, 20, 40)]          # (Nq, Nk, D) at B = 8, H = 8


def _time(variants, a, nbuf):
    """{name: [p10, median, p90]} microseconds per launch; the variants alternate inside every repetition."""
    for fn in variants.values():
        for w in range(a.warmup):
            fn(w % nbuf)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    it = 0
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn(it % nbuf)
                it += 1
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.inner * 1e3)
    return {k: torch.tensor(v).quantile(torch.tensor([0.1, 0.5, 0.9])).tolist() for k, v in times.items()}


def _log2w(Nk, dev, g):
    w = torch.exp2(torch.randn(B, Nk, generator=g))
    w[1::2, Nk - 1] = 0.0
    return torch.log2(w).float().to(dev)


def weights_table(a, dev):
    cell = lambda q: f"{q[1]:8.1f} [{q[0]:7.1f} .. {q[2]:7.1f}]"      # noqa: E731
    lines = [f"# exemplar-weight forms vs their unweighted forms; device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); "
             f"B = {B} samples, {H} heads",
             f"# per launch, microseconds: median [p10 .. p90] over {a.reps} repetitions of {a.inner} back-to-back launches, arms alternating",
             f"# pbe_ctx_attention_w_f16 vs pbe_ctx_attention_f16\n# {'M':>6} {'C':>5} {'Nk':>3} | {'unweighted':>28} | {'weighted':>28} | w/plain  spread"]
    g = torch.Generator().manual_seed(0)
    for M, C in SHAPES:
        nbuf = max(2, min(16, -(-(512 << 20) // (2 * M * C))))
        xs = [(torch.randn(M, C, generator=g) * 0.8 + 0.1).half().to(dev) for _ in range(nbuf)]
        sts = [ops.row_stats(x) for x in xs]
        for Nk in TOKENS:
            oc, _ = build(M, C, Nk, dev, g)
            ow = ops.CtxOperands(oc.kq, oc.colsum, oc.kbias, oc.vo, oc.bias, oc.H, oc.Nk, _log2w(Nk, dev, g))
            q = _time({"plain": lambda i: ops.ctx_attention(xs[i], oc, sts[i], 1e-5, tokens=M // B),
                       "w": lambda i: ops.ctx_attention(xs[i], ow, sts[i], 1e-5, tokens=M // B)}, a, nbuf)
            lines.append(f"  {M:6d} {C:5d} {Nk:3d} | {cell(q['plain']):>28} | {cell(q['w']):>28} | {q['w'][1] / q['plain'][1]:7.3f}  "
                         f"{(q['plain'][2] - q['plain'][0]) / q['plain'][1]:6.2f}")
            print(lines[-1], flush=True)
        del xs, sts
    lines.append(f"# pbe_attention_kbias_f16 vs pbe_attention_f16\n# {'launch':>20} | {'unbiased':>28} | {'key bias':>28} | kb/plain  spread")
    for Nq, Nk, D in CROSS:
        C = H * D
        npad = (Nk + 7) // 8 * 8
        nbuf = max(2, min(16, -(-(512 << 20) // (2 * B * Nq * C))))
        qs = [torch.randn(B * Nq, C, generator=g).half().to(dev) for _ in range(nbuf)]
        k = torch.randn(B * Nk, C, generator=g).half().to(dev)
        vt = torch.zeros(B, C, npad, dtype=torch.float16)
        vt[:, :, :Nk] = torch.randn(B, C, Nk, generator=g).half()
        vt, kb = vt.to(dev), _log2w(Nk, dev, g)
        outs = [torch.empty(B, Nq, C, dtype=torch.float16, device=dev) for _ in range(nbuf)]
        att = lambda i, bias: ops.attention(qs[i], k, vt, B, H, Nq, Nk, D, D ** -0.5, q_strides=(Nq * C, C), k_strides=(Nk * C, C),      # noqa: E731
                                            vt_strides=(C * npad, npad), out=outs[i], key_bias=bias)
        q = _time({"plain": lambda i: att(i, None), "kb": lambda i: att(i, kb)}, a, nbuf)
        lines.append(f"  {f'a:{B}:{H}:{Nq}:{Nk}:{D}':>20} | {cell(q['plain']):>28} | {cell(q['kb']):>28} | {q['kb'][1] / q['plain'][1]:8.3f}  "
                     f"{(q['plain'][2] - q['plain'][0]) / q['plain'][1]:6.2f}")
        print(lines[-1], flush=True)
    return "\n".join(lines) + "\n"


def regions_table(a, dev):
    cell = lambda q: f"{q[1]:8.1f} [{q[0]:7.1f} .. {q[2]:7.1f}]"      # noqa: E731
    lines = [f"# row-weight form vs the weighted form; device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); "
             f"B = {B} samples, {H} heads",
             f"# per launch, microseconds: median [p10 .. p90] over {a.reps} repetitions of {a.inner} back-to-back launches, arms alternating",
             f"# pbe_ctx_attention_rw_f16 (xar) vs pbe_ctx_attention_w_f16 (xaw)\n# {'M':>6} {'C':>5} {'Nk':>3} | {'xaw':>28} | {'xar':>28} | xar/xaw  spread"]
    g = torch.Generator().manual_seed(0)
    for M, C in SHAPES:
        nbuf = max(2, min(16, -(-(512 << 20) // (2 * M * C))))
        xs = [(torch.randn(M, C, generator=g) * 0.8 + 0.1).half().to(dev) for _ in range(nbuf)]
        sts = [ops.row_stats(x) for x in xs]
        for Nk in TOKENS:
            oc, _ = build(M, C, Nk, dev, g)
            lw = _log2w(Nk, dev, g)
            ow = ops.CtxOperands(oc.kq, oc.colsum, oc.kbias, oc.vo, oc.bias, oc.H, oc.Nk, lw)
            r = torch.rand(B, M // B, Nk, generator=g)
            e = torch.where(r < 0.6, torch.zeros_like(r), r) * torch.exp2(lw.cpu())[:, None, :]
            e = torch.where(e.sum(-1, keepdim=True) <= 0, torch.exp2(lw.cpu())[:, None, :].expand_as(e), e)
            orw = oc.with_row_weights(torch.log2(e).float().to(dev).contiguous())
            q = _time({"w": lambda i: ops.ctx_attention(xs[i], ow, sts[i], 1e-5, tokens=M // B),
                       "rw": lambda i: ops.ctx_attention(xs[i], orw, sts[i], 1e-5, tokens=M // B)}, a, nbuf)
            lines.append(f"  {M:6d} {C:5d} {Nk:3d} | {cell(q['w']):>28} | {cell(q['rw']):>28} | {q['rw'][1] / q['w'][1]:7.3f}  "
                         f"{(q['w'][2] - q['w'][0]) / q['w'][1]:6.2f}")
            print(lines[-1], flush=True)
        del xs, sts
    return "\n".join(lines) + "\n"


def maps_table(a, dev):
    cell = lambda q: f"{q[1]:8.1f} [{q[0]:7.1f} .. {q[2]:7.1f}]"      # noqa: E731
    lines = [f"# map-emitting form vs the form without the map; device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); "
             f"B = {B} samples, {H} heads",
             f"# per launch, microseconds: median [p10 .. p90] over {a.reps} repetitions of {a.inner} back-to-back launches, arms alternating",
             f"# pbe_ctx_attention_map_f16 (xawm: store / accumulate) vs pbe_ctx_attention_w_f16 (xaw)\n# {'M':>6} {'C':>5} {'Nk':>3} | {'xaw':>28} | "
             f"{'xawm store':>28} | {'xawm accumulate':>28} | store/xaw  acc/xaw  spread"]
    g = torch.Generator().manual_seed(0)
    for M, C in SHAPES:
        nbuf = max(2, min(16, -(-(512 << 20) // (2 * M * C))))
        xs = [(torch.randn(M, C, generator=g) * 0.8 + 0.1).half().to(dev) for _ in range(nbuf)]
        sts = [ops.row_stats(x) for x in xs]
        for Nk in TOKENS:
            oc, _ = build(M, C, Nk, dev, g)
            ow = ops.CtxOperands(oc.kq, oc.colsum, oc.kbias, oc.vo, oc.bias, oc.H, oc.Nk, _log2w(Nk, dev, g))
            maps = [torch.zeros(B, M // B, Nk, device=dev) for _ in range(nbuf)]
            q = _time({"w": lambda i: ops.ctx_attention(xs[i], ow, sts[i], 1e-5, tokens=M // B),
                       "st": lambda i: ops.ctx_attention(xs[i], ow, sts[i], 1e-5, tokens=M // B, attn_map=(maps[i], False)),
                       "acc": lambda i: ops.ctx_attention(xs[i], ow, sts[i], 1e-5, tokens=M // B, attn_map=(maps[i], True))}, a, nbuf)
            lines.append(f"  {M:6d} {C:5d} {Nk:3d} | {cell(q['w']):>28} | {cell(q['st']):>28} | {cell(q['acc']):>28} | {q['st'][1] / q['w'][1]:9.3f}  "
                         f"{q['acc'][1] / q['w'][1]:7.3f}  {(q['w'][2] - q['w'][0]) / q['w'][1]:6.2f}")
            print(lines[-1], flush=True)
            del maps
        del xs, sts
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--weights", action="store_true", help="time the exemplar-weight forms against the unweighted ones instead")
    ap.add_argument("--regions", action="store_true", help="time the row-weight form (xar) against the weighted form (xaw) instead")
    ap.add_argument("--maps", action="store_true", help="time the map-emitting form (xawm, store and accumulate) against the form without the map (xaw) instead")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ctx_attention.py needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    if a.weights or a.regions or a.maps:
        text = maps_table(a, dev) if a.maps else regions_table(a, dev) if a.regions else weights_table(a, dev)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    lines = [f"# pbe_ctx_attention_f16 vs the kernels it replaces; device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs); B = {B} samples, {H} heads",
             f"# per launch, microseconds: median [p10 .. p90] over {a.reps} repetitions of {a.inner} back-to-back launches, variants alternating; "
             "inputs rotate over >= 512 MB",
             f"# {'M':>6} {'C':>5} {'Nk':>3} | {'fused':>24} | {'composition (4 launches)':>28} | {'LN-folded q (3 launches)':>28} | fused/best  spread  rel-L2"]
    g = torch.Generator().manual_seed(0)
    for M, C in SHAPES:
        nbuf = max(2, min(16, -(-(512 << 20) // (2 * M * C))))
        xs = [(torch.randn(M, C, generator=g) * 0.8 + 0.1).half().to(dev) for _ in range(nbuf)]
        sts = [ops.row_stats(x) for x in xs]
        for Nk in TOKENS:
            oc, comp = build(M, C, Nk, dev, g)
            variants = {"fused": lambda i: ops.ctx_attention(xs[i], oc, sts[i], 1e-5, tokens=M // B),
                        "comp": lambda i: composition(xs[i], sts[i], comp, False),
                        "fold": lambda i: composition(xs[i], sts[i], comp, True)}
            ya, yb = variants["fused"](0)[0].double(), variants["comp"](0)[0].double()
            rel = ((ya - yb).norm() / yb.norm()).item()
            for fn in variants.values():
                for w in range(a.warmup):
                    fn(w % nbuf)
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            it = 0
            for _ in range(a.reps):
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        fn(it % nbuf)
                        it += 1
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) / a.inner * 1e3)
            q = {k: torch.tensor(v).quantile(torch.tensor([0.1, 0.5, 0.9])).tolist() for k, v in times.items()}
            best = min(q["comp"][1], q["fold"][1])
            cell = lambda k: f"{q[k][1]:8.1f} [{q[k][0]:7.1f} .. {q[k][2]:7.1f}]"      # noqa: E731
            lines.append(f"  {M:6d} {C:5d} {Nk:3d} | {cell('fused'):>24} | {cell('comp'):>28} | {cell('fold'):>28} | {q['fused'][1] / best:9.2f}  "
                         f"{(q['comp'][2] - q['comp'][0]) / q['comp'][1]:6.2f}  {rel:.1e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
