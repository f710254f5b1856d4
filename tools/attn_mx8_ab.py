"""fp16 vs MX-fp8 attention core on the same device, interleaved (pbe_attention_f16 vs pbe_quant_mx8_f16 + pbe_attention_mx8).

    python tools/attn_mx8_ab.py [--reps 20] [--rounds 7] [--no-sampler] [--out FILE]   (default FILE: results/attn_mx8_ab.json)

Kernel legs, one launch each per rep, the two cores alternating rep by rep, median over rounds:
  64x64 level N 4 096, d 40; 32x32 level N 1 024, d 80; 16x16 level N 256, d 160; 96x96 latents N 9 216, d 40 (B*H = 64 each).
The MX-fp8 core is timed alone (operands quantised once) and with its three quantiser launches (q, k, V^T).
Projection legs, same levels and device, interleaved per rep group, median over rounds: the LayerNorm-folded q|k|v^T projection plus
the core as (a) fp16 projection + fp16 core, (b) fp16 projection + 3 quantiser launches + MX core (the path before the MX copy-out),
(c) MX-out projection (pbe_gemm_mx8out_f16) + MX core.
Sampler legs: attention fp8 alone at 512x512 (64x64 latents, guidance, B = 1, 50 PLMS steps): fp16, attention fp8 through the
quantisers (CrossAttention.mx8_from_projection = False) and through the MX-out projection, alternating; and the configs[4] geometry (96x96 latents, guidance, B = 4) PLMS passes with linear fp8 alone and with linear + attention fp8,
alternating; reports ms per sampler step (one guidance-pair U-Net evaluation) and the images/s of a 100-step run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOG2E = 1.4426950408889634


def _elapsed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def kernel_legs(dev, reps, rounds):
    from pbe_amd import ops
    out = []
    for name, N, D in (("64x64", 4096, 40), ("32x32", 1024, 80), ("16x16", 256, 160), ("96x96", 9216, 40)):
        B, H = 8, 8
        inner = H * D
        g = torch.Generator().manual_seed(N + D)
        qk = (torch.randn(B * N, 2 * inner, generator=g) * 1.5).half().to(dev)
        npad = (N + 7) // 8 * 8
        vt = torch.randn(B, inner, npad, generator=g).half().to(dev)
        scale = D ** -0.5
        kw = dict(q_strides=(N * 2 * inner, 2 * inner), k_strides=(N * 2 * inner, 2 * inner), vt_strides=(inner * npad, npad))

        def quant():
            return (ops.quant_mx8(qk, B, H, N, D, rs=2 * inner, alpha=scale * LOG2E), ops.quant_mx8(qk[:, inner:], B, H, N, D, rs=2 * inner),
                    ops.quant_mx8(vt, B, H, N, D, rs=npad, vt=True))
        q8, k8, v8 = quant()
        f16 = lambda: ops.attention(qk, qk[:, inner:], vt, B, H, N, N, D, scale, **kw)       # noqa: E731
        f8 = lambda: ops.attention_mx8(q8, k8, v8, 1.0)                                      # noqa: E731
        f8q = lambda: ops.attention_mx8(*quant(), 1.0)                                      # noqa: E731
        for f in (f16, f8, f8q):
            f()
        torch.cuda.synchronize()
        t = {"fp16": [], "mx8": [], "mx8+quant": []}
        for _ in range(rounds):
            for k, f in (("fp16", f16), ("mx8", f8), ("mx8+quant", f8q)):
                t[k].append(_elapsed(f, reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"level": name, "N": N, "D": D, "BH": B * H, "us_fp16": round(med["fp16"], 1), "us_mx8": round(med["mx8"], 1),
               "us_mx8_with_quant": round(med["mx8+quant"], 1), "speedup_kernel": round(med["fp16"] / med["mx8"], 3),
               "speedup_with_quant": round(med["fp16"] / med["mx8+quant"], 3),
               "spread_us": {k: round(max(v) - min(v), 1) for k, v in t.items()}}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def projection_legs(dev, reps, rounds):
    from pbe_amd import ops
    out = []
    for name, N, D in (("64x64", 4096, 40), ("32x32", 1024, 80), ("16x16", 256, 160), ("96x96", 9216, 40)):
        B, H = 8, 8
        C = inner = H * D
        g = torch.Generator().manual_seed(N + D)
        x = (torch.randn(B * N, C, generator=g) * 2).half().to(dev)
        W = (torch.randn(3 * C, C, generator=g) / C ** 0.5).to(dev)
        w, c2, c1 = ops.pack_linear_ln(W, None, (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev))
        qs = D ** -0.5 * LOG2E
        c2[:C] *= qs
        stats = ops.row_stats(x)
        qk = torch.empty((B * N, 2 * inner), dtype=torch.float16, device=dev)
        vt = torch.empty((B, inner, N), dtype=torch.float16, device=dev)
        kw = dict(q_strides=(N * 2 * inner, 2 * inner), k_strides=(N * 2 * inner, 2 * inner), vt_strides=(inner * N, N), q_prescaled=True)

        def proj():
            ops.gemm(x, w, c2, ln=(stats, c1, 1e-5), alpha=qs, alpha_cols=C, out=qk, vt=vt, vt_col0=2 * inner, vt_tokens=N)

        def f16():
            proj()
            return ops.attention(qk, qk[:, inner:], vt, B, H, N, N, D, D ** -0.5, **kw)

        def quant():
            proj()
            return ops.attention_mx8(ops.quant_mx8(qk, B, H, N, D, rs=2 * inner), ops.quant_mx8(qk[:, inner:], B, H, N, D, rs=2 * inner),
                                     ops.quant_mx8(vt, B, H, N, D, rs=N, vt=True), 1.0)

        def mx8out():
            return ops.attention_mx8(*ops.qkv_mx8(x, w, c2, ln=(stats, c1, 1e-5), B=B, H=H, N=N, D=D, alpha=qs, alpha_cols=C), 1.0)
        legs = (("fp16", f16), ("quant", quant), ("mx8out", mx8out))
        for _, f in legs:
            f()
        torch.cuda.synchronize()
        t = {k: [] for k, _ in legs}
        for _ in range(rounds):
            for k, f in legs:
                t[k].append(_elapsed(f, reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"level": name, "N": N, "D": D, "BH": B * H, "us_proj_fp16_core_fp16": round(med["fp16"], 1),
               "us_proj_fp16_quant_core_mx8": round(med["quant"], 1), "us_proj_mx8out_core_mx8": round(med["mx8out"], 1),
               "mx8out_vs_quant": round(med["quant"] / med["mx8out"], 3), "mx8out_vs_fp16": round(med["fp16"] / med["mx8out"], 3),
               "spread_us": {k: round(max(v) - min(v), 1) for k, v in t.items()}}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def _arms(arms, run, rounds):
    """Alternate the (name, setup) arms rep by rep after one warm-up each; median ms per step."""
    res = {k: [] for k, _ in arms}
    for _, setup in arms:
        setup()
        run()
    for _ in range(rounds):
        for k, setup in arms:
            setup()
            res[k].append(run())
    return res


def sampler_512_leg(dev, steps, rounds):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import modelbuild
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.modules.attention import CrossAttention
    from pbe_amd.precision import set_attention_precision
    with torch.no_grad():
        model = modelbuild.full_model(dev, parts=("unet",))
    B = 1
    g = torch.Generator().manual_seed(37)
    xT = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    z = (torch.randn(B, 4, 64, 64, generator=g) * 0.8).to(dev)
    m = torch.ones(B, 1, 64, 64)
    m[:, :, 20:46, 14:40] = 0
    m = m.to(dev)
    c, uc = torch.randn(B, 1, 768, generator=g).to(dev), torch.randn(B, 1, 768, generator=g).to(dev)

    def run():
        smp = PLMSSampler(model)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            smp.sample(S=steps, batch_size=B, shape=[4, 64, 64], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                       unconditional_conditioning=uc, eta=0.0, x_T=xT, test_model_kwargs={"inpaint_image": z, "inpaint_mask": m})
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def arm(att, mx):
        def setup():
            set_attention_precision(model, att)
            CrossAttention.mx8_from_projection = mx
        return setup
    try:
        res = _arms((("fp16", arm("fp16", True)), ("attention_fp8_quant", arm("fp8", False)), ("attention_fp8_mx8out", arm("fp8", True))),
                    run, rounds)
    finally:
        set_attention_precision(model, "fp16")
        CrossAttention.mx8_from_projection = True
    out = {}
    for k, v in res.items():
        ms = statistics.median(v)
        out[k] = {"ms_per_run": round(ms, 1), "images_per_s": round(B / (ms / 1e3), 4), "spread_ms": round(max(v) - min(v), 1)}
    out["mx8out_vs_quant"] = round(out["attention_fp8_quant"]["ms_per_run"] / out["attention_fp8_mx8out"]["ms_per_run"], 4)
    out["mx8out_vs_fp16"] = round(out["fp16"]["ms_per_run"] / out["attention_fp8_mx8out"]["ms_per_run"], 4)
    print(json.dumps({"sampler_512_50_steps": out}), flush=True)
    return out


def sampler_leg(dev, steps, rounds):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import modelbuild
    from ldm.models.diffusion.plms import PLMSSampler
    from pbe_amd.precision import set_attention_precision, set_linear_precision
    with torch.no_grad():
        model = modelbuild.full_model(dev, parts=("unet",))
    B = 4
    g = torch.Generator().manual_seed(31)
    xT = torch.randn(B, 4, 96, 96, generator=g).to(dev)
    z = (torch.randn(B, 4, 96, 96, generator=g) * 0.8).to(dev)
    m = torch.ones(B, 1, 96, 96)
    m[:, :, 30:70, 20:60] = 0
    m = m.to(dev)
    c, uc = torch.randn(B, 1, 768, generator=g).to(dev), torch.randn(B, 1, 768, generator=g).to(dev)

    def run():
        smp = PLMSSampler(model)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            smp.sample(S=steps, batch_size=B, shape=[4, 96, 96], conditioning=c, verbose=False, unconditional_guidance_scale=5.0,
                       unconditional_conditioning=uc, eta=0.0, x_T=xT, test_model_kwargs={"inpaint_image": z, "inpaint_mask": m})
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (steps + 1) * 1e3        # PLMS: S + 1 U-Net evaluations

    from ldm.modules.attention import CrossAttention
    set_linear_precision(model, "fp8")

    def arm(att, mx):
        def setup():
            set_attention_precision(model, att)
            CrossAttention.mx8_from_projection = mx
        return setup
    try:
        res = _arms((("linear_fp8", arm("fp16", True)), ("linear+attention_fp8_quant", arm("fp8", False)),
                            ("linear+attention_fp8", arm("fp8", True))), run, rounds)
    finally:
        set_attention_precision(model, "fp16")
        set_linear_precision(model, "fp16")
        CrossAttention.mx8_from_projection = True
    out = {}
    for k, v in res.items():
        ms = statistics.median(v)
        out[k] = {"ms_per_step": round(ms, 2), "images_per_s_100_steps": round(B / (101 * ms / 1e3), 4), "spread_ms": round(max(v) - min(v), 2)}
    out["speedup"] = round(out["linear_fp8"]["ms_per_step"] / out["linear+attention_fp8"]["ms_per_step"], 4)
    print(json.dumps({"sampler_configs4_geometry": out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sampler-rounds", type=int, default=3)
    ap.add_argument("--no-sampler", action="store_true")
    ap.add_argument("--only", choices=("kernels", "sampler"), default=None, help="run the kernel / projection legs or the sampler legs only")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "attn_mx8_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only != "sampler":
        res["kernels"] = kernel_legs(dev, a.reps, a.rounds)
        res["projection"] = projection_legs(dev, a.reps, a.rounds)
    if not a.no_sampler and a.only != "kernels":
        res["sampler_512"] = sampler_512_leg(dev, 50, a.sampler_rounds)
        res["sampler"] = sampler_leg(dev, a.steps, a.sampler_rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
