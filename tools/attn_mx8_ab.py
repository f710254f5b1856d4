"""fp16 vs MX-fp8 attention core on the same device, interleaved (pbe_attention_f16 vs pbe_quant_mx8_f16 + pbe_attention_mx8).

    python tools/attn_mx8_ab.py [--reps 20] [--rounds 7] [--no-sampler] [--out FILE]   (default FILE: results/attn_mx8_ab.json)

Kernel legs, one launch each per rep, the two cores alternating rep by rep, median over rounds:
  64x64 level N 4 096, d 40; 32x32 level N 1 024, d 80; 16x16 level N 256, d 160; 96x96 latents N 9 216, d 40 (B*H = 64 each).
The MX-fp8 core is timed alone (operands quantised once) and with its three quantiser launches (q, k, V^T).
Sampler leg: configs[4] geometry (96x96 latents, guidance, B = 4) PLMS passes with linear fp8 alone and with linear + attention fp8,
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

    set_linear_precision(model, "fp8")
    res = {"linear_fp8": [], "linear+attention_fp8": []}
    try:
        for k, a in (("linear_fp8", "fp16"), ("linear+attention_fp8", "fp8")):
            set_attention_precision(model, a)
            run()                                                        # warm-up (packs, first launches)
        for _ in range(rounds):
            for k, a in (("linear_fp8", "fp16"), ("linear+attention_fp8", "fp8")):
                set_attention_precision(model, a)
                res[k].append(run())
    finally:
        set_attention_precision(model, "fp16")
        set_linear_precision(model, "fp16")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "attn_mx8_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernel_legs(dev, a.reps, a.rounds)}
    if not a.no_sampler:
        res["sampler"] = sampler_leg(dev, a.steps, a.sampler_rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
