#!/usr/bin/env python3
"""Sampler time of PLMS at 50 steps (51 U-Net calls) against DPM-Solver++(2M) at 20 steps (20 calls) on the headline geometry.

    python tools/bench_samplers.py [--out profiles/dpm_solver_timing.txt] [--reps 9] [--warmup 2]

One process, the model of bench.py (configs/v1.yaml, name-seeded weights) and its inputs (B = 4 synthetic 512 x 512 triples, scale 5).
Each arm is one pipeline.inpaint(timings=) pass; `sampler_ms` is the device-event time between the end of the VAE encode and the start
of the VAE decode, i.e. the whole denoising loop.  Both arms are warmed up (`--warmup` passes each: code objects, packs, the per-step
embedding rows), then alternate inside every repetition; the table gives the median and the 10 % / 90 % quantiles over the repetitions
and "spread" = (p90 - p10) / median.  The expectation from the call counts is 20 / 51 = 0.392 of the PLMS sampler time.

This measures TIME only.  It says nothing about the pictures: on name-seeded weights no sampler's quality can be judged, and the quality
of 20 DPM-Solver++ steps on a trained checkpoint is not verified here."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

ARMS = (("plms", 50, 51), ("dpm", 20, 20))          # (pipeline sampler, steps, U-Net calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--scale", type=float, default=5.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_samplers.py needs an MI355X: a timing taken anywhere else says nothing")
    import cases
    from ldm.util import instantiate_from_config, load_yaml_config
    from pbe_amd.pipeline import inpaint
    from pbe_amd.weights import fill_latent_diffusion_
    dev = torch.device("cuda:0")
    model = instantiate_from_config(load_yaml_config(os.path.join(ROOT, "configs", "v1.yaml"))["model"])
    fill_latent_diffusion_(model)
    model = model.to(dev).eval()
    inp = {k: v.to(dev) for k, v in cases.synthetic_triples(a.batch, 512).items()}

    def one(sampler, steps):
        t = {}
        out = inpaint(model, inp["image"], inp["mask"], inp["ref"], steps=steps, scale=a.scale, x_T=inp["x_T"], post_eps=inp["post_eps"],
                      sampler=sampler, timings=t)
        if not bool(torch.isfinite(out["latent"]).all()):
            raise SystemExit(f"tools/bench_samplers.py: non-finite latent from {sampler}")
        return t["sampler_ms"], sum(t.values())

    with torch.no_grad():
        for _ in range(a.warmup):
            for name, steps, _ in ARMS:
                one(name, steps)
        torch.cuda.synchronize()
        smp = {name: [] for name, _, _ in ARMS}
        tot = {name: [] for name, _, _ in ARMS}
        for _ in range(a.reps):
            for name, steps, _ in ARMS:
                s, t = one(name, steps)
                smp[name].append(s)
                tot[name].append(t)
    q = lambda v: torch.tensor(v, dtype=torch.float64).quantile(torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64)).tolist()      # noqa: E731
    p = torch.cuda.get_device_properties(0)
    lines = [f"# sampler_ms of pipeline.inpaint(timings=): PLMS 50 steps vs DPM-Solver++(2M) 20 steps; device: {torch.cuda.get_device_name(0)} "
             f"({p.gcnArchName}); B = {a.batch}, 512 x 512, scale {a.scale:g}, name-seeded weights",
             f"# milliseconds per batch: median [p10 .. p90] over {a.reps} repetitions after {a.warmup} warm-up passes per arm, arms alternating in one process",
             f"# {'arm':>8} {'steps':>5} {'calls':>5} | {'sampler_ms':>28} | {'ms per call':>11} | {'all stages ms':>28} | spread"]
    med = {}
    for name, steps, calls in ARMS:
        s, t = q(smp[name]), q(tot[name])
        med[name] = (s[1], t[1])
        lines.append(f"  {name:>8} {steps:5d} {calls:5d} | {s[1]:8.1f} [{s[0]:7.1f} .. {s[2]:7.1f}]    | {s[1] / calls:11.2f} | {t[1]:8.1f} [{t[0]:7.1f} .. {t[2]:7.1f}]    | "
                     f"{(s[2] - s[0]) / s[1]:6.3f}")
    lines.append(f"# dpm / plms: sampler_ms {med['dpm'][0] / med['plms'][0]:.3f} (call counts: 20 / 51 = {20 / 51:.3f}); all stages "
                 f"{med['dpm'][1] / med['plms'][1]:.3f}; images/s over all stages: plms {1e3 * a.batch / med['plms'][1]:.2f}, dpm {1e3 * a.batch / med['dpm'][1]:.2f}")
    lines.append("# time only: the quality of 20 DPM-Solver++ steps on a trained checkpoint is not verified (name-seeded weights here)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
