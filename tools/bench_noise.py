#!/usr/bin/env python3
"""Time of the seeded noise draw (pbe_amd/csrc/noise.hip) per call, beside the draws it replaces.

    python tools/bench_noise.py [--out profiles/noise_timing.txt] [--reps 25] [--inner 50]

  randn_seeded        = ops.randn_seeded(seeds, shape, stream 0) into a preallocated tensor, seeds already on the device
  randn_seeded lists  = the same from a Python list of seeds (one small host-to-device copy per call)
  add (a = 1)         = the accumulate form, out += 0.3 z
  torch.randn device  = torch.randn(shape, device=...) on the device's global generator: x_T as the samplers draw it without seeds
  CPU draw + upload   = torch.randn(shape).to(device): the posterior noise as it is drawn without seeds (wall clock around a synchronise)
at [4, 4, 64, 64] (a 512 x 512 batch of 4) and [16, 4, 96, 96] (768 x 768, batch 16).  Device rows: the device-event time around `--inner`
back-to-back calls divided by `--inner`; median and the 10 % / 90 % quantiles of `--reps` samples after 3 warm-up samples, microseconds.

This measures TIME only, and the draw is a few launches per run: it is here so that the cost is known, not because it matters."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def timed(fn, reps, inner, wall=False):
    out = []
    for i in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            out.append((time.perf_counter() - t0) * 1e6 / inner if wall else a.elapsed_time(b) * 1e3 / inner)
    t = torch.tensor(out, dtype=torch.float64)
    return float(t.median()), float(t.quantile(0.1)), float(t.quantile(0.9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_noise.py needs an MI355X: a timing taken anywhere else says nothing")
    from pbe_amd import ops
    dev = torch.device("cuda:0")
    fmt = lambda t: f"{t[0]:.1f} [{t[1]:.1f}, {t[2]:.1f}]"      # noqa: E731
    lines = [f"# tools/bench_noise.py: median [p10, p90] of {a.reps} samples of {a.inner} calls each, microseconds per call; one run on one device",
             f"{'case':>44s} {'us':>28s}"]
    for shape in ((4, 4, 64, 64), (16, 4, 96, 96)):
        B = shape[0]
        ints = [1000 + i for i in range(B)]
        seeds = ops.seed_tensor(ints, B, dev)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        rows = (("randn_seeded", lambda: ops.randn_seeded(seeds, shape, 0, out=out), False),
                ("randn_seeded, seeds as a list", lambda: ops.randn_seeded(ints, shape, 0, out=out), False),
                ("randn_seeded add (a = 1)", lambda: ops.randn_seeded(seeds, shape, 16, out=out, a=1.0, b=0.3), False),
                ("torch.randn on the device", lambda: torch.randn(shape, device=dev), False),
                ("torch.randn on the CPU + upload (wall)", lambda: torch.randn(shape).to(dev), True))
        for name, fn, wall in rows:
            t = timed(fn, a.reps, a.inner, wall)
            lines.append(f"{f'{name} {list(shape)}':>44s} {fmt(t):>28s}")
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
