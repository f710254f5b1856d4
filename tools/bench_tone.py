#!/usr/bin/env python3
"""Time of the tone matching (pbe_amd/csrc/tone.hip, pbe_paste_window_tone_u8) per call, beside the plain paste.

    python tools/bench_tone.py [--out profiles/tone_timing.txt] [--reps 25] [--inner 20]

  stats       = ops.tone_stats on fp32 [B, 3, 512, 512] pictures with about 80 % of the pixels selected, B = 1 and 16, and on one
                2048 x 2048 window (B = 1)
  paste       = ops.paste_window of one 512 x 512 result into a 512 x 512 window (scale 1), and of one 2048 x 2048 result into a
                2048 x 2048 window, alpha > 0 on about 30 % of the window
  paste tone  = the same through tone=(gain, offset)
Each sample is the device-event time around `--inner` back-to-back repetitions divided by `--inner` (one repetition is too short for
the event clock); the table gives the median and the 10 % / 90 % quantiles of `--reps` samples after 3 warm-up samples, in
microseconds.  The host part (one read of the [B, 3, 6] table and pbe_amd.window.fit_tone) is timed once with the wall clock.

This measures TIME only; it says nothing about the pictures."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

TONE = ((1.05, 0.97, 1.02), (-0.01, 0.02, 0.0))


def timed(fn, reps, inner):
    out = []
    for i in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            out.append(a.elapsed_time(b) * 1e3 / inner)
    t = torch.tensor(out, dtype=torch.float64)
    return float(t.median()), float(t.quantile(0.1)), float(t.quantile(0.9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_tone.py needs an MI355X: a timing taken anywhere else says nothing")
    from pbe_amd import ops
    from pbe_amd.window import fit_tone
    dev = torch.device("cuda:0")
    fmt = lambda t: f"{t[0]:.1f} [{t[1]:.1f}, {t[2]:.1f}]"      # noqa: E731
    lines = [f"# tools/bench_tone.py: median [p10, p90] of {a.reps} samples of {a.inner} repetitions each, microseconds per call",
             f"{'case':>34s} {'us':>28s}"]
    g = torch.Generator().manual_seed(3)
    for B, edge in ((1, 512), (16, 512), (1, 2048)):
        image = (torch.rand((B, 3, edge, edge), generator=g) * 2 - 1).to(dev)
        result = torch.rand((B, 3, edge, edge), generator=g).to(dev)
        sel = (torch.rand((B, 1, edge, edge), generator=g) < 0.8).float().to(dev)
        stats = torch.empty((B, 3, 6), dtype=torch.int64, device=dev)
        t = timed(lambda: ops.tone_stats(image, result, sel, out=stats), a.reps, a.inner)
        lines.append(f"{f'tone_stats B = {B}, {edge} x {edge}':>34s} {fmt(t):>28s}")
        print(lines[-1], flush=True)
        if B == 16:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit_tone(stats.cpu())
            lines.append(f"{'table read + fit_tone, B = 16':>34s} {f'{(time.perf_counter() - t0) * 1e6:.0f} (wall clock, once)':>28s}")
            print(lines[-1], flush=True)
        del image, result, sel
    for edge in (512, 2048):
        result = torch.rand((3, edge, edge), generator=g).to(dev)
        alpha = torch.rand((edge, edge), generator=g)
        alpha[torch.rand((edge, edge), generator=g) < 0.7] = 0.0
        alpha = alpha.to(dev)
        pic = torch.randint(0, 256, (edge, edge, 3), dtype=torch.uint8, generator=g).to(dev)
        win = (0, 0, edge, edge)
        for name, tone in (("paste_window", None), ("paste_window tone", TONE)):
            t = timed(lambda: ops.paste_window(result, alpha, pic, win, tone=tone), a.reps, a.inner)
            lines.append(f"{f'{name} {edge} x {edge}':>34s} {fmt(t):>28s}")
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
