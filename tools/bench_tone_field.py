#!/usr/bin/env python3
"""Time of the tone field (pbe_amd/csrc/tone_field.hip, pbe_paste_window_field_u8) per call, beside tone_stats and the two other pastes.

    python tools/bench_tone_field.py [--out profiles/tone_field_timing.txt] [--reps 25] [--inner 20]

  cells       = ops.tone_cells (cell 8) on fp32 [B, 3, 512, 512] pictures with about 80 % of the pixels selected, B = 1 and 16, and on
                one 2048 x 2048 window (B = 1); beside it ops.tone_stats on the same tensors in the same run.  Both read 28 bytes per
                pixel by construction (seven fp32 planes); the GB/s column is that count over the median time.
  field       = ops.tone_field on the tables of the same sizes (grids 64 x 64, B = 1 and 16, and 256 x 256)
  paste       = ops.paste_window of one 512 x 512 result into a 512 x 512 window (scale 1), and of one 2048 x 2048 result into a
                2048 x 2048 window, alpha > 0 on about 30 % of the window: plain, tone=(gain, offset), field=
Each sample is the device-event time around `--inner` back-to-back repetitions divided by `--inner` (one repetition is too short for
the event clock); the table gives the median and the 10 % / 90 % quantiles of `--reps` samples after 3 warm-up samples, in
microseconds.  The tensors are small enough to stay in the caches between repetitions: the GB/s are not HBM rates.

This measures TIME only; it says nothing about the pictures."""
import argparse
import os
import sys

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
        raise SystemExit("tools/bench_tone_field.py needs an MI355X: a timing taken anywhere else says nothing")
    from pbe_amd import ops
    dev = torch.device("cuda:0")
    fmt = lambda t: f"{t[0]:.1f} [{t[1]:.1f}, {t[2]:.1f}]"      # noqa: E731
    lines = [f"# tools/bench_tone_field.py: median [p10, p90] of {a.reps} samples of {a.inner} repetitions each, microseconds per call;",
             "# GB/s = 28 bytes per pixel (what tone_cells and tone_stats read by construction) over the median",
             f"{'case':>34s} {'us':>28s} {'GB/s':>8s}"]

    def row(name, t, nbytes=None):
        lines.append(f"{name:>34s} {fmt(t):>28s} {'' if nbytes is None else format(nbytes / t[0] / 1e3, '.0f'):>8s}")
        print(lines[-1], flush=True)
    g = torch.Generator().manual_seed(3)
    for B, edge in ((1, 512), (16, 512), (1, 2048)):
        image = (torch.rand((B, 3, edge, edge), generator=g) * 2 - 1).to(dev)
        result = torch.rand((B, 3, edge, edge), generator=g).to(dev)
        sel = (torch.rand((B, 1, edge, edge), generator=g) < 0.8).float().to(dev)
        cells = torch.empty((B, 4, edge // 8, edge // 8), dtype=torch.int32, device=dev)
        stats = torch.empty((B, 3, 6), dtype=torch.int64, device=dev)
        field = torch.empty((B, 3, edge // 8, edge // 8), dtype=torch.float32, device=dev)
        nbytes = 28.0 * B * edge * edge
        row(f"tone_cells B = {B}, {edge} x {edge}", timed(lambda: ops.tone_cells(image, result, sel, 8, out=cells), a.reps, a.inner), nbytes)
        row(f"tone_stats B = {B}, {edge} x {edge}", timed(lambda: ops.tone_stats(image, result, sel, out=stats), a.reps, a.inner), nbytes)
        row(f"tone_field B = {B}, grid {edge // 8} x {edge // 8}", timed(lambda: ops.tone_field(cells, out=field), a.reps, a.inner))
        del image, result, sel
    for edge in (512, 2048):
        result = torch.rand((3, edge, edge), generator=g).to(dev)
        alpha = torch.rand((edge, edge), generator=g)
        alpha[torch.rand((edge, edge), generator=g) < 0.7] = 0.0
        alpha = alpha.to(dev)
        pic = torch.randint(0, 256, (edge, edge, 3), dtype=torch.uint8, generator=g).to(dev)
        fld = (torch.rand((3, edge // 8, edge // 8), generator=g) * 0.2 - 0.1).to(dev)
        win = (0, 0, edge, edge)
        for name, kw in (("paste_window", {}), ("paste_window tone", {"tone": TONE}), ("paste_window field", {"field": fld})):
            row(f"{name} {edge} x {edge}", timed(lambda: ops.paste_window(result, alpha, pic, win, **kw), a.reps, a.inner))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
