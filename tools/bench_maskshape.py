#!/usr/bin/env python3
"""Time of the mask-shape kernels (pbe_amd/csrc/maskshape.hip) per picture, beside the project's other separable integer pass.

    python tools/bench_maskshape.py [--out profiles/maskshape_report.txt] [--reps 7] [--sizes 1024x1024,4096x4096,16384x8192] [--radii 8,64,512]

Per picture size (rows x columns), per radius r and per mask kind
  blobs    five filled rectangles, about 10 % of the area together: most pixels lie farther than r from the hole, so the row pass of the
           distance map takes all 2 r + 1 taps there
  dense    every pixel a hole pixel with probability 0.5, independently: every pixel has the set within a pixel or two, a few taps each
the columns are
  dist2    ops.mask_dist2(mask, to_hole=True, rmax=r)              (column pass + row pass)
  grow     ops.mask_grow(mask, r)                                  (dist2 + the threshold)
  close    ops.mask_close(mask, r)                                 (two of those)
  box      window.shape_mask(mask, box=True)                       (labelling, the component table READ BACK to the host, fill_boxes; blobs only:
                                                                    the dense mask has far more components than fill_boxes takes)
  feather  ops.feather_alpha(mask, (0, 0, Hs, Ws), r)              (the yardstick: four separable integer passes of csrc/window.hip, square element)
Device-event times around one call; median and 10 % / 90 % quantiles of `--reps` samples after 2 warm-up samples, in milliseconds.  A cell
that could not run (a workspace that does not fit, a limit of the entry point) holds the reason instead.

This measures TIME only; no threshold is set anywhere."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def make_mask(kind, hs, ws, dev):
    g = torch.Generator().manual_seed(hs + ws + len(kind))
    if kind == "dense":
        return (torch.rand((hs, ws), generator=g) < 0.5).to(torch.uint8).mul_(255).to(dev)
    mask = torch.zeros((hs, ws), dtype=torch.uint8)
    sh, sw = int(hs * 0.141), int(ws * 0.141)                          # 5 x 0.141^2 = 10 % of the area
    for fy, fx in ((0.05, 0.05), (0.05, 0.8), (0.43, 0.43), (0.8, 0.05), (0.8, 0.8)):
        mask[int(fy * hs):int(fy * hs) + sh, int(fx * ws):int(fx * ws) + sw] = 255
    return mask.to(dev)


def timed(fn, reps):
    out = []
    for i in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(a.elapsed_time(b))
    t = torch.tensor(out, dtype=torch.float64)
    return float(t.median()), float(t.quantile(0.1)), float(t.quantile(0.9))


def cell(fn, reps):
    """The timing of fn, or the reason it could not run: a limit of an entry point (PbeError) or a buffer that does not fit.  Anything else
    ends the run."""
    from pbe_amd.lib import PbeError
    try:
        q = timed(fn, reps)
    except (PbeError, torch.cuda.OutOfMemoryError) as e:
        return f"n/a ({type(e).__name__}: {str(e)[:40]})"
    return f"{q[0]:.3f} [{q[1]:.3f}, {q[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskshape_report.txt"), help="the table goes here too; '' = print only")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1024x1024,4096x4096,16384x8192")
    ap.add_argument("--radii", default="8,64,512")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_maskshape.py needs an MI355X: a timing taken anywhere else says nothing")
    from pbe_amd import ops
    from pbe_amd.window import shape_mask
    dev = torch.device("cuda:0")
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    radii = [int(v) for v in a.radii.split(",")]
    lines = [f"# tools/bench_maskshape.py on {torch.cuda.get_device_name(0)}: median [p10, p90] of {a.reps} samples, milliseconds per call",
             f"{'picture':>14s} {'mask':>6s} {'r':>4s} {'dist2 ms':>26s} {'grow ms':>26s} {'close ms':>26s} {'box ms':>26s} {'feather ms':>26s}"]
    print("\n".join(lines), flush=True)
    for hs, ws in sizes:
        for kind in ("blobs", "dense"):
            mask = make_mask(kind, hs, ws, dev)
            d2 = torch.empty((hs, ws), dtype=torch.int32, device=dev)
            out = torch.empty((hs, ws), dtype=torch.uint8, device=dev)
            box = cell(lambda: shape_mask(mask, box=True), a.reps) if kind == "blobs" else "-"
            for r in radii:
                cols = [cell(lambda: ops.mask_dist2(mask, True, r, out=d2), a.reps), cell(lambda: ops.mask_grow(mask, r, out=out), a.reps),
                        cell(lambda: ops.mask_close(mask, r, out=out), a.reps), box, cell(lambda: ops.feather_alpha(mask, (0, 0, hs, ws), r), a.reps)]
                lines.append(f"{f'{hs} x {ws}':>14s} {kind:>6s} {r:>4d} " + " ".join(f"{c:>26s}" for c in cols))
                print(lines[-1], flush=True)
                box = "\""
            del mask, d2, out
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
