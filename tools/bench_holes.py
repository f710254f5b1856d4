#!/usr/bin/env python3
"""Time of the hole kernels (pbe_amd/csrc/holes.hip) per mask, beside the host path they replace.

    python tools/bench_holes.py [--out profiles/holes_timing.txt] [--reps 15] [--inner 5]

Per mask size (1024 x 1024, 4096 x 4096, 8192 x 8192) and per mask kind
  blobs   five filled rectangles, about 10 % of the area together
  dense   every pixel a hole pixel with probability 0.5, independently (hundreds of thousands of components at 4096 x 4096)
the columns are
  label    ops.mask_components at connectivity 8                          (three launches)
  boxes    pbe_component_boxes_i32 alone, capacity = the mask's component count (no read-back: the entry point, not the wrapper)
  select   ops.select_components of the first four labels
  hole_box window.hole_box on the same device tensor: the device-to-host copy of the whole mask and the numpy pass that
           pipeline.inpaint_window makes per sample, in wall-clock time (it synchronises)
The kernel columns are device-event times around `--inner` back-to-back repetitions divided by `--inner`; median and 10 % / 90 %
quantiles of `--reps` samples after 3 warm-up samples, in microseconds.  `components` is the count the boxes kernel returned; a `*`
behind it says that it exceeds the largest capacity, 2^20, so that the boxes column holds the counting pass alone.

This measures TIME only; no threshold is set anywhere."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SIZES = (1024, 4096, 8192)


def make_mask(kind, n, dev):
    g = torch.Generator().manual_seed(n + len(kind))
    if kind == "dense":
        return (torch.rand((n, n), generator=g) < 0.5).to(torch.uint8).mul_(255).to(dev)
    mask = torch.zeros((n, n), dtype=torch.uint8)
    side = int(n * 0.141)                                            # 5 x 0.141^2 = 10 % of the area
    for fy, fx in ((0.05, 0.05), (0.05, 0.8), (0.43, 0.43), (0.8, 0.05), (0.8, 0.8)):
        mask[int(fy * n):int(fy * n) + side, int(fx * n):int(fx * n) + side] = 255
    return mask.to(dev)


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
    return quantiles(out)


def quantiles(samples):
    t = torch.tensor(samples, dtype=torch.float64)
    return float(t.median()), float(t.quantile(0.1)), float(t.quantile(0.9))


def cell(q):
    return f"{q[0]:.1f} [{q[1]:.1f}, {q[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holes_timing.txt"), help="the table goes here too; '' = print only")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_holes.py needs an MI355X: a timing taken anywhere else says nothing")
    from pbe_amd import lib, ops
    from pbe_amd.window import hole_box
    dev = torch.device("cuda:0")
    handle = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# tools/bench_holes.py: connectivity 8; median [p10, p90] of {a.reps} samples of {a.inner} repetitions each, microseconds per mask "
             "(hole_box: wall clock of one call, it copies the mask to the host)",
             f"{'mask':>18s} {'components':>10s} {'label us':>26s} {'boxes us':>26s} {'select us':>26s} {'hole_box us':>30s}"]
    for n in SIZES:
        for kind in ("blobs", "dense"):
            mask = make_mask(kind, n, dev)
            labels = torch.empty((n, n), dtype=torch.int32, device=dev)
            sel = torch.empty((n, n), dtype=torch.uint8, device=dev)
            ops.mask_components(mask, 8, out=labels)
            count = int((labels == torch.arange(n * n, dtype=torch.int32, device=dev).view(n, n)).sum())
            cap = min(max(count, 1), 1 << 20)
            table = torch.empty((cap, 6), dtype=torch.int32, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            ws = torch.empty(handle.pbe_component_boxes_workspace_bytes(n, n, cap), dtype=torch.uint8, device=dev)
            wanted = [int(v) for v in torch.unique(labels[labels >= 0])[:4]]

            def boxes():
                lib.check(handle.pbe_component_boxes_i32(labels.data_ptr(), table.data_ptr(), cnt.data_ptr(), n, n, cap, ws.data_ptr(), ws.numel(), stream), "boxes")
            t_label = timed(lambda: ops.mask_components(mask, 8, out=labels), a.reps, a.inner)
            t_boxes = timed(boxes, a.reps, a.inner)
            if int(cnt.cpu()[0]) != count:
                raise SystemExit(f"tools/bench_holes.py: the boxes kernel counted {int(cnt.cpu()[0])} components, the labels hold {count}")
            t_select = timed(lambda: ops.select_components(labels, wanted, out=sel), a.reps, a.inner)
            host = []
            for i in range(a.reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hole_box(mask)
                if i >= 3:
                    host.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"{f'{n} x {n} {kind}':>18s} {str(count) + ('*' if count > cap else ''):>10s} {cell(t_label):>26s} {cell(t_boxes):>26s} {cell(t_select):>26s} {cell(quantiles(host)):>30s}")
            print(lines[-1], flush=True)
            del mask, labels, sel, table, ws
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
