#!/usr/bin/env python3
"""Time of the exemplar kernels (pbe_amd/csrc/exemplar.hip) per picture, beside the host path they can replace.

    python tools/bench_exemplar.py [--out profiles/exemplar_timing.txt] [--reps 15] [--inner 5]

Per picture (the three bundled reference JPEGs, random pictures of 512 x 512 and 4096 x 4096, and a 600 x 600 box of the latter), all
resized to 224 x 224 with the bicubic filter, the columns are
  kernels    pbe_resample_h_u8 + pbe_resample_v_u8 (with the planes) alone, tables already on the device: device-event time around
             `--inner` back-to-back repetitions divided by `--inner`
  ops        ops.resample_u8 on the resident picture: the host tables, their upload and the launches; wall clock, synchronised
  up + ops   the picture's full-size bytes from host memory to the device, then ops.resample_u8; wall clock, synchronised
  host       what load_triple_device does with a decoded picture (a PIL image, made before the clock starts): Image.resize on the CPU,
             the 224 x 224 bytes to the device, ops.u8_to_planes; wall clock, synchronised (with a box: Image.resize(box=))
  mask_box   ops.mask_box of a mask of the picture's size (it reads the band table back); wall clock
  hole_box   window.hole_box of the same device mask (it copies the mask to the host); wall clock
Decoding is in none of them.  Median and 10 % / 90 % quantiles of `--reps` samples after 3 warm-up samples, in microseconds.  The
device results are compared with the host's bytes before anything is timed.

This measures TIME only; no threshold is set anywhere."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def quantiles(samples):
    t = torch.tensor(samples, dtype=torch.float64)
    return float(t.median()), float(t.quantile(0.1)), float(t.quantile(0.9))


def events(fn, reps, inner):
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


def wall(fn, reps):
    out = []
    for i in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 3:
            out.append((time.perf_counter() - t0) * 1e6)
    return quantiles(out)


def cell(q):
    return f"{q[0]:.1f} [{q[1]:.1f}, {q[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exemplar_timing.txt"), help="the table goes here too; '' = print only")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_exemplar.py needs an MI355X: a timing taken anywhere else says nothing")
    import ctypes
    from PIL import Image
    from pbe_amd import exemplar, lib, ops
    from pbe_amd.window import hole_box
    dev = torch.device("cuda:0")
    handle, stream = lib.load(), torch.cuda.current_stream().cuda_stream
    golden = os.path.join(ROOT, "tests", "golden", "examples")
    rng = np.random.default_rng(0)
    pictures = [(f"reference_example_{i}.jpg", np.array(Image.open(os.path.join(golden, f"reference_example_{i}.jpg")).convert("RGB"), dtype=np.uint8), None)
                for i in (1, 2, 3)]
    big = rng.integers(0, 256, size=(4096, 4096, 3), dtype=np.uint8)
    pictures += [("random 512 x 512", rng.integers(0, 256, size=(512, 512, 3), dtype=np.uint8), None), ("random 4096 x 4096", big, None),
                 ("the same, box 600 x 600", big, (1000, 2000, 1600, 2600))]
    mean, std = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)
    lines = [f"# tools/bench_exemplar.py: -> 224 x 224 bicubic; median [p10, p90] of {a.reps} samples, microseconds per picture (kernels: device events over "
             f"{a.inner} repetitions; the rest: wall clock of one synchronised call)",
             f"{'picture (H x W)':>40s} {'kernels us':>24s} {'ops us':>26s} {'up + ops us':>28s} {'host us':>28s} {'mask_box us':>24s} {'hole_box us':>28s}"]
    for name, pic, box in pictures:
        Hs, Ws = pic.shape[:2]
        d = torch.from_numpy(pic).to(dev)
        host_u8 = np.array(Image.fromarray(pic).resize((224, 224), box=box), dtype=np.uint8)
        got, _ = ops.resample_u8(d, (224, 224), box=box, mean=CLIP_MEAN, std=CLIP_STD)
        if not np.array_equal(got.cpu().numpy(), host_u8):
            raise SystemExit(f"tools/bench_exemplar.py: {name}: the device bytes differ from Pillow's")
        x0, y0, x1, y1 = exemplar.validate_box(box, (Hs, Ws))
        bh, kh = exemplar.resample_tables(Ws, x0, x1, 224, "bicubic")
        bv, kv = exemplar.resample_tables(Hs, y0, y1, 224, "bicubic")
        first, last = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
        bv[:, 0] -= first
        dbh, dkh, dbv, dkv = (torch.from_numpy(t).to(dev) for t in (bh, kh, bv, kv))
        tmp = torch.empty(handle.pbe_resample_workspace_bytes(last - first, 224), dtype=torch.uint8, device=dev)
        out, planes = torch.empty((224, 224, 3), dtype=torch.uint8, device=dev), torch.empty((3, 224, 224), dtype=torch.float32, device=dev)

        def kernels():
            lib.check(handle.pbe_resample_h_u8(d.data_ptr(), None, None, tmp.data_ptr(), Hs, Ws, first, last, 224, dbh.data_ptr(), dkh.data_ptr(), kh.shape[1],
                                               stream), "h")
            lib.check(handle.pbe_resample_v_u8(tmp.data_ptr(), None, None, out.data_ptr(), planes.data_ptr(), last - first, 224, 224, dbv.data_ptr(),
                                               dkv.data_ptr(), kv.shape[1], mean, std, stream), "v")
        kernels()
        torch.cuda.synchronize()
        if not np.array_equal(out.cpu().numpy(), host_u8):
            raise SystemExit(f"tools/bench_exemplar.py: {name}: the two launches alone differ from Pillow's bytes")

        img = Image.fromarray(pic)                                    # the decoded picture, as Image.open(...).convert("RGB") leaves it

        def host():
            u8 = np.array(img.resize((224, 224), box=box), dtype=np.uint8)
            return ops.u8_to_planes(torch.from_numpy(u8).to(dev)[None], CLIP_MEAN, CLIP_STD)
        mask = torch.zeros((Hs, Ws), dtype=torch.uint8, device=dev)
        mask[Hs // 3:Hs // 2, Ws // 4:Ws // 2] = 255
        t = (events(kernels, a.reps, a.inner), wall(lambda: ops.resample_u8(d, (224, 224), box=box, mean=CLIP_MEAN, std=CLIP_STD), a.reps),
             wall(lambda: ops.resample_u8(torch.from_numpy(pic).to(dev), (224, 224), box=box, mean=CLIP_MEAN, std=CLIP_STD), a.reps), wall(host, a.reps),
             wall(lambda: ops.mask_box(mask), a.reps), wall(lambda: hole_box(mask), a.reps))
        lines.append(f"{f'{name} ({Hs} x {Ws})':>40s} {cell(t[0]):>24s} {cell(t[1]):>26s} {cell(t[2]):>28s} {cell(t[3]):>28s} {cell(t[4]):>24s} {cell(t[5]):>28s}")
        print(lines[-1], flush=True)
        del d, tmp, mask
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
