#!/usr/bin/env python3
"""Time of the windowed pre- and post-processing (pbe_amd/csrc/window.hip) per picture, beside the sampler time of the same inpaint call.

    python tools/bench_window.py [--out profiles/window_timing.txt] [--reps 25] [--inner 20] [--no-sampler]

Per picture size (1024 x 1024, 2048 x 2048, 4096 x 3072; a rectangular hole of about 10 % of the area in the middle; default context 0.5
and feather 8; working size 512 x 512):
  pre   = ops.window_image + ops.window_mask + ops.mul_planes          (what pipeline.window_inputs launches for one picture)
  post  = ops.feather_alpha + ops.paste_window                         (on a 512 x 512 result; the picture is pasted in place)
Each sample is the device-event time around `--inner` back-to-back repetitions divided by `--inner` (one repetition is too short for
the event clock); the table gives the median and the 10 % / 90 % quantiles of `--reps` samples after 3 warm-up samples, in
microseconds.  `sampler_ms` is the denoising loop of one pipeline.inpaint_window call (configs/v1.yaml, name-seeded weights, one
picture of the first size, 50 PLMS steps, scale 5) after one warm-up call: the time the two columns stand beside.

This measures TIME only; it says nothing about the pictures."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

SIZES = ((1024, 1024), (2048, 2048), (4096, 3072))
WORKING = (512, 512)


def picture_and_mask(Hs, Ws, dev):
    g = torch.Generator().manual_seed(Hs * 7 + Ws)
    pic = torch.randint(0, 256, (Hs, Ws, 3), dtype=torch.uint8, generator=g)
    mask = torch.zeros((Hs, Ws), dtype=torch.uint8)
    bh, bw = int(Hs * 0.316), int(Ws * 0.316)                       # 0.316^2 = 10 % of the area
    mask[(Hs - bh) // 2:(Hs - bh) // 2 + bh, (Ws - bw) // 2:(Ws - bw) // 2 + bw] = 255
    return pic.to(dev), mask.to(dev)


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
    ap.add_argument("--no-sampler", action="store_true", help="skip the model: the kernel columns only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_window.py needs an MI355X: a timing taken anywhere else says nothing")
    from pbe_amd import ops, pipeline
    from pbe_amd.window import plan_window
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_window.py: working size {WORKING[0]} x {WORKING[1]}, context 0.5, feather 8, hole = 10 % of the area; "
             f"median [p10, p90] of {a.reps} samples of {a.inner} repetitions each, microseconds per picture",
             f"{'picture':>12s} {'window (y0, x0, wh, ww)':>28s} {'pre us':>28s} {'post us':>28s}"]
    result = torch.rand((3, *WORKING), generator=torch.Generator().manual_seed(1)).to(dev)
    first = None
    for Hs, Ws in SIZES:
        pic, mask = picture_and_mask(Hs, Ws, dev)
        win = plan_window(mask, WORKING)
        first = first or (pic, mask)
        image = torch.empty((1, 3, *WORKING), dtype=torch.float32, device=dev)
        keep = torch.empty((1, 1, *WORKING), dtype=torch.float32, device=dev)
        alpha = torch.empty((win[2], win[3]), dtype=torch.float32, device=dev)
        work = pic.clone()

        def pre():
            ops.window_image(pic, win, WORKING, out=image[0])
            ops.window_mask(mask, win, WORKING, out=keep[0])
            ops.mul_planes(image, keep)

        def post():
            ops.feather_alpha(mask, win, 8, out=alpha)
            ops.paste_window(result, alpha, work, win)
        p, q = timed(pre, a.reps, a.inner), timed(post, a.reps, a.inner)
        lines.append(f"{f'{Hs} x {Ws}':>12s} {str(win):>28s} {f'{p[0]:.1f} [{p[1]:.1f}, {p[2]:.1f}]':>28s} {f'{q[0]:.1f} [{q[1]:.1f}, {q[2]:.1f}]':>28s}")
        print(lines[-1], flush=True)
    if not a.no_sampler:
        import cases
        from ldm.util import instantiate_from_config, load_yaml_config
        from pbe_amd.weights import fill_latent_diffusion_
        model = instantiate_from_config(load_yaml_config(os.path.join(ROOT, "configs", "v1.yaml"))["model"])
        fill_latent_diffusion_(model)
        model = model.to(dev).eval()
        inp = {k: v.to(dev) for k, v in cases.synthetic_triples(1, 512).items()}
        with torch.no_grad():
            for i in range(2):
                t = {}
                out = pipeline.inpaint_window(model, [first[0]], [first[1]], inp["ref"], size=WORKING, steps=50, scale=5.0, x_T=inp["x_T"],
                                              post_eps=inp["post_eps"], timings=t)
        if not bool(torch.isfinite(out["latent"]).all()):
            raise SystemExit("tools/bench_window.py: non-finite latent")
        lines.append(f"sampler_ms of the same inpaint_window call ({SIZES[0][0]} x {SIZES[0][1]} picture, batch 1, 50 PLMS steps, scale 5): {t['sampler_ms']:.1f} ms "
                     f"(clip {t['clip_ms']:.1f}, vae encode {t['vae_encode_ms']:.1f}, vae decode {t['vae_decode_ms']:.1f})")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
