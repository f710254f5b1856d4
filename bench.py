#!/usr/bin/env python3
"""bench.py — Paint-by-Example PLMS hot path on MI355X.

One "step" = one full pass of the hot path over one batch of synthetic 512x512 triples per GPU:
CLIP exemplar encode + VAE encode + 50 PLMS steps (51 U-Net calls at batch 2B under classifier-free
guidance, scale 5) + VAE decode.  Inputs (image / mask / exemplar / x_T / posterior
noise) are resident in HBM before the timed region.  Weights: name-seeded random init of the
configs/v1.yaml architecture (no checkpoint exists offline).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (driver, N > 1)

Prints ONE JSON line on rank 0: metric, value (images/s of the whole job), unit, higher_is_better, dtype, ms_per_step, the config,
e2e_mfma_frac and, when N > 1, per_rank_ms and startup.  A plain run does nothing else: set-up, warm-up, the timed steps,
--dump-outputs, the line.

--full adds the measurements that take passes of their own after the timed region (`extra_legs`; --no-profile, --no-batch16 and
--no-cpu-baseline trim them):
  stage_ms_per_batch  one more step with per-stage events (CLIP, VAE encode, sampler, VAE decode), and unet_ms_per_step_per_image
  roofline     the kernel class with the most GPU time (3x3-conv implicit GEMM or the Linear GEMM, both MFMA): algorithmic
               FLOP per launch / average launch duration, measured with HIP events on the launch stream in a separate
               profiled pass AFTER the timed region (pbe_prof_*), against 2.5 PFLOP/s dense fp16; `classes` holds the same
               for every kernel class plus `frac_of_binding_roofline` (per launch: max(FLOP / peak, bytes / 8 TB/s)).
  batch16      BASELINE configs[2]'s size (16 per GPU), 1 warm-up + 2 timed steps, beside the headline (N = 1, headline config)
  cpu_baseline the CPU oracle (a port: oracle/pbe_oracle.py, fp32 torch) timed on this box's host
               cores on a bounded sample (warm-up + 3 CFG U-Net pairs, median; VAE enc/dec + CLIP for one image),
               extrapolated to images/sec; CPU model and physical core count reported.  Rank 0, N = 1 only.

--dump-outputs DIR writes what the LAST timed step returned (rank 0) as DIR/<name>.npy, float32: the `inpaint` dict (image, latent,
c, z_inpaint, mask_lat; rank 0's own shard) and image_u8, the uint8 images the step hands back (all ranks' when N > 1).  Inputs and
weights are seeded, so the same arguments give the same inputs on every run and two builds can be compared file for file.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4, help="images per GPU per step (BASELINE config #2: 4)")
    ap.add_argument("--plms-steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=5.0)
    ap.add_argument("--image-size", type=int, default=512, choices=(512, 768), help="768 = BASELINE configs[4] geometry (96x96 latents)")
    ap.add_argument("--precision", default="fp16", choices=("fp16", "fp8"),
                    help="fp8 = BASELINE configs[4]: e4m3 operands for the LayerNorm-fed projections (pbe_amd.precision); not the headline config")
    ap.add_argument("--weights", default="broadcast", choices=("broadcast", "local"),
                    help="N > 1: rank 0 synthesises and broadcasts over RCCL (default, the north-star's step) or every rank synthesises its own copy")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure the stage split, the per-kernel-class roofline, batch 16 and the CPU baseline")
    ap.add_argument("--no-batch16", action="store_true", help="--full: skip the extra BASELINE configs[2]-size (batch 16) measurement")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-profile", action="store_true", help="--full: skip the per-kernel-class profiled pass (roofline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's outputs as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--rehearse-launch", action="store_true",
                    help="tests only: workers rendezvous (gloo), all-reduce one number and rank 0 prints a JSON line; no GPU work")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def self_launch(a) -> int:
    """`python bench.py --gpus N` with N > 1 and no RANK in the environment: this process becomes a pure launcher.
    It starts N workers (one per GPU: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set) BEFORE importing torch or touching
    HIP in any way, waits for them, and returns non-zero if any worker failed.  Rank 0 inherits stdout, so its single
    JSON line is the launcher's output; the other ranks' stdout goes to stderr.  Nothing is exec'ed: the workers are
    child processes, and a failed worker takes the rest down (exact PIDs) instead of leaving them in a rendezvous."""
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    alive = set(range(a.gpus))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"[bench] rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr, flush=True)
                for o in sorted(alive):
                    procs[o].terminate()
        if alive:
            time.sleep(0.2)
    return rc


if __name__ == "__main__" and "RANK" not in os.environ:
    _a = parse_args()
    if _a.gpus > 1:
        sys.exit(self_launch(_a))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# algorithmic FLOP per image at the headline config = 85.08e12 (51*2*796.94 + 1116.7 + 2514.5 + 155.5 + 0.13 GFLOP); main() computes it
MFMA_PEAK_TFLOPS = 2500.0          # dense fp16/bf16, MI355X_MICROARCH.md "Chip-level parameters"
HBM_PEAK_TBS = 8.0                 # HBM3E spec, same table (6.3 TB/s is what a streaming copy reaches)


DUMP_BYTES = 64_000_000 - 64 * 1024       # --dump-outputs: array payload cap (64 MB in all, .npy headers included)


def dump_outputs(path, arrays):
    """arrays: name -> tensor, written as path/<name>.npy in float32.  Arrays that fit their share of DUMP_BYTES are written whole;
    a larger one is cut to a fixed, seeded sample of its flattened elements (sorted indices from one seed: identical for identical
    shapes, so two runs stay comparable element for element).  Returns {name: (full shape, elements written)}."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    left, info = DUMP_BYTES, {}
    names = sorted(host, key=lambda k: host[k].size)                  # small arrays first: they are kept whole
    for i, k in enumerate(names):
        x = host[k]
        share = left // 4 // (len(names) - i)
        flat = x.reshape(-1)
        if flat.size > share:
            flat = flat[np.sort(np.random.default_rng(0).choice(flat.size, share, replace=False))]
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(flat if flat.size < x.size else x, dtype=np.float32))
        left -= 4 * flat.size
        info[k] = (list(x.shape), int(flat.size))
    return info


def extra_legs(a, world, rank):
    """The measurements this rank makes after the timed region.  None without --full; with it, every one that applies to the
    configuration and was not switched off.  `stage` and `profile` run on every rank (a step gathers images across ranks)."""
    if not a.full:
        return set()
    headline = a.image_size == 512 and a.precision == "fp16" and a.plms_steps == 50
    legs = {"stage"}
    if not a.no_profile:
        legs.add("profile")
    if world == 1 and rank == 0 and headline and not a.no_batch16 and a.batch != 16:
        legs.add("batch16")
    if world == 1 and rank == 0 and headline and not a.no_cpu_baseline:
        legs.add("cpu_baseline")
    return legs


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench] {msg}", file=sys.stderr, flush=True)


def build_model(device, rank, world, weights="broadcast"):
    """weights = "broadcast" (the north-star's step): rank 0 synthesises the name-seeded weights, the other ranks
    allocate empty storage and receive them through ONE bucketed RCCL broadcast (fp32 masters, 1 GiB buckets over xGMI);
    "local": every rank synthesises its own copy concurrently (name-seeded = bit-identical by construction; no rank waits for rank 0's
    14-23 s of CPU work) and a 2-number checksum all-reduce proves the copies agree.  Either way the packs are built per rank."""
    from ldm.util import instantiate_from_config, load_yaml_config
    from pbe_amd.shard import broadcast_weights_, weights_checksum
    from pbe_amd.weights import fill_latent_diffusion_
    cfg = load_yaml_config(os.path.join(ROOT, "configs", "v1.yaml"))["model"]
    cpu_sd = None
    t0 = time.time()
    info = {"weights": weights if world > 1 else "single rank"}
    if rank == 0 or weights == "local":
        model = instantiate_from_config(cfg)
        fill_latent_diffusion_(model)
        if world == 1:
            # fp32 CPU copy for the oracle baseline, held on plain runs too: without it the host tensors are freed while the
            # weights move to the device, which made set-up about 9 s slower on the MI355X host
            cpu_sd = {k: v for k, v in model.state_dict().items()}
        model = model.to(device).eval()
    else:
        with torch.device("meta"):
            model = instantiate_from_config(cfg)
        model = model.to_empty(device=device).eval()
        model.register_schedule(linear_start=0.00085, linear_end=0.0120, timesteps=1000)
        model = model.to(device)
    info["build_s"] = time.time() - t0
    log(f"model built in {info['build_s']:.1f}s")
    if world > 1:
        t0 = time.time()
        if weights == "broadcast":
            b = broadcast_weights_(model, src=0)
            torch.cuda.synchronize()
            info.update(broadcast_gb=b["bytes"] / 1e9, broadcast_messages=int(b["messages"]), broadcast_s=time.time() - t0)
            log(f"weight broadcast: {info['broadcast_gb']:.2f} GB in {info['broadcast_messages']} messages, {info['broadcast_s']:.2f}s")
        info["weights_identical_on_all_ranks"] = weights_checksum(model)
    model.prepare()
    return model, cpu_sd, info


def cpu_info():
    """CPU model string and physical core count of the box (BASELINE.md section 3 asks for both beside the baseline)."""
    model, cores = "unknown", set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name") and model == "unknown":
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    phys = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
    except OSError:
        pass
    return model, len(cores) or (os.cpu_count() or 1)


def cpu_baseline(cpu_sd, threads, pairs=3):
    """Time the oracle (fp32 torch restatement of the reference) on the host: bounded sample.  One untimed warm-up CFG pair, then
    `pairs` timed pairs (median reported), VAE encode / decode and CLIP once each."""
    import statistics
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pbe_oracle as O
    import cases
    torch.set_num_threads(threads)
    inp = cases.synthetic_triples(1, 512)
    with torch.no_grad():
        t0 = time.time()
        c = O.learned_conditioning(cpu_sd, inp["ref"])
        t_clip = time.time() - t0
        t0 = time.time()
        z = O.first_stage_encode(cpu_sd, inp["image"] * inp["mask"], inp["post_eps"], prefix="first_stage_model.")
        t_enc = time.time() - t0
        x9 = torch.cat([inp["x_T"], z, O.resize_mask(inp["mask"], (64, 64))], 1)
        ctx = torch.cat([cpu_sd["learnable_vector"].float(), c])
        t_pairs = []
        for i in range(pairs + 1):                           # first one is the warm-up (allocator, thread pool, oneDNN primitives)
            t0 = time.time()
            O.unet_forward(cpu_sd, torch.cat([x9] * 2), torch.full((2,), 981 - 20 * i, dtype=torch.int64), ctx, prefix="model.diffusion_model.")
            t_pairs.append(time.time() - t0)
        t_pair = statistics.median(t_pairs[1:])
        t0 = time.time()
        O.first_stage_decode(cpu_sd, inp["x_T"] * 0.18215, prefix="first_stage_model.")
        t_dec = time.time() - t0
    per_image = 51 * t_pair + t_enc + t_dec + t_clip
    model, phys = cpu_info()
    return {"value": 1.0 / per_image, "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": f"warm-up + {pairs} timed CFG U-Net pairs (median {t_pair:.2f}s; all {', '.join('%.2f' % t for t in t_pairs[1:])}; warm-up {t_pairs[0]:.2f}s) "
                      f"+ VAE encode ({t_enc:.2f}s) + decode ({t_dec:.2f}s) + CLIP+mapper ({t_clip:.2f}s) for one 512x512 image, fp32 oracle; "
                      f"extrapolated x51 U-Net pairs",
            "unet_s_per_step_per_image": t_pair, "cpu_model": model, "physical_cores": phys, "threads_used": threads}


def measured_traffic():
    """profiles/igemm_traffic.json (tools/pmc_bench_traffic.py over rocprofv3 --pmc passes of THIS command) - only when it was
    taken with the library sources and tile table this run uses; otherwise (None, reason)."""
    import hashlib
    from pbe_amd import lib
    path = os.path.join(ROOT, "profiles", "igemm_traffic.json")
    if not os.path.exists(path):
        return None, "no profiles/igemm_traffic.json"
    with open(path) as f:
        tj = json.load(f)
    with open(os.path.join(ROOT, "pbe_amd", "tuned_mi355x.json"), "rb") as f:
        table = hashlib.sha256(f.read()).hexdigest()[:16]
    if tj.get("source_hash") != lib.source_hash() or tj.get("tuned_table_sha") != table:
        return None, f"stale: taken with sources {tj.get('source_hash')} / table {tj.get('tuned_table_sha')}, this run uses {lib.source_hash()} / {table}"
    return tj, "profiles/igemm_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes over this command)"


def main():
    a = parse_args()

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:          # checked before anything touches the GPU
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}; run `python bench.py --gpus N` (self-launching) "
                         "or torch.distributed.run with --nproc-per-node equal to --gpus")
    if os.environ.get("PBE_BENCH_FAIL_RANK") == str(rank):          # tests only: a worker that dies before the rendezvous
        raise SystemExit(3)
    backend = os.environ.get("PBE_DIST_BACKEND", "nccl")
    if a.rehearse_launch:        # tests only (tests/test_shard_gloo.py): the launch / rendezvous / relay path without a GPU
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        per_rank = [10.0 * (rank + 1)]
        if world > 1:
            dist.init_process_group("gloo")
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            mine = torch.tensor([10.0 * (rank + 1)], dtype=torch.float64)          # the per-rank timing exchange of the real run
            allr = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allr, mine)
            per_rank = [float(x.item()) for x in allr]
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"rehearsal": True, "n_gpus": world, "rank_sum": float(t.item()), "steps": a.steps, "warmup": a.warmup,
                              "per_rank_ms": {"min": min(per_rank), "max": max(per_rank), "all": per_rank}}), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # one process per GPU.  PBE_DIST_BACKEND=gloo + fewer GPUs than ranks is a REHEARSAL mode only
    # (ranks share a card): it exercises the sharding / broadcast / gather code on a 1-GPU box.
    ndev = torch.cuda.device_count()
    dev_index = local if (backend == "nccl" or local < ndev) else local % ndev
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)          # RCCL over xGMI
        else:
            dist.init_process_group(backend)

    import cases
    from pbe_amd import ops
    from pbe_amd.pipeline import inpaint
    from pbe_amd.shard import gather_images

    legs = extra_legs(a, world, rank)
    model, cpu_sd, build_info = build_model(device, rank, world, a.weights)
    if a.precision == "fp8":
        from pbe_amd.precision import set_linear_precision
        set_linear_precision(model, "fp8")
    B = a.batch
    inp = {k: v.to(device) for k, v in cases.synthetic_triples(B, a.image_size, first_index=rank * B).items()}      # resident in HBM

    def one_step(timings=None):
        out = inpaint(model, inp["image"], inp["mask"], inp["ref"], steps=a.plms_steps, scale=a.scale, x_T=inp["x_T"],
                      post_eps=inp["post_eps"], timings=timings)
        u8 = (out["image"] * 255.0).round().to(torch.uint8)
        return out, (gather_images(u8) if world > 1 else u8)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    with torch.no_grad():
        for _ in range(a.warmup):
            one_step()
        fence()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            last = one_step()
        torch.cuda.synchronize()
        own_elapsed = time.perf_counter() - t0                     # this rank's K steps, before it waits for the others
        fence()
        elapsed = time.perf_counter() - t0
        per_rank_ms = [1e3 * elapsed / a.steps]
        if world > 1:
            # every rank's own time for its K steps (before the closing barrier it would equal the slowest): a slow (power-capped) device
            # shows up as ONE large entry, a code-level scaling loss as all of them growing with N
            mine = torch.tensor([own_elapsed], device=device if backend == "nccl" else "cpu", dtype=torch.float64)
            allr = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allr, mine)
            per_rank_ms = [1e3 * float(x.item()) / a.steps for x in allr]
            t = torch.tensor([elapsed], device=device if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        if a.dump_outputs and rank == 0:                          # before the passes below reuse any buffer
            out, u8 = last
            info = dump_outputs(a.dump_outputs, {**out, "image_u8": u8})
            log(f"outputs of the last timed step -> {a.dump_outputs}: " + ", ".join(f"{k} {s} ({n} written)" for k, (s, n) in info.items()))
        del last

        # ---- --full: separate passes (outside the timed region): stage split and per-kernel-class events ----
        stage = None
        if "stage" in legs:
            stage = {}
            one_step(timings=stage)
        prof = None
        if "profile" in legs:
            ops.prof_reset()
            ops.prof_enable(True)
            one_step()
            torch.cuda.synchronize()
            ops.prof_enable(False)
            prof = ops.prof_collect()
            ops.prof_reset()

        # ---- BASELINE configs[2] geometry (batch 16 per GPU, same everything else): reported beside the headline, never as `value` ----
        b16 = None
        if "batch16" in legs:
            inp16 = {k: v.to(device) for k, v in cases.synthetic_triples(16, 512).items()}
            run16 = lambda: inpaint(model, inp16["image"], inp16["mask"], inp16["ref"], steps=a.plms_steps, scale=a.scale, x_T=inp16["x_T"],      # noqa: E731
                                    post_eps=inp16["post_eps"])
            run16()
            torch.cuda.synchronize()
            t16 = time.perf_counter()
            for _ in range(2):
                run16()
            torch.cuda.synchronize()
            t16 = (time.perf_counter() - t16) / 2
            b16 = {"per_gpu_batch": 16, "value": 16 / t16, "unit": "images/sec", "ms_per_step": 1e3 * t16, "steps": 2, "warmup": 1}
            del inp16

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    images = world * B * a.steps
    value = images / elapsed
    headline = a.image_size == 512 and a.precision == "fp16" and a.plms_steps == 50
    # algorithmic FLOP per image (FlopCounterMode on the reference modules): U-Net forward per sample 796.94 GF at
    # 64x64 latents, 2137.5 GF at 96x96; VAE encode + decode 3631.2 GF at 512x512 (x2.25 at 768x768); CLIP + mapper 155.6 GF
    unet_gf = 796.94 if a.image_size == 512 else 2137.5
    flop_per_image = ((a.plms_steps + 1) * 2 * unet_gf + 3631.2 * (1.0 if a.image_size == 512 else 2.25) + 155.6) * 1e9
    lat = a.image_size // 8
    if headline:
        workload = ("BASELINE configs[1]: batch=4/GPU, 512x512, 50 PLMS steps (51 U-Net calls at batch 8), scale=5, fp16 "
                    "activations + fp32 accumulate, name-seeded random-init U-Net + VAE + CLIP ViT-L/14 weights; the "
                    "context-independent prefix of each guidance pair (first ResBlock + first self-attention) is evaluated once")
    else:
        workload = (f"batch={B}/GPU, {a.image_size}x{a.image_size} ({lat}x{lat} latents), {a.plms_steps} PLMS steps ({a.plms_steps + 1} U-Net calls at batch "
                    f"{2 * B}), scale={a.scale:g}, " + ("e4m3 operands for the LayerNorm-fed projections (q|k, V^T, GEGLU) + fp16 elsewhere, fp32 accumulate"
                                                        if a.precision == "fp8" else "fp16 activations + fp32 accumulate")
                    + ", name-seeded random-init weights" + ("; BASELINE configs[4] geometry" if a.image_size == 768 else ""))
    line = {
        "metric": f"{a.image_size}x{a.image_size} images/sec @{a.plms_steps} PLMS steps scale={a.scale:g}", "value": value, "unit": "images/sec", "n_gpus": world,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "fp16" if a.precision == "fp16" else "fp8 (e4m3 linear operands) + fp16", "data": "synthetic",
        "config": {"workload": workload, "per_gpu_batch": B, "global_batch": world * B, "plms_steps": a.plms_steps, "cfg_scale": a.scale,
                   "parallelism": f"batch-sharded x{world}, no per-step collective"},
        **({"unet_ms_per_step_per_image": stage.get("sampler_ms", 0.0) / a.plms_steps / B, "stage_ms_per_batch": stage} if stage is not None else {}),
        # reference-FLOP normalisation: what the reference's modules would execute per image (FlopCounterMode) ...
        "e2e_mfma_frac": value / world * flop_per_image / (MFMA_PEAK_TFLOPS * 1e12),
    }
    if prof:
        # ... and the FLOP this implementation actually LAUNCHES per step (matrix-core classes of the profiled pass): less than the
        # reference count because attn2's dead q/k/softmax and the shared guidance prefix are not evaluated (bit-identical, tested)
        exe = sum(prof[k]["work"] for k in ("conv3x3_igemm", "gemm", "attention") if k in prof)
        line["executed_tflop_per_step"] = exe / 1e12
        line["e2e_mfma_frac_executed"] = exe / (elapsed / a.steps) / (MFMA_PEAK_TFLOPS * 1e12)
    if world > 1:
        line["per_rank_ms"] = {"min": min(per_rank_ms), "max": max(per_rank_ms), "all": [round(x, 2) for x in per_rank_ms]}
        line["startup"] = build_info
    if b16:
        line["batch16"] = b16
    if prof:
        MFMA = ("conv3x3_igemm", "gemm", "attention")
        tj, traffic_src = measured_traffic()
        classes = {}
        for k, v in prof.items():
            if not v["launches"]:
                continue
            mf = k in MFMA
            ach = v["work"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0              # TFLOP/s (matrix-core classes) or TB/s
            row = {"launches": v["launches"], "ms": round(v["ms"], 3), "avg_launch_us": 1e3 * v["ms"] / v["launches"], "achieved": ach,
                   "unit": "TFLOP/s" if mf else "TB/s", "peak": MFMA_PEAK_TFLOPS if mf else HBM_PEAK_TBS,
                   "frac": ach / (MFMA_PEAK_TFLOPS if mf else HBM_PEAK_TBS),
                   "algorithmic_bytes_per_launch": v["bytes"] / v["launches"],
                   # per launch the roofline that binds THAT launch: max(FLOP / MFMA peak, algorithmic bytes / HBM peak), summed over the class
                   "roofline_ms": round(v["roofline_ms"], 3), "frac_of_binding_roofline": v["roofline_ms"] / v["ms"] if v["ms"] > 0 else 0.0}
            if mf:
                row["gflop_per_launch"] = v["work"] / v["launches"] / 1e9
            t = (tj or {}).get("classes", {}).get(k)
            row["traffic"] = (t["traffic_B_per_pass"] / v["launches"] if "traffic_B_per_pass" in t else t["traffic_B_per_launch"]) if t else None
            classes[k] = row
        dom = max((k for k in classes if k in MFMA), key=lambda k: classes[k]["ms"])           # the class with the most GPU time
        d = classes[dom]
        names = {"conv3x3_igemm": "igemm_kernel<*,*,*,*,1|2,*> (3x3 conv: gather and halo-resident implicit GEMM)", "gemm": "igemm_kernel<*,*,*,*,0,*> + astat_regs_kernel<*,*> (Linear / 1x1 conv GEMM)",
                 "attention": "attn_kernel<*,*,*> (fused self-attention)"}
        line["roofline"] = {"bound": "mfma", "kernel": names[dom], "achieved": d["achieved"], "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                            "frac": d["frac"], "traffic": d["traffic"], "traffic_unit": "B per launch (L2-fabric side)", "traffic_source": traffic_src,
                            "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"], "launches": d["launches"],
                            "avg_launch_us": d["avg_launch_us"], "avg_gflop_per_launch": d["gflop_per_launch"],
                            "frac_of_binding_roofline": d["frac_of_binding_roofline"], "classes": classes}
        line["kernel_classes"] = {k: {"launches": v["launches"], "ms": v["ms"], "rate": v["achieved"], "rate_unit": v["unit"]} for k, v in classes.items()}
    if "cpu_baseline" in legs:
        try:
            line["cpu_baseline"] = cpu_baseline(cpu_sd, max(1, min(16, os.cpu_count() or 1)))     # a 1-GPU box owns a 16-core share of the host
        except Exception as e:                                              # noqa: BLE001
            line["cpu_baseline"] = {"value": None, "error": f"{type(e).__name__}: {e}"}
    print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
