"""Quantised golden of the full-size U-Net forward - runs on any CPU-only machine, from this repository's own code alone.

    python oracle/gen_q8_golden.py            # writes tests/golden/full_q8.npz (about a CPU-minute; the weights take 3.5 GB)

oracle/pbe_oracle.py's unet_forward (fp32) on tests/cases.py's full_inputs() and the name-seeded weights (pbe_amd/weights.py; names and
shapes from tests/golden/v1_keys.txt), with its transformer_block replaced by tests/q8ref.py's block64: the BasicTransformerBlock in exact
fp64 arithmetic with only the operand quantisations of a mode ("linear": pbe_amd.precision.set_linear_precision(model, "fp8"),
"attention": set_attention_precision(model, "fp8"), "both").  The N = 4096 self-attention runs one (sample, head) at a time.

Before anything is written the same recipe with NO quantisation (block64 in plain fp64) must reproduce tests/golden/full.npz's unet_y
(the reference's own output) within 1e-5 rel-L2: that pins the wiring of the replacement.  tests/test_q8gate_gpu.py reads the file.
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


O = _load(os.path.join(HERE, "pbe_oracle.py"), "pbe_oracle")
W = _load(os.path.join(REPO, "pbe_amd", "weights.py"), "pbe_weights")
import cases as CASES  # noqa: E402
import q8ref as Q  # noqa: E402

UP = "model.diffusion_model."
PIN_TOL = 1e-5
torch.set_grad_enabled(False)


def unet_state_dict():
    sd = {}
    with open(os.path.join(OUT, "v1_keys.txt")) as f:
        for line in f:
            name, shape = line.split()
            if name.startswith(UP):
                sd[name] = W.synth_tensor(name, tuple(int(s) for s in shape.split("x")))
    return sd


def forward(sd, inp, mode):
    """unet_forward with every transformer block in fp64 (mode None: plain; else the operand quantisations of the mode)."""
    saved = O.transformer_block
    O.transformer_block = lambda sd_, p, x, context, heads: Q.block64(sd_, p, x.double(), context, heads, mode).float()
    try:
        return O.unet_forward(sd, inp["unet_x"], inp["unet_t"], inp["unet_ctx"], O.UNET_V1, UP)
    finally:
        O.transformer_block = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(OUT, "full_q8.npz"))
    args = ap.parse_args()
    inp = CASES.full_inputs()
    sd = unet_state_dict()
    gold = np.load(os.path.join(OUT, "full.npz"))["unet_y"]
    t0 = time.time()
    pin = Q.rel_l2(forward(sd, inp, None), torch.from_numpy(gold).double())
    print(f"plain fp64 blocks vs tests/golden/full.npz: rel-L2 {pin:.2e} (limit {PIN_TOL:.0e}), {time.time() - t0:.0f}s", flush=True)
    assert pin <= PIN_TOL, pin
    out = {"plain_pin_rel_l2": np.float64(pin)}
    for mode in Q.MODES:
        t0 = time.time()
        y = forward(sd, inp, mode)
        r = Q.rel_l2(y, torch.from_numpy(gold).double())
        print(f"{mode:10s} q64 vs the plain golden: rel-L2 {r:.3e}, {time.time() - t0:.0f}s", flush=True)
        out["unet_y_" + mode] = y.float().numpy()
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
