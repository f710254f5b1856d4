#!/usr/bin/env python3
"""Record tests/golden/prologue_parent.npz: the outputs of the launches of tests/prologue_cases.py, as the library that is loaded computes
them.  Run ONCE on the GPU with the build of the commit BEFORE a change that must not move a bit (PBE_LIB_PATH names that library), then
commit the file; tests/test_prologue_gpu.py compares every later build against it.

    PBE_LIB_PATH=<parent build>/pbe_amd/libpbe_hip.so python tools/record_prologue_golden.py [out.npz]

Per output j of case <id>: "<id>/<j>/sha" (SHA-256 of all bytes) and "<id>/<j>/sub" (every stride-th element, raw: fp16 stays fp16).
Also prints, per halo case, whether the halo tile's bits equal gather tile 9's at the same split-K factor.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import prologue_cases as pc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "prologue_parent.npz")
    dev = torch.device("cuda:0")
    arrays = {}
    with torch.no_grad():
        for spec in pc.specs():
            outs = pc.run(spec, dev)
            for j, t in enumerate(outs):
                sha, sub = pc.digest(t)
                arrays[f"{spec['id']}/{j}/sha"], arrays[f"{spec['id']}/{j}/sub"] = sha, sub
            note = ""
            if spec["kind"] == "conv":
                y9 = pc.run(spec, dev, tile=9)[0]
                note = f"  equals gather tile 9: {bool(torch.equal(outs[0], y9))}"
            print(f"{spec['id']:44s} {[tuple(t.shape) for t in outs]}{note}", flush=True)
    np.savez_compressed(out, **arrays)
    print(f"{len(arrays) // 2} outputs -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
