#!/usr/bin/env python3
"""Record tests/golden/block_parent.npz: what the cases of tests/block_cases.py compute and launch, with the ldm/ package and the library
that are loaded.  Run ONCE on the GPU with the tree of the commit BEFORE a change that must move neither a bit nor a launch of
BasicTransformerBlock, then commit the file; tests/test_block_paths_gpu.py compares every later tree against it.

    python tools/record_block_golden.py [out.npz]

Per run w ("run" = st.run(cat([x, x]), vecs), "paired" = st.run_paired(x, vecs)) of case <id>: "<id>/<w>/<j>/sha" and "<id>/<w>/<j>/sub"
(output j: SHA-256 of all bytes, every stride-th element raw), "<id>/<w>/launches" (JSON as bytes: the ordered GEMM plans and the launch
count per kernel class), and "<id>/equal" (1: the two runs' outputs were equal).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import block_cases as bc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "block_parent.npz")
    dev = torch.device("cuda:0")
    arrays = {}
    with torch.no_grad():
        st = bc.transformer(dev)
        for spec in bc.specs():
            res = bc.run(spec, st, dev)
            for which, r in res.items():
                for j, t in enumerate(r["out"]):
                    arrays[f"{spec['id']}/{which}/{j}/sha"], arrays[f"{spec['id']}/{which}/{j}/sub"] = bc.digest(t)
                arrays[f"{spec['id']}/{which}/launches"] = bc.as_array(bc.launch_record(r))
            equal = all(torch.equal(a, b) for a, b in zip(res["run"]["out"], res["paired"]["out"]))
            arrays[f"{spec['id']}/equal"] = np.array([int(equal)], dtype=np.uint8)
            y = res["run"]["out"][0].float()
            print(f"{spec['id']:24s} launches run {sum(res['run']['counts'].values()):3d} paired {sum(res['paired']['counts'].values()):3d}  "
                  f"GEMM plans {len(res['run']['plans']):2d} / {len(res['paired']['plans']):2d}  paired == run: {equal}  "
                  f"finite {bool(torch.isfinite(y).all())}  rms {float(y.pow(2).mean().sqrt()):.3f}", flush=True)
    np.savez_compressed(out, **arrays)
    print(f"{len(bc.specs())} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
