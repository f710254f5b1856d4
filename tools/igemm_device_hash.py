"""sha256 of the gfx950 device code of every igemm translation unit: the identity check for refactors of the igemm kernel
("Refactoring the igemm kernel").

    python tools/igemm_device_hash.py <csrc dir> <defines, comma separated, or -> <output file>

Each TU is compiled with build.py's own FLAGS / EXTRA plus -cuid=pbe --offload-device-only -c (the fixed cuid makes the output
byte-reproducible: without it the static zero block of a TU gets a random suffix) and the output file gets one line per TU,
"<sha256>  <tu>  <defines>".  Run it on the csrc directory of two trees (a `git worktree` of the parent and the head) and compare the
files: a line that differs means the device code changed.  It only hashes.
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_pbe_build", os.path.join(ROOT, "pbe_amd", "build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)

TUS = ["igemm_dense", "igemm_conv", "igemm_halo", "igemm_f8", "igemm_ex", "igemm_ex_ln", "igemm_ex_st", "igemm_ex_qkv", "igemm_ex_all", "igemm_astat"]


def device_hash(csrc: str, tu: str, defines, tmp: str) -> str:
    src, out = tu + ".hip", os.path.join(tmp, tu + ".out")
    cmd = [_build._hipcc(), *_build.FLAGS, *_build.EXTRA.get(src, []), *[f"-D{d}" for d in defines], "-cuid=pbe", "--offload-device-only", "-c",
           os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    with open(out, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main(argv) -> int:
    if len(argv) != 4:
        print(__doc__)
        return 2
    csrc, defines, out_path = os.path.abspath(argv[1]), [d for d in argv[2].split(",") if d and d != "-"], argv[3]
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        hashes = list(ex.map(lambda tu: device_hash(csrc, tu, defines, tmp), TUS))
    with open(out_path, "w") as f:
        for tu, h in zip(TUS, hashes):
            f.write(f"{h}  {tu}  {','.join(defines) or '-'}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
