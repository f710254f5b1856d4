"""igemm_kernel's prologue gets its launch-invariant values from the host (no division before the first fetch): not a bit of any output
may differ from what the build before that change wrote.

Every case of tests/prologue_cases.py is launched with its tile forced and compared, torch.equal, with tests/golden/prologue_parent.npz -
recorded on an MI355X by tools/record_prologue_golden.py with the parent build (SHA-256 of the whole output; every stride-th element raw, to
say what moved) - and, for the halo-resident convs, with gather tile 9 on the same operands.

  * halo tiles 10 - 14 on [2,8,8] 128->128 (whole images per tile), [1,16,16] 64->160, [1,32,32] 64+64 concat->160 (the source switches at a
    block boundary) and [1,64,64] 64->160, each tile where the planner's halo rule admits it; tile 10 also with the plain main loop
  * split-K 3 over 5 channel blocks (slices of 2, 2, 1 blocks).  Against the recording only: a halo tile slices channel blocks, the gather
    tile k-tiles (45 in slices of 15), so the fp32 slabs hold other partial sums - the parent build differs from tile 9 here as well
  * a row vector with 2 and with 4 samples per tile; the phase-form 16 -> 32 upsampling conv (a gather tile: recording only)
  * dense tiles 3, 6, 9, 17, 21 at M = 200, N = 168, K = 200 (ragged in all three, K % 64 != 0): plain; a second source from K1 = 96, inside
    a k-tile (K1 = 72 is not a launch: pbe_gemm_f16 takes K1 % 32 == 0, checked below); batch 2 with a padded batch stride; split-K 2, at
    K = 520 because a slice holds at least 4 k-tiles and K = 200 has 4 in all
  * extended-epilogue tiles 3, 6, 9, 17 with the LayerNorm fold in and row statistics out; the A-stationary tiles 19 / 20 on the one problem
    they take (K = 320 GEGLU projection with the fold)
"""
import os

import numpy as np
import pytest
import torch

import prologue_cases as pc

pytestmark = pytest.mark.gpu
SPECS = pc.specs()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "prologue_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_cases_cover_every_halo_tile_and_map():
    halo = [s for s in SPECS if s["kind"] == "conv" and s["id"].count("-") == 2]
    assert {s["tile"] for s in halo} == set(pc.HALO_TILES) and {s["shape"] for s in halo} == set(pc.HALO_MAPS)
    assert len(halo) == 18 and len({s["id"] for s in SPECS}) == len(SPECS)


@pytest.mark.parametrize("spec", SPECS, ids=[s["id"] for s in SPECS])
def test_bits_of_the_parent_build(dev, golden, spec):
    with torch.no_grad():
        outs = pc.run(spec, dev)
        for j, t in enumerate(outs):
            sha, sub = pc.digest(t)
            want_sub = golden[f"{spec['id']}/{j}/sub"]
            assert sub.dtype == want_sub.dtype and sub.shape == want_sub.shape
            moved = int((sub.view(np.uint8) != want_sub.view(np.uint8)).reshape(sub.size, -1).any(1).sum())
            assert moved == 0, f"{spec['id']} output {j}: {moved} of {sub.size} sampled elements differ from the parent build"
            assert np.array_equal(sha, golden[f"{spec['id']}/{j}/sha"]), f"{spec['id']} output {j}: differs from the parent build outside the sampled elements"
        if spec["kind"] == "conv" and spec.get("splits", 1) == 1:
            y9 = pc.run(spec, dev, tile=9)[0]
            assert torch.equal(outs[0], y9), f"{spec['id']}: halo tile and gather tile 9 differ in {int((outs[0] != y9).sum())} elements"


def test_second_source_must_start_on_a_32_column_boundary(dev):
    from pbe_amd import lib, ops
    a, a2 = torch.zeros(pc.GM, 72, dtype=torch.float16, device=dev), torch.zeros(pc.GM, pc.GK - 72, dtype=torch.float16, device=dev)
    with pytest.raises(lib.PbeError, match="K1"):
        ops.gemm(a, torch.zeros(pc.GN, pc.GK, dtype=torch.float16, device=dev), None, a2=a2)
