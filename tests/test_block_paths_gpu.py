"""BasicTransformerBlock runs every path - one-token or multi-token context, LayerNorm folded / separate / fp8, alone or as a guidance
pair - through one chain of stages (attn1, attn2, ff).  Neither a bit of any output nor a launch may differ from what the tree with the
paths written out one by one computed.

Every case of tests/block_cases.py runs on the seeded two-block SpatialTransformer(320, 8, 40) at B = 2, as st.run(cat([x, x]), vecs) and
as st.run_paired(x, vecs), and is compared with tests/golden/block_parent.npz - recorded on an MI355X by tools/record_block_golden.py with
the parent tree:

  * the output (and, with a ContextMaps, the collector's accumulator): SHA-256 of all bytes, every stride-th element raw to say what moved
  * the ordered GEMM launches (key, tile, split-K, BM, BN, workgroups) and the launch count of every kernel class: the same kernels in the
    same order on the same tiles, not merely the same bits
  * run_paired equals run, torch.equal, wherever the recording says the parent's did

  one-token context: default switches at 8 x 8 (folded) and 5 x 5 (plain: N % 8 != 0, V^T padded to 32); fold_layernorm off; linear_fp8 at
  both grids; attn_fp8 with the MX copy-out and with the quantiser; linear_fp8 with attn_fp8
  4 tokens: the fused kernel without weights and with one weight 0, at 8 x 8 and at 5 x 5 (statistics computed by the block);
  ctx_fused_max_width = 64 (the ContextKV route) with weights, folded and plain; region maps [4, 4, 8, 8]; a ContextMaps bound to B = 2
  (the conditional half of the pair: the per-range launches of attn2)
"""
import json
import os

import numpy as np
import pytest
import torch

import block_cases as bc

pytestmark = pytest.mark.gpu
SPECS = bc.specs()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "block_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def st(dev):
    with torch.no_grad():
        return bc.transformer(dev)


def test_cases_are_the_recorded_ones(golden):
    assert len({s["id"] for s in SPECS}) == len(SPECS) == 16
    assert {k.split("/")[0] for k in golden} == {s["id"] for s in SPECS}


@pytest.mark.parametrize("spec", SPECS, ids=[s["id"] for s in SPECS])
def test_bits_and_launches_of_the_parent_tree(dev, golden, st, spec):
    with torch.no_grad():
        res = bc.run(spec, st, dev)
    for which, r in res.items():
        tag = f"{spec['id']} {which}"
        for j, t in enumerate(r["out"]):
            sha, sub = bc.digest(t)
            want_sub = golden[f"{spec['id']}/{which}/{j}/sub"]
            assert sub.dtype == want_sub.dtype and sub.shape == want_sub.shape
            moved = int((sub.view(np.uint8) != want_sub.view(np.uint8)).reshape(sub.size, -1).any(1).sum())
            assert moved == 0, f"{tag} output {j}: {moved} of {sub.size} sampled elements differ from the parent tree"
            assert np.array_equal(sha, golden[f"{spec['id']}/{which}/{j}/sha"]), f"{tag} output {j}: differs from the parent tree outside the sampled elements"
        want = json.loads(golden[f"{spec['id']}/{which}/launches"].tobytes().decode())
        got = json.loads(bc.launch_record(r))
        assert got["plans"] == want["plans"], f"{tag}: GEMM launches differ from the parent tree\n got {got['plans']}\nwant {want['plans']}"
        assert got["counts"] == want["counts"], f"{tag}: launches per kernel class differ from the parent tree: got {got['counts']}, want {want['counts']}"
    if int(golden[f"{spec['id']}/equal"][0]):
        for a, b in zip(res["run"]["out"], res["paired"]["out"]):
            assert torch.equal(a, b), f"{spec['id']}: run_paired differs from run in {int((a != b).sum())} of {a.numel()} elements"


def test_multi_token_context_is_refused_with_linear_fp8(dev, st):
    from pbe_amd.lib import PbeError
    spec = next(s for s in SPECS if s["id"] == "k4-fused-8x8")
    with torch.no_grad():
        bc.set_switches(st, {})
        x, ctx, _, _ = bc.inputs(spec, dev)
        vecs = st.context_vectors(ctx)
        bc.set_switches(st, dict(linear_fp8=True))
        try:
            with pytest.raises(PbeError, match="multi-token context is not available with linear_fp8"):
                st.run(torch.cat([x, x], 0), vecs)
            with pytest.raises(PbeError, match="multi-token context is not available with linear_fp8"):
                st.run_paired(x, vecs)
            with pytest.raises(PbeError, match="multi-token context is not available with linear_fp8"):
                st.context_vectors(ctx)
        finally:
            bc.set_switches(st, {})
