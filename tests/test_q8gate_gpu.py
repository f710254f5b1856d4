"""The fp8 block paths (pbe_amd.precision: linear_fp8, attn_fp8) against a quantisation-aware fp64 reference (tests/q8ref.py).

a. Blocks: the seeded SpatialTransformer of tests/block_cases.py through st.run and st.run_paired on three grids, six switch settings,
   each output through q8ref.verdict: within REL_L2_FACTOR of the fp32 emulation's distance to the fp64 chain that makes the same
   quantisation decisions (q64), nearer to the plain fp64 block than 1.5 x the quantisation error itself, fp16 cases within BLOCK_TOL.
b. One full-size forward per fp8 mode against tests/golden/full_q8.npz (oracle/gen_q8_golden.py: the oracle's U-Net with q64 blocks).
c. The headline 50-step trajectory per fp8 mode against tests/golden/full_plms50.npz, twice, equal bits.

The printed lines (pytest -s) are the GPU half of profiles/q8gate_report.txt; PBE_Q8_REPORT=<file> appends them there.
"""
import os

import numpy as np
import pytest
import torch

import block_cases as bc
import cases
import modelbuild as build
import q8ref as Q

pytestmark = pytest.mark.gpu

# b. rel-L2 of the MI355X forward against the q64 golden, measured (profiles/q8gate_report.txt); the limit is 3 x the measurement (DESIGN.md
#    section 2, as MAP_ORACLE_TOL).  For scale: q64 against the plain golden is 3.370e-2 / 2.379e-3 / 3.375e-2.
Q8_FWD_MEASURED = {"linear": 1.398e-2, "attention": 1.909e-3, "both": 1.528e-2}
# c. rel-L2 against tests/golden/full_plms50.npz after steps 0 / 3 / 25 / 49 and on the final latent, measured per mode; each limit is 3 x
#    its measurement.  The fp16 path's own: 4.0e-4, 9.3e-4, 8.5e-4, 8.6e-4 (final) - TRAJ50_TOL, tests/test_model_gpu.py.
Q8_TRAJ_MEASURED = {
    "linear": (9.894e-3, 2.408e-2, 2.728e-2, 2.730e-2, 2.730e-2),
    "attention": (6.554e-4, 1.535e-3, 1.183e-3, 1.185e-3, 1.185e-3),
    "both": (9.909e-3, 2.406e-2, 2.727e-2, 2.729e-2, 2.729e-2),
}


def report(line):
    print(line)
    path = os.environ.get("PBE_Q8_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- a. blocks ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def st(dev):
    with torch.no_grad():
        return bc.transformer(dev)


def _both_runs(st, dev, grid, sw):
    """(st.run on cat([x, x]), st.run_paired on x) of a grid's inputs under the switches sw; the defaults are back afterwards."""
    x, ctx, _, _ = bc.inputs(Q.case_spec(grid), dev)
    try:
        bc.set_switches(st, sw)
        with torch.no_grad():
            vecs = st.context_vectors(ctx)
            return st.run(torch.cat([x, x], 0), vecs).cpu(), st.run_paired(x, vecs).cpu()
    finally:
        bc.set_switches(st, {})


@pytest.mark.parametrize("grid", Q.GRIDS)
@pytest.mark.parametrize("name,sw,mode", Q.CASES, ids=[c[0] for c in Q.CASES])
def test_block_case_against_q64(dev, st, grid, name, sw, mode):
    r = Q.refs(grid)
    path = Q.path_of(mode, grid * grid, sw.get("fold_layernorm", True))
    try:                                                             # the emulation restates the chain the block really takes
        bc.set_switches(st, sw)
        assert all(blk._mode(grid * grid) == path for blk in st.transformer_blocks)
        if mode in ("attention", "both"):
            assert all(blk.attn1._mx8_out(grid * grid) == (sw.get("mx8_from_projection", True) and grid != 5) for blk in st.transformer_blocks)
    finally:
        bc.set_switches(st, {})
    for which, y in zip(("run", "run_paired"), _both_runs(st, dev, grid, sw)):
        ok, text = r.verdict(y, mode, path)
        report(f"q8gate gpu  {name + f'-{grid}x{grid}':22s} {path:6s} {which:10s}: {text}")
        assert ok, (name, grid, which, text)


@pytest.mark.parametrize("grid", Q.GRIDS)
def test_attn_fp8_routes_agree_bit_for_bit(dev, st, grid):
    """pbe_amd/precision.py: the MX copy-out writes the bytes of the quantiser path, so both routes produce the same output (at N = 25
    both take the quantiser)."""
    a = _both_runs(st, dev, grid, dict(attn_fp8=True, mx8_from_projection=True))
    b = _both_runs(st, dev, grid, dict(attn_fp8=True, mx8_from_projection=False))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if grid != 5:                                                    # with linear_fp8 the two fp8-operand projections copy out as well
        a = _both_runs(st, dev, grid, dict(linear_fp8=True, attn_fp8=True, mx8_from_projection=True))
        b = _both_runs(st, dev, grid, dict(linear_fp8=True, attn_fp8=True, mx8_from_projection=False))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- b, c: the full-size model ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(dev):
    with torch.no_grad():
        return build.full_model(dev, parts=("unet",))


class _precision:
    def __init__(self, model, mode):
        self.model, self.mode = model, mode

    def __enter__(self):
        from pbe_amd.precision import set_attention_precision, set_linear_precision
        assert set_linear_precision(self.model, "fp8" if self.mode in ("linear", "both") else "fp16") == 16
        assert set_attention_precision(self.model, "fp8" if self.mode in ("attention", "both") else "fp16") == 16

    def __exit__(self, *exc):
        from pbe_amd.precision import set_attention_precision, set_linear_precision
        set_linear_precision(self.model, "fp16")
        set_attention_precision(self.model, "fp16")


def _rel(got, ref):
    got, ref = got.detach().float().cpu().double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return ((got - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("mode", Q.MODES)
def test_full_forward_against_the_quantised_golden(dev, golden_dir, full, mode):
    q8 = np.load(os.path.join(golden_dir, "full_q8.npz"))["unet_y_" + mode]
    plain = np.load(os.path.join(golden_dir, "full.npz"))["unet_y"]
    inp = cases.full_inputs()
    with torch.no_grad(), _precision(full, mode):
        y = full.apply_model(inp["unet_x"].to(dev), inp["unet_t"].to(dev), inp["unet_ctx"].to(dev))
    r, quant = _rel(y, q8), _rel(torch.from_numpy(q8), plain)
    tol = 3 * Q8_FWD_MEASURED[mode]
    report(f"q8gate gpu  v1 U-Net forward, {mode:9s} fp8: vs the q64 golden {r:.3e} (limit {tol:.2e} = 3 x measured); q64 vs the plain golden {quant:.3e}; "
           f"vs the plain golden {_rel(y, plain):.3e}")
    assert r <= tol, (mode, r, tol)
    assert r < quant, (mode, r, quant)                               # nearer to the quantised reference than the quantisation error is large


def _trajectory(full, dev, inp):
    from ldm.models.diffusion.plms import PLMSSampler
    z0, inter = PLMSSampler(full).sample(S=inp["steps"], batch_size=1, shape=[4, 64, 64], conditioning=inp["c"].to(dev), verbose=False,
                                         unconditional_guidance_scale=inp["scale"], unconditional_conditioning=inp["uc"].to(dev), eta=0.0,
                                         x_T=inp["x_T"].to(dev), log_every_t=1,
                                         test_model_kwargs={"images_inpaint": inp["z_inpaint"].to(dev), "images_mask": inp["mask_lat"].to(dev)})
    assert len(inter["x_inter"]) == inp["steps"] + 1
    return [inter["x_inter"][i + 1].clone() for i in cases.FULL_PLMS50_RECORD] + [z0.clone()]


@pytest.mark.parametrize("mode", Q.MODES)
def test_plms50_trajectory_under_fp8(dev, golden_dir, full, mode):
    """The call of test_full_plms50_headline_trajectory_against_reference under each fp8 mode: 51 U-Net calls on a guidance pair, against
    the reference's trajectory; twice, equal bits.  No bound can be derived for 50 chained guided steps: each limit is 3 x its
    measurement (Q8_TRAJ_MEASURED)."""
    g = np.load(os.path.join(golden_dir, "full_plms50.npz"))
    inp = cases.full_plms50_inputs()
    with torch.no_grad(), _precision(full, mode):
        a = _trajectory(full, dev, inp)
        b = _trajectory(full, dev, inp)
    names = [f"x after step {i}" for i in cases.FULL_PLMS50_RECORD] + ["final latent"]
    want = [g[f"plms_x_{i}"] for i in cases.FULL_PLMS50_RECORD] + [g["plms_latent"]]
    got = [_rel(t, w) for t, w in zip(a, want)]
    report(f"q8gate gpu  v1-size PLMS-50, {mode:9s} fp8 vs the reference trajectory: " + ", ".join(f"{n} {v:.3e}" for n, v in zip(names, got))
           + "; limits 3 x " + ", ".join(f"{m:.2e}" for m in Q8_TRAJ_MEASURED[mode]))
    for n, v, m in zip(names, got, Q8_TRAJ_MEASURED[mode]):
        assert v <= 3 * m, (mode, n, v, 3 * m)
    assert all(torch.equal(x, y) for x, y in zip(a, b))              # run to run bit-identical
