"""Noise from per-sample seeds, host side (-m "not gpu"): the numpy restatement tests/noiseref.py against the three Random123 known
answers and against the statistics a normal draw must have, the declared symbols, and the stream plan and seed validation of
pbe_amd.noise / pbe_amd.ops with the kernel call replaced - in these tests only - by a recorder.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

import noiseref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pbe_philox_u32", "pbe_randn_philox_f32")


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", nr.KAT, ids=["zeros", "ones", "pi"])
def test_random123_known_answers(counter, key, want):
    got = nr.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(x) for x in got] == list(want), [hex(int(x)) for x in got]


def test_words_are_the_counters_in_order():
    w = nr.words(seed=(0x299f31d0 << 32) | 0xa4093822, sub=0x85a308d3, stream=(0x03707344 << 32) | 0x13198a2e, n=4 * 0x10 + 3)
    assert w.dtype == np.uint32 and w.shape == (67,)
    q = 5                                                                        # any counter: key / sub / stream as in the third KAT
    one = nr.philox4x32_10(np.array([q, 0x85a308d3, 0x13198a2e, 0x03707344], dtype=np.uint64), np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
    assert np.array_equal(w[4 * q:4 * q + 4], one)
    assert np.array_equal(nr.words(3, 1, 2, 5), nr.words(3, 1, 2, 64)[:5])       # a prefix whatever n


def test_uniform_ranges_and_the_zero_radius():
    u, v = nr.uniforms(42, 0, 0, 1 << 16)
    assert u.min() > 0.0 and u.max() <= 1.0 and v.min() >= 0.0 and v.max() < 1.0
    assert np.all(u * 2.0 ** 24 == np.round(u * 2.0 ** 24)) and np.all(v * 2.0 ** 24 == np.round(v * 2.0 ** 24))
    assert np.float32(2.0 ** -24 * (2 ** 24)) == 1.0 and np.sqrt(-2.0 * np.log(1.0)) == 0.0      # u = 1: r = 0, both elements zero
    assert np.sqrt(-2.0 * np.log(2.0 ** -24)) < 5.77
    for seed, sub, stream, elems in nr.ZERO_RADIUS:
        u1, _ = nr.uniforms(seed, sub, stream, 4)
        assert u1[elems[0] // 2] == 1.0 and np.all(nr.randn64(seed, sub, stream, 4)[list(elems)] == 0.0)


def test_reference_statistics():
    worst = nr.check_stats(lambda seed, stream, n: nr.randn64(seed, 0, stream, n))
    assert worst["mean"] <= 0.0099 + 1e-4 and worst["std"] <= 0.0098 + 1e-4 and worst["corr"] <= 0.018 + 1e-3     # what the reference alone gives


def test_case_table_covers_every_value():
    ns = {c[0] for c in nr.CASES}
    assert ns == set(nr.N_VALUES) and {len(c[1]) for c in nr.CASES} == {1, 3}
    for n in nr.N_VALUES:
        assert {len(c[1]) for c in nr.CASES if c[0] == n} == {1, 3}
    assert {s for c in nr.CASES for s in c[1]} == set(nr.SEEDS)
    subs = {None if c[2] is None else "given" for c in nr.CASES} | {s for c in nr.CASES if c[2] is not None for s in c[2]}
    assert {None, 0, 1, (1 << 31) - 1} <= subs
    assert {c[3] for c in nr.CASES} == set(nr.STREAMS)
    assert sum(c[0] * len(c[1]) for c in nr.CASES) < 1 << 17                     # seconds, not minutes


# ---- 2. the contract -------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_documents():
    from pbe_amd import lib
    assert lib.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "pbe_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in lib.SYMBOLS, name
        assert f"int {name}(" in header, name
        assert f"`{name}(" in integration, name
    assert "noise.hip" in lib.SOURCES and os.path.join("csrc", "noise.hip") in lib.HASHED
    assert os.path.exists(os.path.join(ROOT, "pbe_amd", "csrc", "noise.hip"))
    res, args = lib.SYMBOLS["pbe_randn_philox_f32"]
    assert res is lib.c_i32 and len(args) == 9 and args[5] is lib.C.c_uint64 and args[6] is lib.c_f32 and args[7] is lib.c_f32
    assert len(lib.SYMBOLS["pbe_philox_u32"][1]) == 7


def test_stream_constants_match_the_reference():
    from pbe_amd import noise
    assert (noise.STREAM_X_T, noise.STREAM_POST_EPS, noise.STREAM_STEP0) == (0, 1, 16) == (nr.STREAM_X_T, nr.STREAM_POST_EPS, nr.STREAM_STEP0)
    for word in ("STREAM_X_T", "STREAM_POST_EPS", "STREAM_STEP0", "Philox4x32-10", "sub"):
        assert word in noise.__doc__                                             # the plan is part of the public contract


# ---- 3. the stream plan, with the launch recorded instead of made ---------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    from pbe_amd import ops
    calls = []

    def fake_randn_seeded(seeds, shape, stream, sub=None, out=None, a=0.0, b=1.0):
        calls.append({"seeds": seeds, "shape": tuple(shape), "stream": stream, "sub": sub, "out": out, "a": a, "b": b})
        return out if out is not None else torch.zeros(tuple(shape))
    monkeypatch.setattr(ops, "randn_seeded", fake_randn_seeded)
    monkeypatch.setattr(ops, "seed_tensor", lambda seeds, B, device=None: torch.tensor(ops.seed_words(seeds), dtype=torch.int64))
    monkeypatch.setattr(ops, "sub_tensor", lambda sub, B, device: None if sub is None else torch.tensor(list(sub), dtype=torch.int32))
    return calls


def test_stream_plan(recorded):
    from pbe_amd.noise import SeededNoise
    sn = SeededNoise([5, 9], sub=[0, 7])
    sn.x_T((2, 4, 8, 8))
    sn.post_eps((2, 4, 8, 8))
    for _ in range(3):
        sn.noise_like((2, 4, 8, 8), "cpu")
    img = torch.ones((2, 4, 8, 8))
    assert sn.add_noise_(img, 0.25) is img
    sn.noise_like((2, 4, 8, 8))
    assert [c["stream"] for c in recorded] == [0, 1, 16, 17, 18, 19, 20]
    assert all(c["seeds"].tolist() == [5, 9] and c["sub"].tolist() == [0, 7] for c in recorded)
    assert (recorded[5]["a"], recorded[5]["b"], recorded[5]["out"] is img) == (1.0, 0.25, True)
    assert all((c["a"], c["b"], c["out"]) == (0.0, 1.0, None) for i, c in enumerate(recorded) if i != 5)
    other = SeededNoise([5, 9])                                                  # the counter belongs to the object
    other.noise_like((2, 1))
    assert recorded[-1]["stream"] == 16 and recorded[-1]["sub"] is None
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError):
        sn.x_T((3, 4, 8, 8))                                                     # one sample per seed


def test_seed_words_twos_complement():
    from pbe_amd import ops
    assert ops.seed_words([0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 5, (1 << 64) - 1]) == [0, 1, (1 << 63) - 1, -(1 << 63), -(1 << 63) + 5, -1]
    assert [nr.as_i64(s) for s in nr.SEEDS] == ops.seed_words(nr.SEEDS)


@pytest.mark.parametrize("bad", [[-1], [1 << 64], [1.0], [0.5, 2], 3, "12", [True], torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float32),
                                 torch.zeros(2, dtype=torch.int64)], ids=["negative", "2^64", "float", "floats", "scalar", "str", "bool", "int32", "float32", "cpu-int64"])
def test_seed_validation(bad):
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    from pbe_amd.noise import SeededNoise
    with pytest.raises(PbeError):
        SeededNoise(bad)
    with pytest.raises(PbeError):
        ops.randn_seeded(bad, (2, 4), 0)
    with pytest.raises(PbeError):
        ops.philox_u32(bad, 4)


def test_sampler_and_pipeline_signatures():
    import inspect
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    from pbe_amd import pipeline
    for cls in (PLMSSampler, DDIMSampler, DPMSolverSampler):
        p = inspect.signature(cls.sample).parameters
        assert p["seeds"].default is None and p["seed_sub"].default is None, cls.__name__
    p = inspect.signature(pipeline.inpaint).parameters
    assert p["seeds"].default is None and p["seed_sub"].default is None
    assert {"seeds", "seed_sub"} <= set(pipeline.PER_WINDOW_KWARGS)
