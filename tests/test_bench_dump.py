"""CPU suite (-m "not gpu"): bench.py's --dump-outputs writer, its --steps check and which legs beyond the timed steps a run makes,
without a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("pbe_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_small_arrays_whole(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    arrays = {"image": torch.rand(2, 3, 16, 16, generator=g), "latent": torch.randn(2, 4, 4, 4, generator=g).half(),
              "image_u8": (torch.rand(2, 3, 16, 16, generator=g) * 255).round().to(torch.uint8)}
    info = bench.dump_outputs(str(tmp_path), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(v.shape) and info[k] == (list(v.shape), v.numel())
        np.testing.assert_array_equal(got, v.float().numpy())


def test_dump_outputs_large_array_seeded_sample(tmp_path):
    bench = _bench()
    big = torch.arange(20_000_000, dtype=torch.float32)            # 80 MB: over the cap on its own
    small = torch.linspace(-1, 1, 1000)
    runs = []
    for d in ("a", "b"):
        out = tmp_path / d
        info = bench.dump_outputs(str(out), {"big": big, "small": small})
        assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000
        np.testing.assert_array_equal(np.load(out / "small.npy"), small.numpy())        # small arrays stay whole
        got = np.load(out / "big.npy")
        assert got.dtype == np.float32 and got.ndim == 1 and info["big"] == ([20_000_000], got.size) and got.size > 10_000_000
        assert np.all(np.diff(got) >= 0)                              # sorted flat indices (arange: values follow the indices)
        runs.append(got)
    np.testing.assert_array_equal(runs[0], runs[1])                   # the same sample on every run


def test_steps_must_be_positive():
    bench = _bench()
    assert bench.parse_args(["--steps", "5", "--warmup", "0"]).steps == 5
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_plain_run_makes_no_extra_legs():
    bench = _bench()
    for argv in ([], ["--steps", "20", "--warmup", "5"], ["--image-size", "768", "--precision", "fp8"], ["--batch", "16"]):
        a = bench.parse_args(["--gpus", "1", *argv])
        assert not a.full and bench.extra_legs(a, 1, 0) == set()
    a = bench.parse_args(["--gpus", "2"])
    assert bench.extra_legs(a, 2, 0) == set() and bench.extra_legs(a, 2, 1) == set()


def test_full_run_legs():
    bench = _bench()
    legs = lambda argv, world=1, rank=0: bench.extra_legs(bench.parse_args(["--full", *argv]), world, rank)      # noqa: E731
    assert legs([]) == {"stage", "profile", "batch16", "cpu_baseline"}
    assert legs(["--no-profile", "--no-batch16", "--no-cpu-baseline"]) == {"stage"}
    assert legs(["--no-profile"]) == {"stage", "batch16", "cpu_baseline"}
    assert legs(["--batch", "16"]) == {"stage", "profile", "cpu_baseline"}           # the headline already is batch 16
    for off_headline in (["--image-size", "768"], ["--precision", "fp8"], ["--plms-steps", "100"]):
        assert legs(off_headline) == {"stage", "profile"}
    for rank in (0, 1):                                                                  # every rank runs the passes that gather
        assert legs(["--gpus", "2"], world=2, rank=rank) == {"stage", "profile"}
