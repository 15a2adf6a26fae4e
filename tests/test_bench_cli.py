"""CPU: bench.py's command line and its --dump-outputs writer (no device).

The timed path itself runs only on the GPU; here: a plain run is the lean one
(--full is off by default and gates everything but the headline figure), and
the dump writes float32 / float64 .npy within its byte budget, a larger array
as the same seeded sample every time.
"""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_is_the_default_and_full_is_an_option():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    b = bench.parse(["--full", "--dump-outputs", "d", "--no-cpu-baseline", "--no-fp32"])
    assert b.full is True and b.dump_outputs == "d" and b.no_cpu_baseline and b.no_fp32


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


def test_dump_writes_float_arrays_as_they_are(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"rgb": torch.rand(33, 3, generator=g), "loss": torch.rand(5, generator=g).double(),
              "half": torch.rand(7, generator=g).bfloat16(), "scalar": torch.tensor(2.5)}
    info = bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["half.npy", "loss.npy", "rgb.npy", "scalar.npy"]
    for name, t in arrays.items():
        a = np.load(tmp_path / "out" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert a.shape == tuple(t.shape) and info[name] == [list(t.shape), str(a.dtype), False]
        np.testing.assert_array_equal(a, t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).numpy())


def test_dump_samples_an_array_beyond_its_share_the_same_way_every_time(tmp_path):
    big = torch.arange(1000, dtype=torch.float32)
    small = torch.arange(10, dtype=torch.float32)
    # 800 bytes for two arrays: 400 each = 100 floats of `big`, `small` whole
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, budget=800)
        assert info["big"] == [[100], "float32", True] and info["small"] == [[10], "float32", False]
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)
    assert a.nbytes + np.load(tmp_path / "a" / "small.npy").nbytes <= 800
    # distinct elements of the array, in their order
    assert len(set(a.tolist())) == 100 and np.all(np.diff(a) > 0) and set(a.tolist()) <= set(big.tolist())
