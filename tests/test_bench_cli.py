"""bench.py's command line and its --dump-outputs writer (host only: nothing here touches a GPU)."""
import os

import numpy as np
import pytest

import bench


def test_steps_and_warmup_are_taken_as_given():
    assert (bench.parse_args([]).steps, bench.parse_args([]).warmup) == (1010, 201)
    for wl in sorted(bench.WORKLOADS):
        a = bench.parse_args(["--workload", wl, "--steps", "1010", "--warmup", "201"])
        assert (a.steps, a.warmup) == (1010, 201), wl
        assert bench.parse_args(["--workload", wl, "--steps", "7"]).steps == 7
    # the per-workload defaults apply only when neither flag is given
    assert (bench.parse_args(["--workload", "pines"]).steps, bench.parse_args(["--workload", "pines"]).warmup) == (202, 202)
    assert (bench.parse_args(["--workload", "4-mode"]).steps, bench.parse_args(["--workload", "4-mode"]).warmup) == (220, 22)
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"positions": rng.standard_normal((100, 8)).astype(np.float32), "logdensity": rng.standard_normal(100),
              "attempts": np.arange(100, dtype=np.int32), "params": rng.standard_normal(5000).astype(np.float32)}
    limit = 10_000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=limit)
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in arrays)
    assert {k: v.dtype for k, v in got.items()} == {"positions": np.float32, "logdensity": np.float64, "attempts": np.float64, "params": np.float32}
    assert sum(v.nbytes for v in got.values()) <= limit
    for k in ("positions", "logdensity", "attempts"):
        np.testing.assert_array_equal(got[k], arrays[k])
    # the largest array is sampled: a subset of its elements, in order, the same on every run
    p = got["params"]
    assert 0 < p.size < arrays["params"].size
    np.testing.assert_array_equal(p, np.load(str(tmp_path / "b" / "params.npy")))
    idx = [int(np.flatnonzero(arrays["params"] == v)[0]) for v in p]
    assert idx == sorted(idx)
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "c"), arrays, limit=100)
