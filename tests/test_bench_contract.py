"""Driver-contract tests for bench.py.

The round-end driver may invoke `python bench.py --gpus N` DIRECTLY
(BENCH_r01.json `cmd`), without torchrun.  bench.py must then self-exec
under torch.distributed.run so N ranks actually run and the reported
`n_gpus` equals N — otherwise an 8-GPU scaling measurement silently
becomes a 1-rank run (round-1 VERDICT.md, top priority fix).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

BENCH = os.path.join(os.path.dirname(__file__), os.pardir, "bench.py")


def _run_bench(extra_args, timeout=600, ranks=1):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    import torch

    if torch.cuda.is_available() and torch.cuda.device_count() < ranks:
        # fewer GPUs than ranks: RCCL refuses two ranks on one device, so
        # the ranks share it over gloo (parallel/ddp.py init_from_env)
        env.setdefault("RL_REPLICAS_AMD_DIST_BACKEND", "gloo")
    return subprocess.run(
        [sys.executable, BENCH] + extra_args,
        capture_output=True,
        text=True,
        timeout=timeout,
        env=env,
    )


def _parse_json_line(stdout: str) -> dict:
    for line in stdout.splitlines():
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in bench stdout:\n{stdout}")


@pytest.mark.slow
def test_gpus_flag_spawns_ranks():
    """`python bench.py --gpus 2` with no torchrun env must run 2 ranks."""
    r = _run_bench(
        ["--gpus", "2", "--steps", "1", "--warmup", "0", "--num-envs", "4",
         "--batch-per-gpu", "64", "--env", "cpu"],
        ranks=2,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    result = _parse_json_line(r.stdout)
    assert result["n_gpus"] == 2
    assert result["config"]["parallelism"] == "dp2"
    assert result["config"]["global_batch"] == 128  # world * batch_per_gpu


def test_world_size_mismatch_fails_loudly():
    """--gpus 4 under a WORLD_SIZE=1 env must abort, not report n_gpus=4."""
    env = dict(os.environ)
    env.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "4", "--steps", "1", "--warmup", "0"],
        capture_output=True,
        text=True,
        timeout=300,
        env=env,
    )
    assert r.returncode != 0
    assert "refusing" in (r.stderr + r.stdout)


def test_single_gpu_json_contract():
    r = _run_bench(
        ["--steps", "2", "--warmup", "1", "--num-envs", "4",
         "--batch-per-gpu", "64", "--env", "cpu"]
    )
    assert r.returncode == 0, r.stderr[-3000:]
    result = _parse_json_line(r.stdout)
    for key in (
        "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
        "timed_region_s", "avg_return", "config",
    ):
        assert key in result, key
    assert result["n_gpus"] == 1
    assert result["steps"] == 2 and result["warmup"] == 1
    assert result["value"] > 0
    assert result["avg_return"]["last_epoch"] is not None


def test_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's batch and trained
    parameters as float32/float64 .npy files; equal arguments give equal
    inputs, so two runs must dump the same arrays.  --full is accepted
    and keeps the result line's contract."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / name
        r = _run_bench(
            ["--steps", "2", "--warmup", "1", "--num-envs", "4",
             "--batch-per-gpu", "64", "--env", "cpu", "--dump-outputs", str(out)]
            + extra
        )
        assert r.returncode == 0, r.stderr[-3000:]
        result = _parse_json_line(r.stdout)
        assert result["steps"] == 2 and result["ms_per_step"] > 0
        assert result["ms_per_step"] == pytest.approx(
            result["timed_region_s"] / 2 * 1000.0
        )
        dumps.append({p.name: np.load(p) for p in sorted(out.glob("*.npy"))})

    a, b = dumps
    assert a.keys() == b.keys()
    for expected in (
        "experience.observations.npy", "experience.actions.npy",
        "experience.rewards.npy", "policy.network.0.weight.npy",
        "policy.log_std.npy", "value_function.network.4.weight.npy",
    ):
        assert expected in a, expected
    assert a["experience.observations.npy"].shape == (64, 17)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1024 * 1024
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.isfinite(a[name]).all(), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
