"""Per-epoch `sample()` time of the Pendulum rollout paths on one GPU.

    python tools/pendulum_rollout_bench.py --out profiles/bench_pendulum_rollout_1gpu.json

GaussianPolicy [3,64,32,1] at 200 envs x 20 steps and 16 envs x 250 steps,
five paths:

  a  host       VectorEnv("Pendulum-v1") + VectorSampler, policy on the GPU
  b  torch ops  DevicePendulumEnv stepped by torch fp64 ops from the host
                (the env as it was before it had kernels), eager loop
  e  eager      DevicePendulumEnv on its kernels, graphs disabled
  c  graph      captured epoch, multi-kernel body
  d  fused      captured epoch, persistent kernel

Every path and shape is warmed for `--warmup` epochs first; then the paths
run alternated for `--rounds` rounds in this one process, each timed window
`--epochs` calls long with one synchronise before and one after, so the
run-to-run spread is visible next to the ratios.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = [(200, 20), (16, 250)]
DIMS = [3, 64, 32, 1]
ENV_KEYS = ("RL_REPLICAS_AMD_DISABLE_GRAPHS", "RL_REPLICAS_AMD_ROLLOUT_FUSED")
PATHS = {
    "a_host": None,
    "b_device_torch_ops": {"RL_REPLICAS_AMD_DISABLE_GRAPHS": "1"},
    "e_device_eager": {"RL_REPLICAS_AMD_DISABLE_GRAPHS": "1"},
    "c_graph_multi_kernel": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "0"},
    "d_graph_persistent": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "1"},
}


def make_torch_op_env(n_envs):
    """DevicePendulumEnv with its kernels switched off: every step is the
    torch-op arithmetic and rebinds `state`, as before the kernels."""
    from rl_replicas_amd.envs import DevicePendulumEnv

    class TorchOpPendulumEnv(DevicePendulumEnv):
        state = None  # a plain attribute again: `self.state = ...` rebinds

        def _wants_hip(self):
            return False

    return TorchOpPendulumEnv(n_envs, device="cuda")


def make_runner(name, n_envs, steps):
    import torch.nn as nn

    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import GaussianPolicy
    from rl_replicas_amd.samplers import DeviceSampler, VectorSampler

    torch.manual_seed(0)
    pnet = MLP(DIMS).to("cuda")
    log_std = nn.Parameter(-0.5 * torch.ones(1, device="cuda"))
    policy = GaussianPolicy(
        pnet, ops.make_adam(list(pnet.parameters()) + [log_std], lr=3e-4), log_std
    )
    if PATHS[name] is None:
        sampler = VectorSampler(envs.VectorEnv("Pendulum-v1", num_envs=n_envs), seed=0,
                                is_continuous=True)
    elif name == "b_device_torch_ops":
        sampler = DeviceSampler(make_torch_op_env(n_envs), seed=0, is_continuous=True)
    else:
        sampler = DeviceSampler(envs.DevicePendulumEnv(n_envs, device="cuda"), seed=0,
                                is_continuous=True)
    setting = PATHS[name] or {}

    def run():
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(setting)
        return sampler.sample(n_envs * steps, policy)

    def check():
        if name.startswith(("c_", "d_")):
            fused = {g.fused for g in sampler._graphs.values()}
            assert fused == {name.startswith("d_")}, (name, fused)
        elif name.startswith(("b_", "e_")):
            assert not sampler._graphs

    return run, check


def timed_window(run, epochs):
    """ms per sample() over `epochs` calls between two synchronises."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        run()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pendulum_rollout_bench needs a GPU")
    from rl_replicas_amd import ops

    assert ops.hip_available(), "HIP ops extension must load"

    runners = {}
    for shape in SHAPES:
        for name in PATHS:
            run, check = make_runner(name, *shape)
            for _ in range(args.warmup):  # allocations, every graph pattern
                run()
            torch.cuda.synchronize()
            check()
            runners[(shape, name)] = run
            print(f"warmed {shape} {name}", file=sys.stderr, flush=True)

    samples = {key: [] for key in runners}
    for r in range(args.rounds):
        for key, run in runners.items():
            samples[key].append(timed_window(run, args.epochs))
        print(f"round {r + 1}/{args.rounds} done", file=sys.stderr, flush=True)

    result = {"device": torch.cuda.get_device_name(0), "net": DIMS,
              "rounds": args.rounds, "warmup_epochs": args.warmup,
              "timed_epochs": args.epochs, "shapes": []}
    for shape in SHAPES:
        per_path = {}
        for name in PATHS:
            xs = sorted(samples[(shape, name)])
            med = xs[len(xs) // 2]
            per_path[name] = {
                "ms_per_epoch_rounds": [round(x, 4) for x in samples[(shape, name)]],
                "ms_per_epoch_median": round(med, 4),
                "spread_rel": round((xs[-1] - xs[0]) / med, 4),
            }
        m = {k: v["ms_per_epoch_median"] for k, v in per_path.items()}
        result["shapes"].append({
            "num_envs": shape[0], "steps": shape[1], "paths": per_path,
            "speedup_d_vs_a": round(m["a_host"] / m["d_graph_persistent"], 3),
            "speedup_d_vs_b": round(m["b_device_torch_ops"] / m["d_graph_persistent"], 3),
            "speedup_d_vs_e": round(m["e_device_eager"] / m["d_graph_persistent"], 3),
            "speedup_d_vs_c": round(m["c_graph_multi_kernel"] / m["d_graph_persistent"], 3),
            "speedup_c_vs_b": round(m["b_device_torch_ops"] / m["c_graph_multi_kernel"], 3),
        })
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
