"""Per-epoch `sample()` time of the CartPole rollout paths on one GPU.

    python tools/cartpole_rollout_bench.py --out profiles/bench_cartpole_rollout_1gpu.json

CategoricalPolicy [4,64,64,2] at 200 envs x 20 steps and 16 envs x 250
steps, four paths:

  a  host     VectorEnv("CartPole-v1") + VectorSampler, policy on the GPU
  b  eager    DeviceCartPoleEnv + DeviceEpisodicSampler, graphs disabled
  c  graph    captured epoch, multi-kernel body
  d  fused    captured epoch, persistent kernel

Every path and shape is warmed first; then the paths run alternated for
`--rounds` rounds in this one process, each timed window lasting at least
`--window` seconds and ending in a synchronise, so the run-to-run spread
is visible next to the ratios.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = [(200, 20), (16, 250)]
DIMS = [4, 64, 64, 2]
ENV_KEYS = ("RL_REPLICAS_AMD_DISABLE_GRAPHS", "RL_REPLICAS_AMD_ROLLOUT_FUSED")
PATHS = {
    "a_host": None,
    "b_device_eager": {"RL_REPLICAS_AMD_DISABLE_GRAPHS": "1"},
    "c_graph_multi_kernel": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "0"},
    "d_graph_persistent": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "1"},
}


def make_runner(name, n_envs, steps):
    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import CategoricalPolicy
    from rl_replicas_amd.samplers import DeviceEpisodicSampler, VectorSampler

    torch.manual_seed(0)
    pnet = MLP(DIMS).to("cuda")
    policy = CategoricalPolicy(pnet, ops.make_adam(pnet.parameters(), lr=3e-4))
    if PATHS[name] is None:
        sampler = VectorSampler(envs.VectorEnv("CartPole-v1", num_envs=n_envs), seed=0,
                                is_continuous=True)
    else:
        sampler = DeviceEpisodicSampler(
            envs.DeviceCartPoleEnv(n_envs, device="cuda"), seed=0, is_continuous=True
        )
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
        elif name.startswith("b_"):
            assert not sampler._graphs

    return run, check


def timed_window(run, min_seconds):
    """ms per sample() over a window of at least `min_seconds`, measured to
    a closing synchronise."""
    torch.cuda.synchronize()
    calls = 0
    t0 = time.perf_counter()
    while True:
        run()
        calls += 1
        if time.perf_counter() - t0 >= min_seconds:
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            return 1000.0 * elapsed / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cartpole_rollout_bench needs a GPU")
    from rl_replicas_amd import ops

    assert ops.hip_available(), "HIP ops extension must load"

    runners = {}
    for shape in SHAPES:
        for name in PATHS:
            run, check = make_runner(name, *shape)
            for _ in range(3):  # warm: allocations, graph capture
                run()
            torch.cuda.synchronize()
            check()
            runners[(shape, name)] = run

    samples = {key: [] for key in runners}
    for _ in range(args.rounds):
        for key, run in runners.items():
            ms, _ = timed_window(run, args.window)
            samples[key].append(ms)

    result = {"device": torch.cuda.get_device_name(0), "net": DIMS,
              "rounds": args.rounds, "window_s": args.window, "shapes": []}
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
            "speedup_c_vs_a": round(m["a_host"] / m["c_graph_multi_kernel"], 3),
            "speedup_d_vs_c": round(m["c_graph_multi_kernel"] / m["d_graph_persistent"], 3),
            "speedup_d_vs_b": round(m["b_device_eager"] / m["d_graph_persistent"], 3),
        })
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
