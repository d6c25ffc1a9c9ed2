"""Per-epoch `sample()` + `add_experience()` time of the off-policy collection
paths on one GPU, on Pendulum-v1 (the default) or a synthetic env.

    python tools/replay_collect_bench.py --out profiles/bench_replay_collect_1gpu.json
    python tools/replay_collect_bench.py --env Ant-v4 \
        --out profiles/bench_synthetic_collect_1gpu.json

Actor [3,256,256,1] (ReLU, Tanh head; the benchmark actor), both behaviour
policies of `OffPolicyAlgorithm.learn` (uniform warm-up, noised actor), at
the off-policy shapes 1 env x 50 steps and 10 envs x 5 steps and at
200 envs x 20 steps, into a 1e6-slot ring:

  a  host        VectorEnv("Pendulum-v1") + VectorSampler, actor on the GPU
  e  eager       DeviceSampler on DevicePendulumEnv's kernels + the tensor
                 ring copy of add_experience
  c  graph       DeviceReplaySampler, captured multi-kernel body
  d  persistent  DeviceReplaySampler, pendulum_collect_fused; in noised mode
                 at both workgroup sizes of its wide regime (uniform mode
                 reads no net and has one kernel)

Every path and shape is warmed for `--warmup` epochs first (enough for every
lockstep cut pattern of horizon 200 to have its graph); then the paths run
alternated for `--rounds` rounds in this one process, each timed window
`--epochs` calls long with one synchronise before and one after, so the
run-to-run spread is visible next to the ratios.

With `--env` naming a synthetic env (Ant-v4, ...) the same protocol runs on
VectorEnv(env) / DeviceVectorEnv(env) with the actor [O,256,256,A] and
synthetic_collect_fused; a shape is then warmed for at least
horizon / steps + 5 epochs, so that the 1000-step horizon's cut patterns
have their graphs too.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = [(1, 50), (10, 5), (200, 20)]
DIMS = [3, 256, 256, 1]
MODES = ("uniform", "noised")
RING = int(1e6)
ENV_KEYS = ("RL_REPLICAS_AMD_ROLLOUT_FUSED", "RL_REPLICAS_AMD_COLLECT_WG")
PATHS = {
    "a_host": None,
    "e_device_eager": {},
    "c_graph_multi_kernel": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "0"},
    "d_persistent_wg256": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "1",
                           "RL_REPLICAS_AMD_COLLECT_WG": "256"},
    "d_persistent_wg1024": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "1",
                            "RL_REPLICAS_AMD_COLLECT_WG": "1024"},
}


def actor_dims(env_id):
    if env_id == "Pendulum-v1":
        return DIMS
    from rl_replicas_amd.envs import MUJOCO_SHAPES

    obs_dim, act_dim = MUJOCO_SHAPES[env_id]
    return [obs_dim, 256, 256, act_dim]


def warmup_epochs(env_id, warmup, steps):
    """Epochs that bring every lockstep cut pattern of the env's horizon."""
    if env_id == "Pendulum-v1":
        return warmup
    from rl_replicas_amd import envs

    horizon = envs.make(env_id).spec.max_episode_steps or 0
    return max(warmup, horizon // steps + 5)


def paths_of(mode):
    # uniform mode reads no net: the persistent kernel has no wide regime
    return [p for p in PATHS if not (mode == "uniform" and p == "d_persistent_wg1024")]


def make_runner(name, mode, n_envs, steps, env_id="Pendulum-v1"):
    import torch.nn as nn

    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
    from rl_replicas_amd.replay_buffer import ReplayBuffer
    from rl_replicas_amd.samplers import DeviceReplaySampler, DeviceSampler, VectorSampler
    from rl_replicas_amd.utils import add_noise_to_get_action

    torch.manual_seed(0)
    pendulum = env_id == "Pendulum-v1"

    def device_env():
        if pendulum:
            return envs.DevicePendulumEnv(n_envs, device="cuda")
        return envs.DeviceVectorEnv(env_id, n_envs, device="cuda")

    net = MLP(actor_dims(env_id), activation_function=nn.ReLU, output_activation_function=nn.Tanh).to("cuda")
    det = DeterministicPolicy(net, ops.make_adam(net.parameters(), lr=1e-3))
    buf = ReplayBuffer(RING, device="cuda")
    if PATHS[name] is None:
        env = envs.VectorEnv(env_id, num_envs=n_envs)
        sampler = VectorSampler(env, seed=0, is_continuous=True)
    elif name == "e_device_eager":
        env = device_env()
        sampler = DeviceSampler(env, seed=0, is_continuous=True)
    else:
        env = device_env()
        sampler = DeviceReplaySampler(env, buf, seed=0)
    policy = (RandomPolicy(env.action_space) if mode == "uniform"
              else add_noise_to_get_action(det, env.action_space, 0.1))
    setting = PATHS[name] or {}

    def run():
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(setting)
        buf.add_experience(sampler.sample(n_envs * steps, policy))

    def check(epochs_run):
        assert len(buf) == min(epochs_run * n_envs * steps, RING), (name, len(buf))
        if name.startswith(("c_", "d_")):
            graphs = sampler._graphs.values()
            assert graphs and {g.fused for g in graphs} == {name.startswith("d_")}, name
            assert {g.mode for g in graphs} == {mode}
        else:
            assert not getattr(sampler, "_graphs", None)

    return run, check


def timed_window(run, epochs):
    """ms per sample() + add_experience() over `epochs` calls between two
    synchronises."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        run()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=45)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--env", default="Pendulum-v1",
                    help="Pendulum-v1 or a synthetic env id (Ant-v4, ...)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_collect_bench needs a GPU")
    from rl_replicas_amd import ops

    assert ops.hip_available(), "HIP ops extension must load"

    runners = {}
    for mode in MODES:
        for shape in SHAPES:
            for name in paths_of(mode):
                run, check = make_runner(name, mode, *shape, env_id=args.env)
                warm = warmup_epochs(args.env, args.warmup, shape[1])
                for _ in range(warm):  # allocations, every graph pattern
                    run()
                torch.cuda.synchronize()
                check(warm)
                runners[(mode, shape, name)] = run
                print(f"warmed {mode} {shape} {name}", file=sys.stderr, flush=True)

    samples = {key: [] for key in runners}
    for r in range(args.rounds):
        for key, run in runners.items():
            samples[key].append(timed_window(run, args.epochs))
        print(f"round {r + 1}/{args.rounds} done", file=sys.stderr, flush=True)

    result = {"device": torch.cuda.get_device_name(0), "actor": actor_dims(args.env),
              "ring_slots": RING,
              "rounds": args.rounds, "warmup_epochs": args.warmup,
              "timed_epochs": args.epochs, "what": "ms per sample() + add_experience()",
              "cases": []}
    if args.env != "Pendulum-v1":
        result = {"env": args.env, **result,
                  "warmup_epochs_min_per_shape": "horizon / steps + 5"}
    for mode in MODES:
        for shape in SHAPES:
            per_path = {}
            for name in paths_of(mode):
                xs = sorted(samples[(mode, shape, name)])
                med = xs[len(xs) // 2]
                per_path[name] = {
                    "ms_per_epoch_rounds": [round(x, 4) for x in samples[(mode, shape, name)]],
                    "ms_per_epoch_median": round(med, 4),
                    "spread_rel": round((xs[-1] - xs[0]) / med, 4),
                }
            m = {k: v["ms_per_epoch_median"] for k, v in per_path.items()}
            case = {"mode": mode, "num_envs": shape[0], "steps": shape[1],
                    "paths": per_path}
            for d in (p for p in m if p.startswith("d_")):
                tag = d[len("d_persistent_"):]
                case[f"speedup_d_{tag}_vs_c"] = round(m["c_graph_multi_kernel"] / m[d], 3)
                case[f"speedup_d_{tag}_vs_e"] = round(m["e_device_eager"] / m[d], 3)
            case["speedup_c_vs_e"] = round(m["e_device_eager"] / m["c_graph_multi_kernel"], 3)
            case["speedup_c_vs_a"] = round(m["a_host"] / m["c_graph_multi_kernel"], 3)
            result["cases"].append(case)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
