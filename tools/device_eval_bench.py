"""Time of one `evaluate()` call of the policy-evaluation paths on one GPU.

    python tools/device_eval_bench.py --out profiles/bench_device_eval_1gpu.json

Shapes: the off-policy actor [3,256,256,1] (ReLU, Tanh head) on Pendulum-v1
at 5 and 256 episodes of 200 steps; a Gaussian policy [3,64,32,1] at 16
episodes; a categorical policy on CartPole-v1 at 16 and 256 episodes with
horizon 500, once as the untrained [4,64,32,2] net (episodes end after a few
dozen steps) and once as a hand-set linear net [4,2] that balances (every
episode runs the whole horizon).

  a  host    Evaluator: the numpy env stepped on the host, policy on the GPU
  e  eager   DeviceEvaluator with graphs disabled: the private device env's
             kernels and the policy's get_action_tensor, one read-back
  c  graph   DeviceEvaluator, captured multi-kernel body
  d  fused   DeviceEvaluator, pendulum_eval_fused / cartpole_eval_fused

Every path and shape is warmed first; then the paths run alternated for
`--rounds` rounds in this one process, each timed window `--evals` calls long
with one synchronise before and one after, so the run-to-run spread is
visible next to the ratios.  CartPole cases record the mean episode length
beside each time.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ENV_KEYS = ("RL_REPLICAS_AMD_ROLLOUT_FUSED", "RL_REPLICAS_AMD_DISABLE_GRAPHS")
PATHS = {
    "a_host": None,
    "e_device_eager": {"RL_REPLICAS_AMD_DISABLE_GRAPHS": "1"},
    "c_graph_multi_kernel": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "0"},
    "d_fused": {"RL_REPLICAS_AMD_ROLLOUT_FUSED": "1"},
}
EXPECTED_PATH = {"e_device_eager": "eager", "c_graph_multi_kernel": "graph",
                 "d_fused": "fused"}
# (case name, env id, horizon, policy kind, episodes)
CASES = [
    ("pendulum_actor_256x256", "Pendulum-v1", 200, "deterministic", 5),
    ("pendulum_actor_256x256", "Pendulum-v1", 200, "deterministic", 256),
    ("pendulum_gaussian_64x32", "Pendulum-v1", 200, "gaussian", 16),
    ("cartpole_untrained_64x32", "CartPole-v1", 500, "untrained", 16),
    ("cartpole_untrained_64x32", "CartPole-v1", 500, "untrained", 256),
    ("cartpole_balancing_linear", "CartPole-v1", 500, "balancing", 16),
    ("cartpole_balancing_linear", "CartPole-v1", 500, "balancing", 256),
]
# logits = -+ 5 * (0.5 x + x_dot + 10 theta + 2 theta_dot): pushes under the pole
BALANCE = [2.5, 5.0, 50.0, 10.0]


def make_policy(kind):
    import torch.nn as nn

    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import CategoricalPolicy, DeterministicPolicy, GaussianPolicy

    torch.manual_seed(0)
    if kind == "deterministic":
        net = MLP([3, 256, 256, 1], activation_function=nn.ReLU,
                  output_activation_function=nn.Tanh).to("cuda")
        return DeterministicPolicy(net, ops.make_adam(net.parameters(), lr=1e-3))
    if kind == "gaussian":
        net = MLP([3, 64, 32, 1]).to("cuda")
        log_std = nn.Parameter(-0.5 * torch.ones(1, device="cuda"))
        params = list(net.parameters()) + [log_std]
        return GaussianPolicy(net, ops.make_adam(params, lr=3e-4), log_std)
    if kind == "untrained":
        net = MLP([4, 64, 32, 2]).to("cuda")
    else:
        net = MLP([4, 2]).to("cuda")
        with torch.no_grad():
            w = torch.tensor(BALANCE, device="cuda")
            net.network[0].weight.copy_(torch.stack([-w, w]))
            net.network[0].bias.zero_()
    return CategoricalPolicy(net, ops.make_adam(net.parameters(), lr=3e-4))


def make_runner(name, env_id, horizon, kind, episodes):
    from rl_replicas_amd import envs
    from rl_replicas_amd.evaluator import DeviceEvaluator, Evaluator

    policy = make_policy(kind)
    env = envs.make(env_id)
    env.spec.max_episode_steps = horizon
    evaluator = Evaluator(seed=0) if PATHS[name] is None else DeviceEvaluator(seed=0)
    setting = PATHS[name] or {}
    last = {}

    def run():
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(setting)
        last["out"] = evaluator.evaluate(policy, env, episodes)

    def check():
        returns, lengths = last["out"]
        assert len(returns) == episodes and len(lengths) == episodes
        if name in EXPECTED_PATH:
            assert evaluator.last_path == EXPECTED_PATH[name], (name, evaluator.last_path)
        return sum(lengths) / len(lengths)

    return run, check


def timed_window(run, evals):
    """ms per evaluate() over `evals` calls between two synchronises."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(evals):
        run()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("device_eval_bench needs a GPU")
    from rl_replicas_amd import ops

    assert ops.hip_available(), "HIP ops extension must load"

    runners, mean_len = {}, {}
    for case in CASES:
        for name in PATHS:
            run, check = make_runner(name, *case[1:])
            for _ in range(args.warmup):  # allocations, the graph capture
                run()
            torch.cuda.synchronize()
            check()
            runners[(case, name)] = (run, check)
            print(f"warmed {case} {name}", file=sys.stderr, flush=True)

    samples = {key: [] for key in runners}
    for r in range(args.rounds):
        for key, (run, check) in runners.items():
            samples[key].append(timed_window(run, args.evals))
            mean_len[key] = check()
        print(f"round {r + 1}/{args.rounds} done", file=sys.stderr, flush=True)

    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "warmup_evals": args.warmup, "timed_evals": args.evals,
              "what": "ms per evaluate()", "cases": []}
    for case in CASES:
        per_path = {}
        for name in PATHS:
            xs = sorted(samples[(case, name)])
            med = xs[len(xs) // 2]
            per_path[name] = {
                "ms_per_eval_rounds": [round(x, 4) for x in samples[(case, name)]],
                "ms_per_eval_median": round(med, 4),
                "spread_rel": round((xs[-1] - xs[0]) / med, 4),
            }
            if case[1] == "CartPole-v1":
                per_path[name]["mean_episode_length"] = round(mean_len[(case, name)], 2)
        m = {k: v["ms_per_eval_median"] for k, v in per_path.items()}
        result["cases"].append({
            "case": case[0], "env": case[1], "horizon": case[2], "policy": case[3],
            "episodes": case[4], "paths": per_path,
            "speedup_d_vs_c": round(m["c_graph_multi_kernel"] / m["d_fused"], 3),
            "speedup_d_vs_e": round(m["e_device_eager"] / m["d_fused"], 3),
            "speedup_d_vs_a": round(m["a_host"] / m["d_fused"], 3),
            "speedup_c_vs_a": round(m["a_host"] / m["c_graph_multi_kernel"], 3),
        })
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
