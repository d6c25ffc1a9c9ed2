"""Per-epoch PPO update time (policy + value) of a categorical policy on one
GPU.

    python tools/categorical_ppo_update_bench.py \
        --out profiles/bench_categorical_ppo_update_1gpu.json

CategoricalPolicy [4,64,64,2] + value net [4,64,64,1], batch 4000, 80 policy
and 80 value iterations, at max_kl_divergence 1e9 (every iteration runs) and
at the default 0.01 (KL early stop), three paths:

  a  multi_kernel  RL_REPLICAS_AMD_CATEGORICAL_ITER=0: chunked multi-kernel
                   policy loop, then the value loop graph
  b  fused_iter    fused 2-kernel policy iteration, RL_REPLICAS_AMD_PPO_TWIN=0:
                   separate policy and value loops
  c  twin_graph    one graph per epoch, twin kernel pair per iteration

Every timed call restores parameters, Adam state and the old policy to the
same snapshot first (inside the timed region, the same few copies on every
path), so every call of every path runs the same epoch from the same state
and the early-stop count cannot drift with how often a path has run.

Every path and setting is warmed first; then the paths run alternated for
`--rounds` rounds in this one process, each timed window lasting at least
`--window` seconds and ending in a synchronise, so the run-to-run spread is
visible next to the ratios.  `--only c_twin_graph --epochs N` runs N epochs
of one path and exits (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

P_DIMS = [4, 64, 64, 2]
V_DIMS = [4, 64, 64, 1]
BATCH = 4000
ITERS = 80
MAX_KLS = {"max_kl_1e9": 1e9, "max_kl_default": 0.01}
ENV_KEYS = ("RL_REPLICAS_AMD_CATEGORICAL_ITER", "RL_REPLICAS_AMD_PPO_TWIN")
PATHS = {
    "a_multi_kernel": {"RL_REPLICAS_AMD_CATEGORICAL_ITER": "0"},
    "b_fused_iter": {"RL_REPLICAS_AMD_PPO_TWIN": "0"},
    "c_twin_graph": {},
}


def make_batch():
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(BATCH, P_DIMS[0], generator=g).cuda()
    actions = torch.randint(0, P_DIMS[-1], (BATCH,), generator=g).float().cuda()
    adv = torch.randn(BATCH, generator=g).cuda()
    returns = torch.randn(BATCH, generator=g).cuda()
    return obs, actions, adv, returns


def make_runner(name, max_kl, batch):
    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.algorithms import PPO
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.ops.fused_onpolicy import _ensure_adam_state
    from rl_replicas_amd.policies import CategoricalPolicy
    from rl_replicas_amd.samplers import VectorSampler
    from rl_replicas_amd.value_function import ValueFunction

    torch.manual_seed(0)
    pnet = MLP(P_DIMS).to("cuda")
    policy = CategoricalPolicy(pnet, ops.make_adam(pnet.parameters(), lr=3e-4))
    vnet = MLP(V_DIMS).to("cuda")
    vf = ValueFunction(vnet, ops.make_adam(vnet.parameters(), lr=1e-3))
    venv = envs.VectorEnv("CartPole-v1", num_envs=2)
    model = PPO(policy, vf, venv, VectorSampler(venv, seed=0),
                max_kl_divergence=max_kl, num_policy_gradients=ITERS,
                num_value_gradients=ITERS)
    state = [p.data for p in policy.parameters()]
    state += [p.data for p in model.old_policy.parameters()]
    state += [p.data for p in vf.parameters()]
    state += _ensure_adam_state(policy.optimizer)
    state += _ensure_adam_state(vf.optimizer)
    snapshot = [t.clone() for t in state]
    setting = PATHS[name]
    obs, actions, adv, returns = batch

    def run():
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(setting)
        torch._foreach_copy_(state, snapshot)
        joint = model._update_policy_and_value(obs, actions, adv, returns)
        if joint is None:
            joint = (model._update_policy(obs, actions, adv),
                     model._update_value_function(obs, returns))
        return joint

    def iters_done():
        twin = getattr(model, "_ppo_twin_graph", None)
        graph = twin if twin is not None else model._ppo_policy_graph
        return int(graph[1].iters_done)

    def check():
        twin = getattr(model, "_ppo_twin_graph", None)
        assert (twin is not None) == name.startswith("c_"), (name, twin)
        if twin is None:
            fused = bool(model._ppo_policy_graph[1].use_mega)
            assert fused == name.startswith("b_"), (name, fused)
        else:
            assert twin[1].kind == "categorical"

    return run, check, iters_done


def timed_window(run, min_seconds):
    """ms per update over a window of at least `min_seconds`, measured to a
    closing synchronise."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=list(PATHS))
    ap.add_argument("--epochs", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("categorical_ppo_update_bench needs a GPU")
    from rl_replicas_amd import ops

    assert ops.hip_available(), "HIP ops extension must load"
    batch = make_batch()

    if args.only:
        for max_kl in MAX_KLS.values():
            run, check, _ = make_runner(args.only, max_kl, batch)
            for _ in range(args.epochs):
                run()
            torch.cuda.synchronize()
            check()
        return

    runners, iters = {}, {}
    for kl_name, max_kl in MAX_KLS.items():
        for name in PATHS:
            run, check, iters_done = make_runner(name, max_kl, batch)
            for _ in range(3):  # warm: allocations, graph capture
                run()
            torch.cuda.synchronize()
            check()
            runners[(kl_name, name)] = run
            iters[(kl_name, name)] = iters_done()

    samples = {key: [] for key in runners}
    for _ in range(args.rounds):
        for key, run in runners.items():
            ms, _ = timed_window(run, args.window)
            samples[key].append(ms)

    result = {"device": torch.cuda.get_device_name(0), "policy_net": P_DIMS,
              "value_net": V_DIMS, "batch": BATCH, "policy_iters": ITERS,
              "value_iters": ITERS, "rounds": args.rounds,
              "window_s": args.window, "settings": []}
    for kl_name, max_kl in MAX_KLS.items():
        per_path = {}
        for name in PATHS:
            xs = sorted(samples[(kl_name, name)])
            med = xs[len(xs) // 2]
            per_path[name] = {
                "ms_per_update_rounds": [round(x, 4) for x in samples[(kl_name, name)]],
                "ms_per_update_median": round(med, 4),
                "spread_rel": round((xs[-1] - xs[0]) / med, 4),
                "policy_iters_done": iters[(kl_name, name)],
            }
        m = {k: v["ms_per_update_median"] for k, v in per_path.items()}
        result["settings"].append({
            "name": kl_name, "max_kl_divergence": max_kl, "paths": per_path,
            "speedup_c_vs_a": round(m["a_multi_kernel"] / m["c_twin_graph"], 3),
            "speedup_b_vs_a": round(m["a_multi_kernel"] / m["b_fused_iter"], 3),
            "speedup_c_vs_b": round(m["b_fused_iter"] / m["c_twin_graph"], 3),
        })
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
