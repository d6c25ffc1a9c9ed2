"""Policy evaluator.

API parity: reference src/rl_replicas/evaluator.py:9-52 — runs
`num_episodes` full episodes in a separate env and returns
`(episode_returns, episode_lengths)`; seeds the env on the first reset
only.  Stochastic policies SAMPLE during evaluation (the reference has
no deterministic flag); DDPG/TD3 pass the un-noised deterministic
policy (reference ddpg.py:155).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from rl_replicas_amd.policies import Policy


class Evaluator:
    def __init__(self, seed: Optional[int] = None, vectorized: bool = True):
        self.seed = seed
        self.vectorized = vectorized

    def evaluate(self, policy: Policy, env, num_episodes: int) -> Tuple[List[float], List[int]]:
        if self.vectorized and hasattr(env, "_reset_b"):
            return self._evaluate_vectorized(policy, env, num_episodes)
        return self._evaluate_serial(policy, env, num_episodes)

    # serial reference path (third-party envs)
    def _evaluate_serial(self, policy: Policy, env, num_episodes: int):
        episode_returns: List[float] = []
        episode_lengths: List[int] = []

        observation, _ = env.reset(seed=self.seed)
        for _ in range(num_episodes):
            done = False
            ep_return = 0.0
            ep_length = 0
            while not done:
                action = policy.get_action_numpy(observation)
                observation, reward, terminated, truncated, _ = env.step(action)
                done = bool(terminated or truncated)
                ep_return += float(reward)
                ep_length += 1
            observation, _ = env.reset()
            episode_returns.append(ep_return)
            episode_lengths.append(ep_length)

        return episode_returns, episode_lengths

    # MI355X fast path: all episodes advance together — one batched
    # policy forward per step instead of num_episodes serial rollouts
    # (episodes are independent, so the returns distribution is the
    # reference's; only the RNG consumption pattern differs)
    def _evaluate_vectorized(self, policy: Policy, env, num_episodes: int):
        import numpy as np

        from rl_replicas_amd.envs.vector import VectorEnv

        venv = VectorEnv(env, num_episodes)
        # reseed on EVERY call, like the reference's reset(seed=self.seed)
        # (evaluator.py:30) and our own serial path: periodic evaluations
        # start from the same seeded initial states each time
        obs = venv.reset(seed=self.seed)
        returns = np.zeros(num_episodes)
        lengths = np.zeros(num_episodes, dtype=np.int64)
        finished = np.zeros(num_episodes, dtype=bool)
        max_steps = env.spec.max_episode_steps or 100_000
        for _ in range(max_steps):
            actions = np.asarray(policy.get_action_numpy(obs))
            obs, rewards, terminated, truncated, _ = venv.step(actions)
            active = ~finished
            returns[active] += rewards[active]
            lengths[active] += 1
            finished |= terminated | truncated
            if finished.all():
                break
        return returns.tolist(), lengths.tolist()


class DeviceEvaluator(Evaluator):
    """`Evaluator` whose Pendulum-v1 and CartPole-v1 episodes run on the
    policy's device, without a host env in the loop.

    `evaluate(policy, env, num_episodes)` recognises `env` by type and
    `spec.id` -- a host `PendulumEnv` / `CartPoleEnv` (what
    `OffPolicyAlgorithm.evaluation_env` is) or a `DevicePendulumEnv` /
    `DeviceCartPoleEnv` -- and never steps or resets it: the episodes run in
    a private device env of `num_episodes` instances with
    `horizon = env.spec.max_episode_steps`.  `last_path` records what ran:

      "fused" / "graph"  GPU, extension present, graphs enabled: one captured
                         evaluation (`ops/fused_rollout.py::GraphedPendulumEval`
                         / `GraphedCartPoleEval`), the persistent kernel or
                         the multi-kernel body
      "eager"            the same policy/env pairs on the CPU, with graphs
                         disabled or with a full graph cache: a Python loop
                         over the private env and `policy.get_action_tensor`,
                         first-episode masking on the device, one read-back
      "host"             anything else: `Evaluator.evaluate`, unchanged

    Seeded (`seed` is not None), every call starts from the same initial
    states -- the reseed-on-every-call contract of `Evaluator`; unseeded, the
    initial states advance with each call.  Stochastic policies draw fresh
    actions on every call either way.  After a graphed call
    `last_initial_state` is the kernel's `init_state` tensor, after an eager
    call a copy of the private env's initial state.

    No reference counterpart (the reference steps one host env serially,
    evaluator.py:9-52)."""

    MAX_GRAPHS = 8

    def __init__(self, seed: Optional[int] = None, device=None):
        super().__init__(seed=seed)
        self.device = device
        self.last_path: Optional[str] = None
        self.last_initial_state = None
        self._envs = {}      # (kind, num_episodes, horizon, device) -> private env
        self._graphs = {}    # (kind, mode, num_episodes, horizon, id(policy)) -> (graph, policy)
        self._counters = {}  # device -> (ctr, reset_ctr)

    # -- recognition --------------------------------------------------------
    @staticmethod
    def _env_kind(env) -> Optional[str]:
        from rl_replicas_amd.envs.classic import CartPoleEnv, PendulumEnv
        from rl_replicas_amd.envs.device import DeviceCartPoleEnv, DevicePendulumEnv

        spec_id = getattr(getattr(env, "spec", None), "id", None)
        if isinstance(env, (PendulumEnv, DevicePendulumEnv)) and spec_id == "Pendulum-v1":
            return "pendulum"
        if isinstance(env, (CartPoleEnv, DeviceCartPoleEnv)) and spec_id == "CartPole-v1":
            return "cartpole"
        return None

    @staticmethod
    def _policy_mode(policy, kind: str) -> Optional[str]:
        """The action law of `policy` on a `kind` env, or None when the pair
        is not one the device paths take."""
        import torch.nn as nn

        from rl_replicas_amd.ops import fused_onpolicy as fop
        from rl_replicas_amd.ops import fused_rollout as fr
        from rl_replicas_amd.ops.fused_mlp import _extract_layers

        if not isinstance(policy, nn.Module) or not hasattr(policy, "network"):
            return None
        if kind == "pendulum":
            mode = fr.pendulum_eval_mode(policy)
            if mode is None:
                return None
            if mode == fr.EVAL_GAUSSIAN and policy.log_std.numel() != 1:
                return None
            in_dim, out_dim = 3, 1
        else:
            if fop._policy_kind(policy) != "categorical":
                return None
            mlp = fop._mlp_of(policy)
            if mlp is None or _extract_layers(mlp) is None:
                return None
            mode, in_dim, out_dim = "categorical", 4, 2
        weights, _, _ = _extract_layers(fop._mlp_of(policy))
        if int(weights[0].shape[1]) != in_dim or int(weights[-1].shape[0]) != out_dim:
            return None
        return mode

    # -- private state ------------------------------------------------------
    def _private_env(self, kind: str, num_episodes: int, horizon: int, device):
        from rl_replicas_amd.envs.device import DeviceCartPoleEnv, DevicePendulumEnv

        key = (kind, num_episodes, horizon, str(device))
        env = self._envs.get(key)
        if env is None:
            cls = DevicePendulumEnv if kind == "pendulum" else DeviceCartPoleEnv
            env = cls(num_episodes, device=device, max_episode_steps=horizon)
            env.seed(self.seed)
            self._envs[key] = env
        return env

    def _device_counters(self, device):
        from rl_replicas_amd.ops import fused_rollout as fr

        key = str(device)
        if key not in self._counters:
            self._counters[key] = (fr.make_counter(device), fr.make_counter(device))
        return self._counters[key]

    # -- entry point --------------------------------------------------------
    def evaluate(self, policy: Policy, env, num_episodes: int) -> Tuple[List[float], List[int]]:
        import torch

        from rl_replicas_amd import ops
        from rl_replicas_amd.ops import fused_onpolicy as fop

        kind = self._env_kind(env)
        horizon = getattr(getattr(env, "spec", None), "max_episode_steps", None)
        mode = self._policy_mode(policy, kind) if kind is not None and horizon else None
        device = None
        if mode is not None:
            def norm(d):  # "cuda" -> the current GPU's indexed device
                return torch.empty(0, device=d).device

            devices = {norm(p.device) for p in policy.parameters()}
            device = norm(self.device) if self.device is not None else next(iter(devices))
            env_device = getattr(env, "device", None)  # host envs have none
            if devices != {device} or (env_device is not None and norm(env_device) != device):
                mode = None  # a policy and an env on different devices
        if mode is None or num_episodes < 1:
            self.last_path = "host"
            self.last_initial_state = None
            return super().evaluate(policy, env, num_episodes)

        horizon = int(horizon)
        penv = self._private_env(kind, num_episodes, horizon, device)
        if device.type == "cuda" and ops.hip_available() and fop._graphs_common(None):
            key = (kind, mode, num_episodes, horizon, id(policy))
            entry = self._graphs.get(key)
            if entry is None and len(self._graphs) < self.MAX_GRAPHS:
                entry = (self._build_graph(kind, policy, penv, num_episodes, horizon,
                                           device), policy)
                self._graphs[key] = entry
            if entry is not None:
                graph = entry[0]
                graph.replay()
                self.last_path = "fused" if graph.fused else "graph"
                self.last_initial_state = graph.init_state
                return graph.returns.tolist(), graph.lengths.tolist()
        return self._evaluate_eager(kind, policy, penv, num_episodes, horizon)

    def _build_graph(self, kind: str, policy, penv, num_episodes: int, horizon: int,
                     device):
        from rl_replicas_amd.ops import fused_rollout as fr

        ctr, reset_ctr = self._device_counters(device)
        cls = fr.GraphedPendulumEval if kind == "pendulum" else fr.GraphedCartPoleEval
        with _on_device(device):
            return cls(policy, num_episodes, horizon, penv._philox_seed, ctr, reset_ctr,
                       advance_reset=self.seed is None)

    def _evaluate_eager(self, kind: str, policy, penv, num_episodes: int, horizon: int):
        import torch

        if self.seed is not None:
            penv.seed(self.seed)  # the same initial states on every call
        obs = penv.reset()
        dev = penv.device
        self.last_initial_state = penv.state.detach().clone()
        returns = torch.zeros(num_episodes, dtype=torch.float64, device=dev)
        lengths = torch.zeros(num_episodes, dtype=torch.int32, device=dev)
        finished = torch.zeros(num_episodes, dtype=torch.bool, device=dev)
        for _ in range(horizon):
            actions = policy.get_action_tensor(obs)
            obs, rewards, done, _ = penv.step(actions)
            if kind == "pendulum":  # lockstep: `done` is a host bool, true at the horizon
                returns += rewards.double()
                lengths += 1
            else:  # count each row's first episode only
                active = ~finished
                returns += torch.where(active, rewards.double(), torch.zeros_like(returns))
                lengths += active.to(torch.int32)
                finished |= done
        self.last_path = "eager"
        return returns.tolist(), lengths.tolist()


def _on_device(device):
    """Context that makes `device` the current GPU (graph capture allocates
    streams and buffers on the current device); a no-op on the CPU."""
    import contextlib

    import torch

    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
