"""Device-resident replay collection — the off-policy twin of DeviceSampler.

Pairs `envs.DevicePendulumEnv` or a synthetic `envs.DeviceVectorEnv` with one
`ReplayBuffer` on the same GPU.  An epoch of DDPG/TD3 collection (warm-up
`RandomPolicy` or the noised actor) is ONE captured hipGraph
(`ops/fused_rollout.py::GraphedPendulumCollect` / `GraphedSyntheticCollect`)
that steps the env and writes every transition straight into the buffer's
HBM ring at the write position the buffer holds on the device.  Nothing is
staged, transposed or copied a second time; the only read-back of an epoch
is the per-episode returns for the metrics layer.

The Pendulum env carries its fp64 `state` in place.  `DeviceVectorEnv`
replaces `env.state` with a fresh tensor on every eager step, so there the
graph owns a stable carry buffer: `sample()` copies the live state into it
before the replay when that is another tensor, and points `env.state` at it
afterwards.

The returned `Experience` carries the episode structure (`episode_returns`,
`episode_lengths`, `dones`, as `DeviceSampler._build_experience` orders
them), no flat cache, and `stored_in_buffer`: the buffer that already holds
its transitions.  `ReplayBuffer.add_experience` returns at once for it, so
`OffPolicyAlgorithm.learn` runs unchanged.

Wherever the collect graph does not apply (CPU, graphs disabled, another
policy or env, more transitions than the ring holds, a full graph cache)
`sample()` is `DeviceSampler.sample()`: the experience then has a flat cache
and no marker, and `add_experience` stores it the usual way.  Both routes
move the same ring bookkeeping, so they can be mixed in any order.

No reference counterpart (the reference samples one env serially on the
host, batch_sampler.py:55-99).
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import numpy as np

from rl_replicas_amd.envs.device import DevicePendulumEnv, DeviceVectorEnv
from rl_replicas_amd.experience import Experience
from rl_replicas_amd.policies import Policy
from rl_replicas_amd.replay_buffer import ReplayBuffer
from rl_replicas_amd.samplers.device_sampler import (
    DeviceSampler,
    cached_graph,
    lockstep_cuts,
    segment_bounds,
)


class DeviceReplaySampler(DeviceSampler):
    def __init__(self, device_env: Union[DevicePendulumEnv, DeviceVectorEnv],
                 replay_buffer: ReplayBuffer, seed: Optional[int] = None):
        super().__init__(device_env, seed=seed, is_continuous=True)
        buffer_device = replay_buffer.device
        if device_env.device.type == "cuda" and (
            buffer_device is None or buffer_device.type != "cuda"
        ):
            raise ValueError(
                "DeviceReplaySampler needs its ReplayBuffer on the env's device "
                f"({device_env.device}), got {buffer_device}"
            )
        self.replay_buffer = replay_buffer

    def sample(self, num_samples: int, policy: Policy) -> Experience:
        from rl_replicas_amd.ops import fused_rollout

        env = self.env
        N = self.num_envs
        buffer = self.replay_buffer
        synthetic = isinstance(env, DeviceVectorEnv)
        if synthetic:
            supported, mode_of, graph_cls = (
                fused_rollout.synthetic_collect_supported,
                fused_rollout.synthetic_collect_mode,
                fused_rollout.GraphedSyntheticCollect)
        else:
            supported, mode_of, graph_cls = (
                fused_rollout.pendulum_collect_supported,
                fused_rollout.pendulum_collect_mode,
                fused_rollout.GraphedPendulumCollect)
        if (num_samples % N != 0 or num_samples > buffer.buffer_size
                or not supported(policy, env, buffer)):
            return super().sample(num_samples, policy)
        steps = num_samples // N
        first = self._obs is None
        horizon = env.spec.max_episode_steps
        start_elapsed = 0 if first else env._elapsed
        cuts = lockstep_cuts(steps, horizon, start_elapsed)
        mode = mode_of(policy, env)
        key = (steps, cuts, first, mode)
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= 8:  # the cache cap of DeviceSampler
                return super().sample(num_samples, policy)
            if first and self.seed is not None:
                env.seed(self.seed)
            g = cached_graph(
                self, key,
                lambda ctr: graph_cls(
                    policy, env, buffer, steps, cuts, first, mode, ctr),
            )
        if synthetic:
            # the live state into the graph's carry (nothing to do when the
            # previous epoch was this graph's)
            if not first and self._obs is not g.carry:
                g.carry.copy_(self._obs)
            g.replay()
            self._obs = env.state = g.carry
        else:
            g.replay()
            self._obs = g.last_obs
        env._elapsed = steps - (cuts[-1] + 1) if cuts else start_elapsed + steps
        return self._build_marked_experience(steps, cuts, g.seg_returns)

    def _build_marked_experience(self, steps: int, cuts: Tuple[int, ...],
                                 seg_returns) -> Experience:
        N = self.num_envs
        bounds = segment_bounds(steps, cuts)  # as in DeviceSampler._build_experience
        experience = Experience()
        # one tiny D2H: per-episode returns for the metrics layer
        experience.episode_returns = [
            float(r) for r in seg_returns.cpu().numpy().reshape(-1)
        ]
        experience.episode_lengths = [e - s for s, e, _ in bounds] * N
        experience.dones = [
            np.concatenate([np.zeros(e - s - 1, dtype=bool), [done]])
            for s, e, done in bounds
        ] * N
        experience.stored_in_buffer = self.replay_buffer
        return experience
