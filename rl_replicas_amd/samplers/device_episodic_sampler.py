"""Device-resident rollout sampler for envs that end episodes PER INSTANCE.

`DeviceSampler` serves the lockstep envs, whose truncation boundaries are
host arithmetic.  An env such as `envs.DeviceCartPoleEnv` terminates each
instance on its own, so here the episode boundaries are DATA: the rollout
records a `[steps, N]` done mask on the device, and one readback of that
mask per epoch (steps * N bytes) gives the host everything it needs to
slice episodes with numpy boundary searches.  Observations, actions,
rewards and bootstrap observations never leave HBM; the flat batch handed
to the algorithms (`Experience.set_flat_cache`) is made of device tensors
with the keys `DeviceSampler` emits.

The sampler drives any device env whose `step(actions)` returns
`(obs, reward, done[N], final_obs)`.  With a `CategoricalPolicy` over an
MLP on a GPU `DeviceCartPoleEnv` the whole epoch is one captured graph
(`ops/fused_rollout.py::GraphedCartPoleRollout`); otherwise an eager loop
issues the same steps.

Episode semantics are `VectorSampler`'s: instance-major episode order, a
`done` episode bootstraps from `final_obs`, an epoch-end cut has
`done=False` and bootstraps from the live observation, `is_continuous`
retains env state across calls, the env is seeded on the first reset only.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from rl_replicas_amd.experience import Experience
from rl_replicas_amd.policies import Policy
from rl_replicas_amd.samplers.device_sampler import cached_graph
from rl_replicas_amd.samplers.sampler import Sampler


class DeviceEpisodicSampler(Sampler):
    def __init__(self, device_env, seed: Optional[int] = None, is_continuous: bool = False):
        self.env = device_env
        self.seed = seed
        self.is_continuous = is_continuous
        self.num_envs = device_env.num_envs
        self._obs: Optional[torch.Tensor] = None
        self._bufs = None  # eager-path buffers, reused across epochs
        self._graphs = {}
        self._graph_ctr: Optional[torch.Tensor] = None

    def sample(self, num_samples: int, policy: Policy) -> Experience:
        N = self.num_envs
        if num_samples % N != 0:
            raise ValueError(
                f"num_samples ({num_samples}) must be divisible by num_envs ({N})"
            )
        steps = num_samples // N
        first = self._obs is None
        reset_epoch = first or not self.is_continuous

        from rl_replicas_amd.ops import fused_rollout

        if fused_rollout.cartpole_supported(policy, self.env):
            if first and self.seed is not None:
                self.env.seed(self.seed)
            bufs = self._sample_graphed(policy, steps, reset_epoch)
        else:
            bufs = self._sample_eager(policy, steps, first, reset_epoch)
        return self._build_experience(steps, *bufs)

    # ------------------------------------------------------------------
    def _sample_graphed(self, policy, steps: int, reset_epoch: bool):
        from rl_replicas_amd.ops import fused_rollout

        g = cached_graph(
            self, (steps, reset_epoch),
            lambda ctr: fused_rollout.GraphedCartPoleRollout(
                policy, self.env, steps, reset_epoch, ctr),
        )
        # the carry (env.state / env.elapsed) is read and written in place
        g.replay()
        self._obs = g.obs_full[steps]
        return g.obs_full[:steps], g.act_buf, g.rew_buf, g.done_buf, g.final_obs

    # ------------------------------------------------------------------
    def _sample_eager(self, policy, steps: int, first: bool, reset_epoch: bool):
        env = self.env
        if first:
            self._obs = env.reset(seed=self.seed)
        elif reset_epoch:
            self._obs = env.reset()
        obs = self._obs
        N = self.num_envs
        dev = obs.device
        for t in range(steps):
            actions = policy.get_action_tensor(obs).to(dev)
            if self._bufs is None or self._bufs[0].shape[0] != steps:
                self._bufs = (
                    torch.empty(steps, *obs.shape, device=dev),
                    torch.empty(steps, *actions.shape, dtype=actions.dtype, device=dev),
                    torch.empty(steps, N, device=dev),
                    torch.empty(steps, N, dtype=torch.uint8, device=dev),
                    torch.empty(steps, *obs.shape, device=dev),
                )
            obs_buf, act_buf, rew_buf, done_buf, final_buf = self._bufs
            obs_buf[t].copy_(obs)
            act_buf[t].copy_(actions)
            obs, reward, done, final_obs = env.step(actions)
            rew_buf[t].copy_(reward)
            done_buf[t].copy_(done)
            final_buf[t].copy_(final_obs)
        self._obs = obs
        return self._bufs

    # ------------------------------------------------------------------
    def _build_experience(self, steps: int, obs_buf, act_buf, rew_buf, done_buf,
                          final_buf) -> Experience:
        N = self.num_envs
        T = N * steps
        device = obs_buf.device
        live = self._obs

        # flat (instance-major) device views for the train pipeline
        def flat(buf):
            out = torch.empty(T, *buf.shape[2:], dtype=buf.dtype, device=device)
            out.view(N, steps, *buf.shape[2:]).copy_(buf.transpose(0, 1))
            return out

        flat_obs, flat_act, flat_rew = flat(obs_buf), flat(act_buf), flat(rew_buf)
        flat_final, flat_done = flat(final_buf), flat(done_buf)

        # per-step successors (the replay-buffer view): the next stored
        # observation, the live one after the last step, and the TRUE
        # pre-reset successor on done steps
        flat_next = torch.empty_like(flat_obs)
        nv = flat_next.view(N, steps, *flat_obs.shape[1:])
        if steps > 1:
            nv[:, : steps - 1].copy_(obs_buf[1:].transpose(0, 1))
        nv[:, steps - 1].copy_(live)
        done_b = flat_done.bool()
        flat_next = torch.where(
            done_b.view(T, *([1] * (flat_obs.dim() - 1))), flat_final, flat_next
        )

        # the epoch's ONE boundary readback: steps * N bytes (queued behind
        # the device-only copies above, so they overlap the host work below)
        done_flat = flat_done.cpu().numpy().astype(bool)
        # an episode ends at every done step and at each instance's last step
        ends_mask = done_flat.copy()
        ends_mask[steps - 1 :: steps] = True
        ends = np.flatnonzero(ends_mask)  # flat (instance-major) row of each end
        offsets_np = np.zeros(len(ends) + 1, dtype=np.int32)
        offsets_np[1:] = ends + 1
        ep_dones = done_flat[ends]
        lengths = np.diff(offsets_np)

        # bootstrap observations: one gather over [final_obs rows | live rows]
        gather_np = np.where(ep_dones, ends, T + ends // steps)
        last_obs = torch.cat([flat_final, live], dim=0).index_select(
            0, torch.as_tensor(gather_np, dtype=torch.int64, device=device)
        )

        # per-episode returns: device segment sum (each row's episode index
        # by binary search over the offsets), one small D2H
        offsets_t = torch.as_tensor(offsets_np, device=device)
        ep_of_row = torch.searchsorted(
            offsets_t[1:], torch.arange(T, dtype=torch.int32, device=device), right=True
        )
        ep_returns = torch.zeros(len(ends), device=device).index_add_(
            0, ep_of_row, flat_rew
        ).cpu().numpy()

        experience = Experience()
        experience.episode_returns = [float(r) for r in ep_returns]
        experience.episode_lengths = [int(L) for L in lengths]
        experience.dones = np.split(done_flat, offsets_np[1:-1])
        experience.set_flat_cache(
            {
                "observations": flat_obs,
                "actions": flat_act,
                "rewards": flat_rew,
                "episode_offsets": offsets_t,
                "episode_dones": torch.as_tensor(ep_dones, device=device),
                "last_observations": last_obs,
                "next_observations": flat_next,
                "step_dones": done_b.float(),
            }
        )
        return experience
