"""GPU-resident vectorized synthetic environments.

The CPU `VectorEnv` path steps numpy dynamics on the host, which makes
every rollout step pay a D2H (actions) + H2D (observations) round trip
plus host arithmetic.  For the synthetic MuJoCo-shaped benchmark envs
(`envs/synthetic.py`) the dynamics are a few small matmuls — exactly
the kind of work the GPU does for free next to the policy forward — so
this module keeps the *entire* environment state in HBM (Isaac-Gym
style): policy forward, Philox action sampling, env transition and
reward all run on device and the epoch's rollout never touches the
host.

Semantics match `SyntheticEnv`/`VectorEnv` (same dynamics matrices —
they are taken from the registered numpy env — same tanh/clip/reward
formulas, same 1000-step horizon with autoreset); only the RNG streams
differ (torch Philox here vs numpy PCG64 there), which is the same
freedom the reference has across gymnasium versions.  Episodes advance
in lockstep: every instance resets together, so truncation boundaries
are host-known arithmetic and episode slicing costs nothing.

No reference counterpart (the reference steps ONE gymnasium env on the
CPU, batch_sampler.py:55-99); this is MI355X-first design, validated
against the numpy env in tests/test_device_env.py.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .core import make
from .synthetic import SyntheticEnv


class DeviceVectorEnv:
    """N synthetic env instances as device tensors, stepped in lockstep.

    s' = tanh(s A + clip(a) B + noise*eps);  r = <s', w> - 0.1|a|^2
    (identical to SyntheticEnv._step_b, synthetic.py:72-78).
    """

    def __init__(self, env: str, num_envs: int, device="cpu", **make_kwargs):
        base = make(env, **make_kwargs)
        if not isinstance(base, SyntheticEnv):
            raise TypeError(
                f"DeviceVectorEnv supports the synthetic benchmark envs (got {type(base).__name__})"
            )
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.observation_space = base.observation_space
        self.action_space = base.action_space
        self.spec = base.spec
        self.noise = float(base.noise)
        # identical dynamics to the numpy env (same seed-derived matrices)
        self.A = torch.from_numpy(base.A).to(self.device)
        self.B = torch.from_numpy(base.B).to(self.device)
        self.w = torch.from_numpy(base.w).to(self.device)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
        self.state: Optional[Tensor] = None
        self._elapsed = 0  # lockstep: one counter for all instances
        # HIP fast path RNG: Philox keyed (seed ^ salt, offset).  The salt
        # decorrelates the env stream from the policy's action-sampling
        # stream, which is keyed on the same torch seed.
        self._philox_seed = (torch.initial_seed() ^ 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
        self._philox_offset = 0

    def seed(self, seed: Optional[int]) -> None:
        if seed is not None:
            self._gen.manual_seed(int(seed))
            self._philox_seed = (int(seed) ^ 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
            self._philox_offset = 0
            self.action_space.seed(seed + 1000)  # VectorEnv.seed contract

    def _wants_hip(self) -> bool:
        from rl_replicas_amd import ops

        return self.device.type == "cuda" and ops.wants_hip(
            self.state if self.state is not None else self.A
        )

    def _init_state(self) -> Tensor:
        return 0.1 * torch.randn(
            self.num_envs, self.A.shape[0], generator=self._gen, device=self.device
        )

    def reset(self, *, seed: Optional[int] = None) -> Tensor:
        if seed is not None:
            self.seed(seed)
        if self._wants_hip():
            from rl_replicas_amd import ops

            ext = ops._load_extension()
            self.state = ext.synthetic_env_reset(
                self.num_envs, self.A.shape[0], self.A,
                self._philox_seed, self._philox_offset,
            )
            self._philox_offset += 1
        else:
            self.state = self._init_state()
        self._elapsed = 0
        return self.state

    def step(self, actions: Tensor) -> Tuple[Tensor, Tensor, bool, Tensor]:
        """-> (obs [N,O], reward [N], truncated: host bool, final_obs [N,O]).

        `truncated` is a scalar (lockstep horizon; synthetic envs never
        terminate early).  On truncation all instances autoreset; `obs`
        is post-reset, `final_obs` the true successor (GAE bootstrap).
        """
        self._elapsed += 1
        truncated = (
            self.spec.max_episode_steps is not None
            and self._elapsed >= self.spec.max_episode_steps
        )
        if self._wants_hip():
            from rl_replicas_amd import ops

            ext = ops._load_extension()
            # ONE kernel: clip + sA + aB + Philox noise + tanh + reward
            # (+ the autoreset init states on lockstep horizon boundaries)
            state, reward, final_obs = ext.synthetic_env_step(
                self.state, actions.contiguous(), self.A, self.B, self.w,
                self.noise, self._philox_seed, self._philox_offset, truncated,
            )
            self._philox_offset += 2
        else:
            a = actions.clamp(-1.0, 1.0)
            eps = torch.randn(
                self.num_envs, self.A.shape[0], generator=self._gen, device=self.device
            )
            state = torch.tanh(
                torch.addmm(self.noise * eps, self.state, self.A).addmm_(a, self.B)
            )
            reward = state @ self.w - 0.1 * (a * a).sum(dim=1)
            final_obs = state
            if truncated:
                state = self._init_state()
        if truncated:
            self._elapsed = 0
        self.state = state
        return state, reward, truncated, final_obs

    def close(self) -> None:
        pass


class DevicePendulumEnv:
    """Pendulum-v1 as a lockstep device vector env.  Dynamics/reward
    formulas match `classic.PendulumEnv` exactly (fp64 state, fp32 obs).
    Pendulum never terminates early, so the lockstep-truncation contract of
    `DeviceSampler` holds.

    On GPU with the extension, `state` is ONE fp64 [N,2] tensor (theta,
    theta_dot) updated in place, and `step`/`reset` are one kernel each
    (`pendulum_env_step` / `pendulum_env_reset`, env_kernels.hip), so
    captured graphs and the persistent rollout kernel
    (`ops/fused_rollout.py::GraphedPendulumRollout`) read and write the same
    storage the eager path uses.  Assigning `env.state = t` there copies into
    that storage.  On the CPU the same arithmetic runs as torch fp64 ops.

    Only the init-state RNG stream differs from the numpy env, and it is not
    the same stream on both devices: Philox keyed by (`_philox_seed`,
    `_philox_offset`, row) on the GPU, the torch generator on the CPU -- the
    freedom the module docstring grants.  A GPU run seeded as before the
    env had kernels therefore starts from other init states.
    """

    def __init__(self, num_envs: int, device="cpu", max_episode_steps: Optional[int] = 200):
        from .classic import PendulumEnv
        from .core import EnvSpec

        base = PendulumEnv()
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.observation_space = base.observation_space
        self.action_space = base.action_space
        self.spec = EnvSpec("Pendulum-v1", max_episode_steps=max_episode_steps)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
        # [N, 2] float64: theta, theta_dot.  GPU: allocated once, in place
        self._state: Optional[Tensor] = None
        if self.device.type == "cuda":
            self._state = torch.zeros(self.num_envs, 2, dtype=torch.float64,
                                      device=self.device)
        self._elapsed = 0
        # same salt as DeviceVectorEnv: decorrelates the env stream from the
        # policy's action-sampling stream keyed on the same torch seed
        self._philox_seed = (torch.initial_seed() ^ 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
        self._philox_offset = 0

    @property
    def state(self) -> Optional[Tensor]:
        return self._state

    @state.setter
    def state(self, value: Optional[Tensor]) -> None:
        if self._state is not None and self._state.is_cuda and value is not None:
            self._state.copy_(value)  # graphs hold this storage
        else:
            self._state = value

    def seed(self, seed: Optional[int]) -> None:
        if seed is not None:
            self._gen.manual_seed(int(seed))
            self._philox_seed = (int(seed) ^ 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
            self._philox_offset = 0
            self.action_space.seed(seed + 1000)

    def _wants_hip(self) -> bool:
        from rl_replicas_amd import ops

        return self.device.type == "cuda" and ops.wants_hip(self._state)

    def _init_state(self) -> Tensor:
        u = torch.rand(self.num_envs, 2, generator=self._gen, device=self.device,
                       dtype=torch.float64)
        import math

        return (2.0 * u - 1.0) * torch.tensor([math.pi, 1.0], device=self.device,
                                              dtype=torch.float64)

    def _obs(self) -> Tensor:
        if self._wants_hip():
            from rl_replicas_amd import ops

            return ops._load_extension().pendulum_env_reset(self._state, 0, 0, draw=False)
        th, thdot = self.state[:, 0], self.state[:, 1]
        return torch.stack([torch.cos(th), torch.sin(th), thdot], dim=1).float()

    def reset(self, *, seed: Optional[int] = None) -> Tensor:
        if seed is not None:
            self.seed(seed)
        self._elapsed = 0
        if self._wants_hip():
            from rl_replicas_amd import ops

            obs = ops._load_extension().pendulum_env_reset(
                self._state, self._philox_seed, self._philox_offset
            )
            self._philox_offset += 1
            return obs
        self.state = self._init_state()
        return self._obs()

    def step(self, actions: Tensor) -> Tuple[Tensor, Tensor, bool, Tensor]:
        """-> (obs [N,3], reward [N], truncated: host bool, final_obs [N,3]).

        On truncation all instances autoreset; `obs` is post-reset,
        `final_obs` the true successor (GAE bootstrap)."""
        if self._wants_hip():
            from rl_replicas_amd import ops

            self._elapsed += 1
            truncated = (
                self.spec.max_episode_steps is not None
                and self._elapsed >= self.spec.max_episode_steps
            )
            # ONE kernel: clamp + cost + Euler step (+ the autoreset draw on
            # the lockstep horizon step) + the fp32 observations
            obs, reward, final_obs = ops._load_extension().pendulum_env_step(
                self._state,
                actions.to(device=self.device, dtype=torch.float32)
                .reshape(self.num_envs, -1)[:, :1].contiguous(),
                truncated, self._philox_seed, self._philox_offset,
            )
            self._philox_offset += 1
            if truncated:
                self._elapsed = 0
            return obs, reward, truncated, final_obs

        import math

        th, thdot = self.state[:, 0], self.state[:, 1]
        u = actions.to(torch.float64).reshape(self.num_envs, -1)[:, 0].clamp(-2.0, 2.0)
        ang = torch.remainder(th + math.pi, 2 * math.pi) - math.pi
        costs = ang * ang + 0.1 * thdot * thdot + 0.001 * u * u
        newthdot = (thdot + (15.0 * torch.sin(th) + 3.0 * u) * 0.05).clamp(-8.0, 8.0)
        newth = th + newthdot * 0.05
        self.state = torch.stack([newth, newthdot], dim=1)
        self._elapsed += 1
        truncated = (
            self.spec.max_episode_steps is not None
            and self._elapsed >= self.spec.max_episode_steps
        )
        final_obs = self._obs()
        obs = final_obs
        if truncated:
            self.state = self._init_state()
            self._elapsed = 0
            obs = self._obs()
        reward = (-costs).float()
        return obs, reward, truncated, final_obs

    def close(self) -> None:
        pass


class DeviceCartPoleEnv:
    """CartPole-v1 as N device-resident instances with PER-INSTANCE
    termination, truncation and autoreset (`VectorEnv.step` semantics).

    Unlike the lockstep envs above, `step` returns a `done` TENSOR: episode
    boundaries are data.  The carry is public and updated in place —
    `state` fp64 [N,4] (x, x_dot, theta, theta_dot; the host env keeps fp64
    state and casts to fp32 only for the observation) and `elapsed` int32
    [N] — so captured graphs and the persistent rollout kernel
    (`ops/fused_rollout.py::GraphedCartPoleRollout`) read and write the
    same storage the eager path uses.

    On GPU with the extension, `step`/`reset` are one kernel each
    (`cartpole_env_step` / `cartpole_env_reset`, env_kernels.hip); otherwise
    the same arithmetic runs as torch fp64 ops.  Dynamics follow
    `classic.CartPoleEnv._step_b` (constants, expression order); only the
    init-state RNG stream differs (Philox / torch generator vs numpy).
    """

    def __init__(self, num_envs: int, device="cpu", max_episode_steps: Optional[int] = 500):
        from .classic import CartPoleEnv
        from .core import EnvSpec

        base = CartPoleEnv()
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.observation_space = base.observation_space
        self.action_space = base.action_space
        self.spec = EnvSpec("CartPole-v1", max_episode_steps=max_episode_steps)
        self.state = torch.zeros(self.num_envs, 4, dtype=torch.float64, device=self.device)
        self.elapsed = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
        # same salt as DeviceVectorEnv: decorrelates the env stream from the
        # policy's action-sampling stream keyed on the same torch seed
        self._philox_seed = (torch.initial_seed() ^ 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
        self._philox_offset = 0

    @property
    def max_steps(self) -> int:
        """Kernel-side horizon (0: no truncation)."""
        return int(self.spec.max_episode_steps or 0)

    def seed(self, seed: Optional[int]) -> None:
        if seed is not None:
            self._gen.manual_seed(int(seed))
            self._philox_seed = (int(seed) ^ 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
            self._philox_offset = 0
            self.action_space.seed(seed + 1000)  # VectorEnv.seed contract

    def _wants_hip(self) -> bool:
        from rl_replicas_amd import ops

        return self.device.type == "cuda" and ops.wants_hip(self.state)

    def _init_state(self) -> Tensor:
        # the kernel's formula on a torch-generator uniform: strictly
        # inside (-0.05, 0.05)
        u = torch.rand(self.num_envs, 4, generator=self._gen, device=self.device,
                       dtype=torch.float64)
        r = torch.floor(u * 4294967296.0)
        return -0.05 + 0.1 * ((r + 0.5) * (1.0 / 4294967296.0))

    def reset(self, *, seed: Optional[int] = None) -> Tensor:
        if seed is not None:
            self.seed(seed)
        if self._wants_hip():
            from rl_replicas_amd import ops

            obs = ops._load_extension().cartpole_env_reset(
                self.state, self.elapsed, self._philox_seed, self._philox_offset
            )
            self._philox_offset += 1
            return obs
        self.state.copy_(self._init_state())
        self.elapsed.zero_()
        return self.state.float()

    def step(self, actions: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """-> (obs [N,4], reward [N], done [N] bool, final_obs [N,4]).

        `obs` is post-autoreset, `final_obs` the true successor (GAE
        bootstrap); `done = terminated | truncated` per instance."""
        if self._wants_hip():
            from rl_replicas_amd import ops

            obs, reward, done, final_obs = ops._load_extension().cartpole_env_step(
                self.state, self.elapsed,
                actions.reshape(-1).to(torch.int64).contiguous(), self.max_steps,
                self._philox_seed, self._philox_offset,
            )
            self._philox_offset += 1
            return obs, reward, done.bool(), final_obs

        import math

        x, x_dot, theta, theta_dot = self.state.unbind(dim=1)
        force = torch.where(actions.reshape(-1).to(self.device) == 1, 10.0, -10.0).to(torch.float64)
        total_mass = 1.0 + 0.1
        polemass_length = 0.1 * 0.5
        costheta = torch.cos(theta)
        sintheta = torch.sin(theta)
        temp = (force + polemass_length * (theta_dot * theta_dot) * sintheta) / total_mass
        thetaacc = (9.8 * sintheta - costheta * temp) / (
            0.5 * (4.0 / 3.0 - 0.1 * (costheta * costheta) / total_mass)
        )
        xacc = temp - polemass_length * thetaacc * costheta / total_mass
        x = x + 0.02 * x_dot
        x_dot = x_dot + 0.02 * xacc
        theta = theta + 0.02 * theta_dot
        theta_dot = theta_dot + 0.02 * thetaacc
        new = torch.stack([x, x_dot, theta, theta_dot], dim=1)
        terminated = (x.abs() > 2.4) | (theta.abs() > 12 * 2 * math.pi / 360)
        elapsed = self.elapsed + 1
        if self.spec.max_episode_steps is not None:
            truncated = (elapsed >= self.spec.max_episode_steps) & ~terminated
        else:
            truncated = torch.zeros_like(terminated)
        done = terminated | truncated
        final_obs = new.float()
        # every row draws (no host sync on `done.any()`); done rows keep it
        self.state.copy_(torch.where(done[:, None], self._init_state(), new))
        self.elapsed.copy_(torch.where(done, torch.zeros_like(elapsed), elapsed))
        reward = torch.ones(self.num_envs, dtype=torch.float32, device=self.device)
        return self.state.float(), reward, done, final_obs

    def close(self) -> None:
        pass
