"""hipGraph-captured device rollout (DeviceSampler fast path).

The eager device rollout issues 3 kernels per env step (fused MLP
forward, Philox action sample, fused env transition) — at 20 steps per
epoch that is ~60 host launches of ~3.5 us each.  Here the WHOLE epoch
rollout (optional lockstep reset / state carry, then steps x
[forward -> sample -> env step], then one RNG-counter bump) is captured
once and replayed as a single hipGraph per epoch.

For the flagship shape (fp32, widths and obs dim <= 64) the 3 x steps
kernels of that graph are ONE persistent kernel (`ppo_rollout_fused`):
each workgroup carries 16 env rows through every step with weights and
state in LDS, using the same device functions, Philox offsets and
element indices as the three kernels, so the buffers hold the same bytes
(`fused_kernel_eligible`; RL_REPLICAS_AMD_ROLLOUT_FUSED=0 keeps the
three-kernel body).

Randomness across replays: by-value Philox offsets are frozen at
capture, so every RNG kernel adds a device-resident int64 counter
(`offset_ctr`) to its offset; the graph's last node advances the
counter past every offset used, so each replay draws a fresh,
deterministic slice of the stream (same seed => bitwise-identical run,
tests/test_gpu_train.py::test_graphed_rollout_determinism).

Weights/log_std are read by pointer, so the Adam updates between
epochs are visible to the next replay without re-capture.  Re-capture
happens only when the epoch's lockstep-truncation pattern changes
(bounded: the horizon/steps arithmetic cycles through at most two
patterns when horizon % steps == 0, the benchmark shape).

`GraphedCartPoleRollout` is the same construction for a
CategoricalPolicy on `DeviceCartPoleEnv` (DeviceEpisodicSampler fast
path): termination, truncation and autoreset are decided in-kernel per
instance, so there are no cut patterns, and the persistent kernel is
`cartpole_rollout_fused` (`cartpole_fused_eligible`).

`GraphedPendulumRollout` is the construction for a GaussianPolicy on
`DevicePendulumEnv` (DeviceSampler): lockstep like the synthetic envs, so
graphs are keyed by the cut pattern, but the carry is the env's own fp64
`state` as with CartPole; the persistent kernel is
`pendulum_rollout_fused` (`pendulum_fused_eligible`).

No reference counterpart (the reference samples one env serially on
the host, batch_sampler.py:55-99).
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from rl_replicas_amd import ops
from rl_replicas_amd.ops import fused_onpolicy as fop
from rl_replicas_amd.ops.fused_mlp import _extract_layers


def supported(policy, env) -> bool:
    from rl_replicas_amd.envs.device import DeviceVectorEnv

    if not (env.device.type == "cuda" and ops.hip_available()
            and isinstance(env, DeviceVectorEnv)  # synthetic-dynamics kernels
            and fop._graphs_common(None)
            and fop._policy_kind(policy) == "gaussian"):
        return False
    mlp = fop._mlp_of(policy)
    return mlp is not None and _extract_layers(mlp) is not None


def fused_kernel_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """Whether the epoch runs as ONE persistent kernel (ppo_rollout_fused,
    rollout_fused_kernels.hip) instead of steps x 3 kernels: fp32 compute,
    a Gaussian policy without action clipping (the only kind `supported`
    admits), every width and the obs dim <= 64, and the net + env image
    within the kernel's LDS budget.  RL_REPLICAS_AMD_ROLLOUT_FUSED=0
    selects the three-kernel body."""
    import os

    if os.environ.get("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1") == "0":
        return False
    if ops.compute_bf16() != 0:
        return False
    ext = ops._load_extension()
    weights, _, _ = _extract_layers(fop._mlp_of(policy))
    O, A = int(env.A.shape[0]), int(env.B.shape[0])
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    # the binding's own limits (common.h), so gate and TORCH_CHECKs agree
    max_layers, max_width, max_cuts, max_lds = ext.ppo_rollout_fused_limits()
    if (len(weights) > max_layers or max(dims) > max_width or dims[0] != O
            or dims[-1] != A or policy.log_std.numel() != A
            or len(cuts) > max_cuts):
        return False
    if any(t.dtype != torch.float32 for t in (*weights, policy.log_std)):
        return False
    return ext.ppo_rollout_fused_lds_bytes(dims, O, A) <= max_lds


def make_counter(device) -> torch.Tensor:
    """Device RNG counter; base 2^40 keeps the graph streams clear of the
    host-side offsets the eager paths use under the same seeds."""
    return torch.full((1,), 1 << 40, dtype=torch.int64, device=device)


class GraphedRollout:
    """One captured epoch: [reset | state carry] + steps x (mlp_forward ->
    gaussian_sample -> synthetic_env_step) + counter bump; or, when
    `fused_kernel_eligible`, ppo_rollout_fused + counter bump."""

    def __init__(self, policy, env, steps: int, cuts: Tuple[int, ...],
                 start_with_reset: bool, ctr: torch.Tensor):
        ext = ops._load_extension()
        N, O, A = env.num_envs, int(env.A.shape[0]), int(env.B.shape[0])
        dev = env.device
        self.env = env
        self.steps = steps
        self.cuts = list(cuts)
        self.start_with_reset = start_with_reset
        # zeros (not empty): capture warmup runs the MLP on these buffers
        # before the first real state lands in the carry slot
        self.obs_full = torch.zeros(steps + 1, N, O, device=dev)
        self.act_buf = torch.zeros(steps, N, A, device=dev)
        self.rew_buf = torch.zeros(steps, N, device=dev)
        self.cut_final = torch.zeros(max(len(cuts), 1), N, O, device=dev)
        # shared across all of a sampler's graphs so truncation-pattern
        # switches never reuse (seed, offset) pairs
        self.ctr = ctr
        policy_seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF
        env_seed = env._philox_seed
        weights, biases, acts = _extract_layers(fop._mlp_of(policy))
        log_std = policy.log_std
        cset = {c: j for j, c in enumerate(cuts)}
        compute_bf16 = ops.compute_bf16()

        self.fused = fused_kernel_eligible(policy, env, cuts)

        def body_fused():
            # 2 nodes: the persistent kernel carries every 16-row tile
            # through all steps; it reads ctr once and the bump follows
            ext.ppo_rollout_fused(
                list(weights), list(biases), acts, log_std.data, env.A, env.B,
                env.w, env.noise, policy_seed, env_seed, list(cuts),
                start_with_reset, self.ctr, self.obs_full, self.act_buf,
                self.rew_buf, self.cut_final,
            )
            ext.counter_add_(self.ctr, 2 * steps + 1)

        def body():
            if start_with_reset:
                ext.synthetic_env_reset(N, O, env.A, env_seed, 2 * steps,
                                        self.ctr, self.obs_full[0])
            else:
                self.obs_full[0].copy_(self.obs_full[steps])
            for t in range(steps):
                mean = ext.mlp_forward(self.obs_full[t], list(weights),
                                       list(biases), acts, False, compute_bf16)[0]
                ext.gaussian_sample(mean, log_std.data, policy_seed, t, -1.0,
                                    -1.0, self.ctr, self.act_buf[t])
                do_reset = t in cset
                ext.synthetic_env_step(
                    self.obs_full[t], self.act_buf[t], env.A, env.B, env.w,
                    env.noise, env_seed, 2 * t, do_reset, self.ctr,
                    self.obs_full[t + 1],
                    self.cut_final[cset[t]] if do_reset else self.obs_full[t + 1],
                    self.rew_buf[t],
                )
            # past every offset used: env 2t/2t+1 (t<steps), reset 2*steps,
            # policy t (t<steps)
            ext.counter_add_(self.ctr, 2 * steps + 1)

        # warmup advances ctr (and the state carry buffer); snapshot/restore
        # so the first replay starts exactly where the eager world left off
        state = [self.ctr] if start_with_reset else [self.ctr, self.obs_full]
        self.loop = fop._CapturedLoop(body_fused if self.fused else body, state)

    def replay(self) -> None:
        self.loop.replay()

    def final_tensors(self) -> List[torch.Tensor]:
        """Per-cut bootstrap observations, in cut order."""
        return [self.cut_final[j] for j in range(len(self.cuts))]


# ---------------------------------------------------------------------------
# Categorical policy on the device CartPole env (DeviceEpisodicSampler)
# ---------------------------------------------------------------------------
def cartpole_supported(policy, env) -> bool:
    """A CategoricalPolicy over an MLP on a GPU DeviceCartPoleEnv, with the
    extension present and graphs enabled."""
    from rl_replicas_amd.envs.device import DeviceCartPoleEnv

    if not (isinstance(env, DeviceCartPoleEnv) and env.device.type == "cuda"
            and ops.hip_available() and fop._graphs_common(None)
            and fop._policy_kind(policy) == "categorical"):
        return False
    mlp = fop._mlp_of(policy)
    return mlp is not None and _extract_layers(mlp) is not None


def cartpole_fused_eligible(policy, env) -> bool:
    """Whether the epoch runs as ONE persistent kernel (cartpole_rollout_fused,
    cartpole_rollout_kernels.hip) instead of steps x 3 kernels: fp32 compute,
    every width <= 64, the net image within the kernel's LDS budget.
    RL_REPLICAS_AMD_ROLLOUT_FUSED=0 selects the multi-kernel body."""
    import os

    if os.environ.get("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1") == "0":
        return False
    if ops.compute_bf16() != 0:
        return False
    ext = ops._load_extension()
    weights, _, _ = _extract_layers(fop._mlp_of(policy))
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    # the binding's own limits (common.h), so gate and TORCH_CHECKs agree
    max_layers, max_width, max_lds = ext.cartpole_rollout_fused_limits()
    if len(weights) > max_layers or max(dims) > max_width or dims[0] != 4:
        return False
    if any(w.dtype != torch.float32 for w in weights):
        return False
    return ext.cartpole_rollout_fused_lds_bytes(dims) <= max_lds


class GraphedCartPoleRollout:
    """One captured epoch on a DeviceCartPoleEnv: [cartpole_env_reset |
    nothing] + steps x (mlp_forward -> categorical_sample ->
    cartpole_env_step) + counter bump; or, when `cartpole_fused_eligible`,
    cartpole_rollout_fused + counter bump.

    Termination, truncation and autoreset are decided in-kernel, so there is
    one graph per (steps, start_with_reset) and no cut patterns.  The env's
    carry tensors (`env.state`, `env.elapsed`) are read and written in
    place.  Philox offsets (both bodies): policy sample and autoreset of
    step t at `t + ctr` (policy seed / env seed), epoch reset at
    `steps + ctr`; the last node advances the counter by steps + 1."""

    def __init__(self, policy, env, steps: int, start_with_reset: bool,
                 ctr: torch.Tensor):
        ext = ops._load_extension()
        N = env.num_envs
        dev = env.device
        self.env = env
        self.steps = steps
        self.start_with_reset = start_with_reset
        self.obs_full = torch.zeros(steps + 1, N, 4, device=dev)
        self.final_obs = torch.zeros(steps, N, 4, device=dev)
        self.act_buf = torch.zeros(steps, N, dtype=torch.int64, device=dev)
        self.rew_buf = torch.zeros(steps, N, device=dev)
        self.done_buf = torch.zeros(steps, N, dtype=torch.uint8, device=dev)
        self.ctr = ctr
        policy_seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF
        env_seed = env._philox_seed
        max_steps = env.max_steps
        weights, biases, acts = _extract_layers(fop._mlp_of(policy))
        compute_bf16 = ops.compute_bf16()

        self.fused = cartpole_fused_eligible(policy, env)

        def body_fused():
            ext.cartpole_rollout_fused(
                list(weights), list(biases), acts, policy_seed, env_seed,
                max_steps, start_with_reset, self.ctr, env.state, env.elapsed,
                self.obs_full, self.final_obs, self.act_buf, self.rew_buf,
                self.done_buf,
            )
            ext.counter_add_(self.ctr, steps + 1)

        def body():
            if start_with_reset:
                ext.cartpole_env_reset(env.state, env.elapsed, env_seed, steps,
                                       self.ctr, self.obs_full[0])
            else:
                self.obs_full[0].copy_(env.state)
            for t in range(steps):
                logits = ext.mlp_forward(self.obs_full[t], list(weights),
                                         list(biases), acts, False, compute_bf16)[0]
                ext.categorical_sample(logits, policy_seed, t, self.ctr,
                                       self.act_buf[t])
                ext.cartpole_env_step(
                    env.state, env.elapsed, self.act_buf[t], max_steps, env_seed,
                    t, self.ctr, self.obs_full[t + 1], self.final_obs[t],
                    self.rew_buf[t], self.done_buf[t],
                )
            # past every offset used: sample/autoreset t (t<steps), reset steps
            ext.counter_add_(self.ctr, steps + 1)

        # warmup advances ctr and the env carry; snapshot/restore so the
        # first replay starts exactly where the eager world left off
        state = [self.ctr, env.state, env.elapsed]
        self.loop = fop._CapturedLoop(body_fused if self.fused else body, state)

    def replay(self) -> None:
        self.loop.replay()


# ---------------------------------------------------------------------------
# Gaussian policy on the device Pendulum env (DeviceSampler)
# ---------------------------------------------------------------------------
def pendulum_supported(policy, env) -> bool:
    """A GaussianPolicy over an MLP on a GPU DevicePendulumEnv, with the
    extension present and graphs enabled."""
    from rl_replicas_amd.envs.device import DevicePendulumEnv

    if not (isinstance(env, DevicePendulumEnv) and env.device.type == "cuda"
            and ops.hip_available() and fop._graphs_common(None)
            and fop._policy_kind(policy) == "gaussian"):
        return False
    mlp = fop._mlp_of(policy)
    return mlp is not None and _extract_layers(mlp) is not None


def pendulum_fused_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """Whether the epoch runs as ONE persistent kernel (pendulum_rollout_fused,
    pendulum_rollout_kernels.hip) instead of steps x 3 kernels: fp32 compute
    and weights, a net [3, ..., 1] with every width <= 64, one log_std, the
    cut list and the net image within the kernel's limits.
    RL_REPLICAS_AMD_ROLLOUT_FUSED=0 selects the multi-kernel body."""
    import os

    if os.environ.get("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1") == "0":
        return False
    if ops.compute_bf16() != 0:
        return False
    ext = ops._load_extension()
    weights, _, _ = _extract_layers(fop._mlp_of(policy))
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    # the binding's own limits (common.h), so gate and TORCH_CHECKs agree
    max_layers, max_width, max_cuts, max_lds = ext.pendulum_rollout_fused_limits()
    if (len(weights) > max_layers or max(dims) > max_width or dims[0] != 3
            or dims[-1] != 1 or policy.log_std.numel() != 1
            or len(cuts) > max_cuts):
        return False
    if any(t.dtype != torch.float32 for t in (*weights, policy.log_std)):
        return False
    return ext.pendulum_rollout_fused_lds_bytes(dims) <= max_lds


class GraphedPendulumRollout:
    """One captured epoch on a DevicePendulumEnv: [pendulum_env_reset | the
    observation of the carried state] + steps x (mlp_forward ->
    gaussian_sample -> pendulum_env_step) + counter bump; or, when
    `pendulum_fused_eligible`, pendulum_rollout_fused + counter bump.

    Pendulum is lockstep, so the graph is keyed (steps, cuts,
    start_with_reset) like `GraphedRollout`.  The carry between epochs is
    the env's own fp64 `state`, read and written in place; the fp32
    observation rows are derived from it.  Philox offsets (both bodies):
    policy sample and autoreset of step t at `t + ctr` (policy seed / env
    seed), epoch reset at `steps + ctr`; the last node advances the counter
    by steps + 1."""

    def __init__(self, policy, env, steps: int, cuts: Tuple[int, ...],
                 start_with_reset: bool, ctr: torch.Tensor):
        ext = ops._load_extension()
        N = env.num_envs
        dev = env.device
        self.env = env
        self.steps = steps
        self.cuts = list(cuts)
        self.start_with_reset = start_with_reset
        self.obs_full = torch.zeros(steps + 1, N, 3, device=dev)
        self.act_buf = torch.zeros(steps, N, 1, device=dev)
        self.rew_buf = torch.zeros(steps, N, device=dev)
        self.cut_final = torch.zeros(max(len(cuts), 1), N, 3, device=dev)
        self.ctr = ctr
        policy_seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF
        env_seed = env._philox_seed
        state = env.state  # the env's in-place carry
        weights, biases, acts = _extract_layers(fop._mlp_of(policy))
        log_std = policy.log_std
        cset = {c: j for j, c in enumerate(cuts)}
        compute_bf16 = ops.compute_bf16()

        self.fused = pendulum_fused_eligible(policy, env, cuts)

        def body_fused():
            ext.pendulum_rollout_fused(
                list(weights), list(biases), acts, log_std.data, policy_seed,
                env_seed, list(cuts), start_with_reset, self.ctr, state,
                self.obs_full, self.act_buf, self.rew_buf, self.cut_final,
            )
            ext.counter_add_(self.ctr, steps + 1)

        # non-cut steps' successor rows equal obs_full[t + 1]; the kernel
        # still writes them somewhere
        fin_scratch = torch.zeros(N, 3, device=dev)

        def body():
            ext.pendulum_env_reset(state, env_seed, steps, self.ctr,
                                   self.obs_full[0], start_with_reset)
            for t in range(steps):
                mean = ext.mlp_forward(self.obs_full[t], list(weights),
                                       list(biases), acts, False, compute_bf16)[0]
                ext.gaussian_sample(mean, log_std.data, policy_seed, t, -1.0,
                                    -1.0, self.ctr, self.act_buf[t])
                do_reset = t in cset
                ext.pendulum_env_step(
                    state, self.act_buf[t], do_reset, env_seed, t, self.ctr,
                    self.obs_full[t + 1],
                    self.cut_final[cset[t]] if do_reset else fin_scratch,
                    self.rew_buf[t],
                )
            # past every offset used: sample/autoreset t (t<steps), reset steps
            ext.counter_add_(self.ctr, steps + 1)

        # warmup advances ctr and the env carry; snapshot/restore so the
        # first replay starts exactly where the eager world left off
        self.loop = fop._CapturedLoop(body_fused if self.fused else body,
                                      [self.ctr, state])

    def replay(self) -> None:
        self.loop.replay()

    def final_tensors(self) -> List[torch.Tensor]:
        """Per-cut bootstrap observations, in cut order."""
        return [self.cut_final[j] for j in range(len(self.cuts))]
