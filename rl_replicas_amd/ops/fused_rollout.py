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

`GraphedPendulumCollect` is the off-policy construction on
`DevicePendulumEnv` (DeviceReplaySampler): the behaviour policy is the
noised deterministic actor or the uniform warm-up draw, and the epoch's
transitions go straight into a ReplayBuffer's HBM ring at the write
position the buffer holds on the device; the persistent kernel is
`pendulum_collect_fused` (`pendulum_collect_fused_eligible`).

`GraphedPendulumEval` / `GraphedCartPoleEval` run whole evaluation
episodes (evaluator.DeviceEvaluator): from the init draw to each episode's
end, returning only per-episode return, length and init state; the
persistent kernels are `pendulum_eval_fused` / `cartpole_eval_fused`
(`pendulum_eval_fused_eligible` / `cartpole_eval_fused_eligible`).

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


# ---------------------------------------------------------------------------
# Off-policy replay collection on the device Pendulum env
# (DeviceReplaySampler)
# ---------------------------------------------------------------------------
COLLECT_NOISED = "noised"
COLLECT_UNIFORM = "uniform"
_COLLECT_MODE_CODE = {COLLECT_NOISED: 0, COLLECT_UNIFORM: 1}  # common.h
# salt of the uniform warm-up stream (the noised stream keeps
# utils._NoisedPolicy's 0x517CC1B727220A95)
_UNIFORM_SALT = 0x2545F4914F6CDD1D
_NOISE_SALT = 0x517CC1B727220A95


def pendulum_collect_mode(policy, env):
    """Which behaviour policy of OffPolicyAlgorithm.learn `policy` is:
    COLLECT_NOISED (a utils._NoisedPolicy over a DeterministicPolicy over an
    fp32 MLP [3, ..., 1] the fused-MLP kernels take, on the env's device),
    COLLECT_UNIFORM (a RandomPolicy over the env's one-dimensional Box), or
    None."""
    import numpy as np

    from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
    from rl_replicas_amd.utils import _NoisedPolicy

    if isinstance(policy, RandomPolicy):
        space = policy.action_space
        own = env.action_space
        if not all(hasattr(s, "low") and hasattr(s, "high") for s in (space, own)):
            return None
        lo, hi = np.asarray(space.low).reshape(-1), np.asarray(space.high).reshape(-1)
        if (lo.size != 1 or hi.size != 1 or not np.isfinite([lo[0], hi[0]]).all()
                or lo[0] > hi[0]
                or not np.array_equal(lo, np.asarray(own.low).reshape(-1))
                or not np.array_equal(hi, np.asarray(own.high).reshape(-1))):
            return None
        return COLLECT_UNIFORM
    if isinstance(policy, _NoisedPolicy) and isinstance(policy.base_policy,
                                                        DeterministicPolicy):
        mlp = fop._mlp_of(policy.base_policy)
        layers = _extract_layers(mlp) if mlp is not None else None
        if layers is None or policy.action_noise_scale < 0 or policy.action_limit < 0:
            return None
        weights, biases, _ = layers
        if (int(weights[0].shape[1]) != 3 or int(weights[-1].shape[0]) != 1
                or any(t.dtype != torch.float32 or t.device != env.state.device
                       for t in (*weights, *biases))):
            return None
        return COLLECT_NOISED
    return None


def pendulum_collect_supported(policy, env, buffer) -> bool:
    """A behaviour policy of `learn()` on a GPU DevicePendulumEnv whose
    ReplayBuffer lives on the same device, with the extension present and
    graphs enabled."""
    from rl_replicas_amd.envs.device import DevicePendulumEnv

    if not (isinstance(env, DevicePendulumEnv) and env.device.type == "cuda"
            and ops.hip_available() and fop._graphs_common(None)):
        return False
    if buffer is None or buffer.device is None or buffer.device.type != "cuda":
        return False
    if env.state is None or torch.empty(0, device=buffer.device).device != env.state.device:
        return False
    return pendulum_collect_mode(policy, env) is not None


def collect_fused_default() -> bool:
    """Which body a collect graph takes when RL_REPLICAS_AMD_ROLLOUT_FUSED is
    unset: the persistent kernel, which beat the multi-kernel body beyond
    their run-to-run spread at both off-policy shapes and in both modes
    (profiles/bench_replay_collect_1gpu.json, docs/ARCHITECTURE.md)."""
    return True


def collect_wide_threads() -> int:
    """Workgroup size of the persistent kernel's wide regime: 1024 (one
    column tile per wave at width 256), the measured default, or 256 (four
    tiles per wave) with RL_REPLICAS_AMD_COLLECT_WG=256."""
    import os

    return 256 if os.environ.get("RL_REPLICAS_AMD_COLLECT_WG", "1024") == "256" else 1024


def pendulum_collect_fused_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """Whether a collect epoch runs as ONE persistent kernel
    (pendulum_collect_fused, pendulum_collect_kernels.hip) instead of the
    multi-kernel body: fp32 compute and weights, an actor [3, ..., 1] and a
    cut list within the binding's own limits.
    RL_REPLICAS_AMD_ROLLOUT_FUSED=0 selects the multi-kernel body."""
    import os

    default = "1" if collect_fused_default() else "0"
    if os.environ.get("RL_REPLICAS_AMD_ROLLOUT_FUSED", default) == "0":
        return False
    if ops.compute_bf16() != 0:
        return False
    ext = ops._load_extension()
    # the binding's own limits (common.h), so gate and TORCH_CHECKs agree
    max_layers, max_width, max_cuts, max_lds = ext.pendulum_collect_fused_limits()
    if len(cuts) > max_cuts:
        return False
    # an fp32 actor [3, ..., 1] on the env's device, or no net at all
    mode = pendulum_collect_mode(policy, env)
    if mode is None:
        return False
    if mode == COLLECT_UNIFORM:
        return True
    weights, _, _ = _extract_layers(fop._mlp_of(policy.base_policy))
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    if len(weights) > max_layers or max(dims) > max_width:
        return False
    return ext.pendulum_collect_fused_lds_bytes(dims) <= max_lds


class GraphedPendulumCollect:
    """One captured off-policy collect epoch on a DevicePendulumEnv, written
    straight into a ReplayBuffer's HBM ring at the write position the
    buffer holds on the device.

    Fused body (`pendulum_collect_fused_eligible`): pendulum_collect_fused,
    ring_advance_, counter_add_.  Multi-kernel body: pendulum_env_reset,
    steps x ([mlp_forward -> gaussian_sample with noise scale / limit] |
    uniform_sample, then pendulum_env_step), replay_scatter, ring_advance_,
    counter_add_.  Both write the same bytes.

    Keyed (steps, cuts, start_with_reset, mode) by the sampler.  Philox
    offsets (both bodies): action and autoreset of step t at `t + ctr`
    (action seed / env seed), epoch reset at `steps + ctr`; the counter
    advances by steps + 1.  Warm-up leaves no trace: the counter, the env
    carry and both ring scalars are restored by `_CapturedLoop`, the ring
    rows the warm-up runs wrote are put back here."""

    def __init__(self, policy, env, buffer, steps: int, cuts: Tuple[int, ...],
                 start_with_reset: bool, mode: str, ctr: torch.Tensor):
        ext = ops._load_extension()
        N = env.num_envs
        dev = env.device
        n = N * steps
        cap = buffer.buffer_size
        assert n <= cap
        self.env = env
        self.buffer = buffer
        self.steps = steps
        self.cuts = list(cuts)
        self.start_with_reset = start_with_reset
        self.mode = mode
        self.ctr = ctr
        self.n_segs = len(cuts) + (1 if not cuts or cuts[-1] != steps - 1 else 0)
        # the one read-back of an epoch
        self.seg_returns = torch.zeros(N, self.n_segs, device=dev)
        storage, write_dev, size_dev = buffer.device_ring(3, (1,))
        state = env.state  # the env's in-place carry
        env_seed = env._philox_seed
        base_seed = torch.initial_seed()
        cset = {c: j for j, c in enumerate(cuts)}
        compute_bf16 = ops.compute_bf16()
        low = float(env.action_space.low.reshape(-1)[0])
        high = float(env.action_space.high.reshape(-1)[0])
        if mode == COLLECT_NOISED:
            weights, biases, acts = _extract_layers(fop._mlp_of(policy.base_policy))
            weights, biases = list(weights), list(biases)
            action_seed = (base_seed ^ _NOISE_SALT) & 0x7FFFFFFFFFFFFFFF
            noise_scale = float(policy.action_noise_scale)
            limit = float(policy.action_limit)
            dummy_log_std = torch.zeros(1, device=dev)
        else:
            weights, biases, acts = [], [], []
            action_seed = (base_seed ^ _UNIFORM_SALT) & 0x7FFFFFFFFFFFFFFF
            noise_scale, limit = 0.0, 0.0

        self.fused = pendulum_collect_fused_eligible(policy, env, cuts)
        wide_threads = collect_wide_threads()

        if self.fused:
            self.last_obs = torch.zeros(N, 3, device=dev)

            def body():
                ext.pendulum_collect_fused(
                    weights, biases, acts, _COLLECT_MODE_CODE[mode], noise_scale,
                    limit, low, high, action_seed, env_seed, list(cuts),
                    start_with_reset, self.ctr, state, steps, storage, write_dev,
                    size_dev, self.seg_returns, self.last_obs, wide_threads,
                )
                ext.ring_advance_(write_dev, size_dev, n, cap)
                ext.counter_add_(self.ctr, steps + 1)
        else:
            self.obs_full = torch.zeros(steps + 1, N, 3, device=dev)
            self.act_buf = torch.zeros(steps, N, 1, device=dev)
            self.rew_buf = torch.zeros(steps, N, device=dev)
            self.cut_final = torch.zeros(max(len(cuts), 1), N, 3, device=dev)
            self.last_obs = self.obs_full[steps]
            cut_slot = torch.tensor([cset.get(t, -1) for t in range(steps)],
                                    dtype=torch.int32, device=dev)
            fin_scratch = torch.zeros(N, 3, device=dev)

            def body():
                ext.pendulum_env_reset(state, env_seed, steps, self.ctr,
                                       self.obs_full[0], start_with_reset)
                for t in range(steps):
                    if mode == COLLECT_NOISED:
                        mean = ext.mlp_forward(self.obs_full[t], weights, biases,
                                               acts, False, compute_bf16)[0]
                        ext.gaussian_sample(mean, dummy_log_std, action_seed, t,
                                            noise_scale, limit, self.ctr,
                                            self.act_buf[t])
                    else:
                        ext.uniform_sample(self.act_buf[t], low, high, action_seed,
                                           t, self.ctr)
                    do_reset = t in cset
                    ext.pendulum_env_step(
                        state, self.act_buf[t], do_reset, env_seed, t, self.ctr,
                        self.obs_full[t + 1],
                        self.cut_final[cset[t]] if do_reset else fin_scratch,
                        self.rew_buf[t],
                    )
                ext.replay_scatter(self.obs_full, self.act_buf, self.rew_buf,
                                   self.cut_final, cut_slot, len(cuts), storage,
                                   write_dev, size_dev, self.seg_returns)
                ext.ring_advance_(write_dev, size_dev, n, cap)
                # past every offset used: action/autoreset t (t<steps), reset steps
                ext.counter_add_(self.ctr, steps + 1)

        # the two warm-up runs write ring rows [write, write + 2n): keep what
        # they held, so warm-up never costs a stored transition
        touched = (buffer._write + torch.arange(min(2 * n, cap), device=dev)) % cap
        kept = [t[touched] for t in storage]
        self.loop = fop._CapturedLoop(body, [self.ctr, state, write_dev, size_dev])
        for t, k in zip(storage, kept):
            t[touched] = k

    def replay(self) -> None:
        self.loop.replay()
        self.buffer.advance_host(self.env.num_envs * self.steps)


# ---------------------------------------------------------------------------
# Whole-episode policy evaluation on the device Pendulum / CartPole dynamics
# (evaluator.DeviceEvaluator)
# ---------------------------------------------------------------------------
EVAL_DETERMINISTIC = "deterministic"
EVAL_GAUSSIAN = "gaussian"
_EVAL_MODE_CODE = {EVAL_DETERMINISTIC: 0, EVAL_GAUSSIAN: 1}  # common.h


def pendulum_eval_mode(policy):
    """How an evaluation turns `policy`'s net output into a Pendulum torque:
    EVAL_DETERMINISTIC for a DeterministicPolicy over an MLP the fused-MLP
    kernels take (the output itself; the env clamps), EVAL_GAUSSIAN for a
    GaussianPolicy over one (a sample around it), or None."""
    from rl_replicas_amd.policies import DeterministicPolicy

    if isinstance(policy, DeterministicPolicy):
        mode = EVAL_DETERMINISTIC
    elif fop._policy_kind(policy) == "gaussian":
        mode = EVAL_GAUSSIAN
    else:
        return None
    mlp = fop._mlp_of(policy)
    if mlp is None or _extract_layers(mlp) is None:
        return None
    return mode


def eval_fused_default(kind: str) -> bool:
    """Which body an evaluation graph of `kind` ("pendulum" | "cartpole")
    takes when RL_REPLICAS_AMD_ROLLOUT_FUSED is unset: the persistent kernel
    where it beat the multi-kernel body beyond the two bodies' run-to-run
    spread at 5 episodes (profiles/bench_device_eval_1gpu.json,
    docs/ARCHITECTURE.md)."""
    return True


def _eval_fused_common(policy, kind: str, ext, limits, lds_bytes, in_dim: int) -> bool:
    import os

    default = "1" if eval_fused_default(kind) else "0"
    if os.environ.get("RL_REPLICAS_AMD_ROLLOUT_FUSED", default) == "0":
        return False
    if ops.compute_bf16() != 0:
        return False
    weights, biases, _ = _extract_layers(fop._mlp_of(policy))
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    # the binding's own limits (common.h), so gate and TORCH_CHECKs agree
    max_layers, max_width, max_lds = limits
    if len(weights) > max_layers or max(dims) > max_width or dims[0] != in_dim:
        return False
    if any(t.dtype != torch.float32 for t in (*weights, *biases)):
        return False
    return lds_bytes(dims) <= max_lds


def pendulum_eval_fused_eligible(policy) -> bool:
    """Whether a Pendulum evaluation runs as ONE persistent kernel
    (pendulum_eval_fused, eval_kernels.hip) instead of the multi-kernel
    body: fp32 compute and parameters, a net [3, ..., 1] within the binding's
    own limits, one log_std for a Gaussian policy.
    RL_REPLICAS_AMD_ROLLOUT_FUSED=0 selects the multi-kernel body."""
    mode = pendulum_eval_mode(policy)
    if mode is None:
        return False
    ext = ops._load_extension()
    weights, _, _ = _extract_layers(fop._mlp_of(policy))
    if int(weights[-1].shape[0]) != 1:
        return False
    if mode == EVAL_GAUSSIAN and (policy.log_std.numel() != 1
                                  or policy.log_std.dtype != torch.float32):
        return False
    return _eval_fused_common(policy, "pendulum", ext, ext.pendulum_eval_fused_limits(),
                              ext.pendulum_eval_fused_lds_bytes, 3)


def cartpole_eval_fused_eligible(policy) -> bool:
    """Whether a CartPole evaluation runs as ONE persistent kernel
    (cartpole_eval_fused, eval_kernels.hip) instead of the multi-kernel
    body: fp32 compute and parameters, a categorical net [4, ..., n_act]
    with every width <= 64, within the binding's own limits.
    RL_REPLICAS_AMD_ROLLOUT_FUSED=0 selects the multi-kernel body."""
    if fop._policy_kind(policy) != "categorical":
        return False
    mlp = fop._mlp_of(policy)
    if mlp is None or _extract_layers(mlp) is None:
        return False
    ext = ops._load_extension()
    return _eval_fused_common(policy, "cartpole", ext, ext.cartpole_eval_fused_limits(),
                              ext.cartpole_eval_fused_lds_bytes, 4)


class _GraphedEval:
    """What both evaluation graphs share: the per-episode outputs, the two
    device counters and the captured loop.

    Philox contract (both bodies): the init draw at (env_seed, *reset_ctr,
    row), the action of step t at (policy_seed, t + *ctr, row).  Every replay
    advances `ctr` by `horizon`; `reset_ctr` advances by 1 only when
    `advance_reset` (an unseeded evaluator: fresh init states per call).
    The weight pointers are those of the live parameters."""

    state_dim = 0

    def __init__(self, num_episodes: int, horizon: int, ctr: torch.Tensor,
                 reset_ctr: torch.Tensor, advance_reset: bool):
        assert num_episodes >= 1 and horizon >= 1
        dev = ctr.device
        self.num_episodes = num_episodes
        self.horizon = horizon
        self.ctr = ctr
        self.reset_ctr = reset_ctr
        self.advance_reset = advance_reset
        self.returns = torch.zeros(num_episodes, dtype=torch.float64, device=dev)
        self.lengths = torch.zeros(num_episodes, dtype=torch.int32, device=dev)
        self.init_state = torch.zeros(num_episodes, self.state_dim,
                                      dtype=torch.float64, device=dev)
        self.policy_seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF

    def _bump(self, ext) -> None:
        ext.counter_add_(self.ctr, self.horizon)
        if self.advance_reset:
            ext.counter_add_(self.reset_ctr, 1)

    def _capture(self, body) -> None:
        # warm-up advances both counters; snapshot/restore so the first
        # replay draws what an uncaptured first call would
        self.loop = fop._CapturedLoop(body, [self.ctr, self.reset_ctr])

    def replay(self) -> None:
        self.loop.replay()


class GraphedPendulumEval(_GraphedEval):
    """One captured evaluation of `num_episodes` Pendulum episodes of
    `horizon` steps.

    Fused body (`pendulum_eval_fused_eligible`): pendulum_eval_fused, then
    the counter bumps.  Multi-kernel body: pendulum_env_reset into a private
    state tensor (copied to `init_state`), horizon x (mlp_forward ->
    [gaussian_sample] -> pendulum_env_step), episode_reduce, the counter
    bumps; it keeps `act_buf` [horizon, N, 1].  Both write the same bytes to
    `returns`, `lengths` and `init_state`."""

    state_dim = 2

    def __init__(self, policy, num_episodes: int, horizon: int, env_seed: int,
                 ctr: torch.Tensor, reset_ctr: torch.Tensor,
                 advance_reset: bool = False):
        super().__init__(num_episodes, horizon, ctr, reset_ctr, advance_reset)
        ext = ops._load_extension()
        N, dev = num_episodes, ctr.device
        self.mode = pendulum_eval_mode(policy)
        assert self.mode is not None
        weights, biases, acts = _extract_layers(fop._mlp_of(policy))
        weights, biases = list(weights), list(biases)
        gaussian = self.mode == EVAL_GAUSSIAN
        log_std = policy.log_std if gaussian else None
        policy_seed = self.policy_seed
        compute_bf16 = ops.compute_bf16()

        self.fused = pendulum_eval_fused_eligible(policy)
        wide_threads = collect_wide_threads()

        if self.fused:
            def body():
                ext.pendulum_eval_fused(
                    weights, biases, acts, _EVAL_MODE_CODE[self.mode],
                    log_std.data if gaussian else None, policy_seed, env_seed,
                    horizon, self.ctr, self.reset_ctr, self.returns, self.lengths,
                    self.init_state, wide_threads,
                )
                self._bump(ext)
        else:
            self.state = torch.zeros(N, 2, dtype=torch.float64, device=dev)
            self.obs_full = torch.zeros(horizon + 1, N, 3, device=dev)
            self.rew_buf = torch.zeros(horizon, N, device=dev)
            if gaussian:
                self._act_buf = torch.zeros(horizon, N, 1, device=dev)
            # the step kernel's successor rows: unused, but the graph writes
            # them on every replay, so the storage lives as long as the graph
            self._fin_scratch = fin_scratch = torch.zeros(N, 3, device=dev)
            self._means: List[torch.Tensor] = []

            def body():
                means = []
                ext.pendulum_env_reset(self.state, env_seed, 0, self.reset_ctr,
                                       self.obs_full[0], True)
                self.init_state.copy_(self.state)
                for t in range(horizon):
                    action = ext.mlp_forward(self.obs_full[t], weights, biases,
                                             acts, False, compute_bf16)[0]
                    if gaussian:
                        ext.gaussian_sample(action, log_std.data, policy_seed, t,
                                            -1.0, -1.0, self.ctr, self._act_buf[t])
                        action = self._act_buf[t]
                    else:
                        means.append(action)  # the deterministic action itself
                    ext.pendulum_env_step(self.state, action, False, env_seed, t,
                                          self.ctr, self.obs_full[t + 1],
                                          fin_scratch, self.rew_buf[t])
                ext.episode_reduce(self.rew_buf, None, self.returns, self.lengths)
                self._bump(ext)
                self._means = means  # the captured run's outputs

        self._capture(body)

    @property
    def act_buf(self) -> torch.Tensor:
        """[horizon, N, 1] actions of the last replay (multi-kernel body)."""
        if self.mode == EVAL_GAUSSIAN:
            return self._act_buf
        return torch.stack(self._means).reshape(self.horizon, self.num_episodes, 1)


class GraphedCartPoleEval(_GraphedEval):
    """One captured evaluation of `num_episodes` CartPole episodes of at most
    `horizon` steps under a CategoricalPolicy.

    Fused body (`cartpole_eval_fused_eligible`): cartpole_eval_fused, which
    stops stepping once every row of a workgroup has finished, then the
    counter bumps.  Multi-kernel body: cartpole_env_reset into private carry
    tensors (state copied to `init_state`), horizon x (mlp_forward ->
    categorical_sample -> cartpole_env_step with autoreset), episode_reduce
    over each row's first episode, the counter bumps; it keeps `act_buf`
    [horizon, N].  Both write the same bytes to `returns`, `lengths` and
    `init_state`."""

    state_dim = 4

    def __init__(self, policy, num_episodes: int, horizon: int, env_seed: int,
                 ctr: torch.Tensor, reset_ctr: torch.Tensor,
                 advance_reset: bool = False):
        super().__init__(num_episodes, horizon, ctr, reset_ctr, advance_reset)
        ext = ops._load_extension()
        N, dev = num_episodes, ctr.device
        assert fop._policy_kind(policy) == "categorical"
        weights, biases, acts = _extract_layers(fop._mlp_of(policy))
        weights, biases = list(weights), list(biases)
        policy_seed = self.policy_seed
        compute_bf16 = ops.compute_bf16()

        self.fused = cartpole_eval_fused_eligible(policy)

        if self.fused:
            def body():
                ext.cartpole_eval_fused(
                    weights, biases, acts, policy_seed, env_seed, horizon,
                    self.ctr, self.reset_ctr, self.returns, self.lengths,
                    self.init_state,
                )
                self._bump(ext)
        else:
            self.state = torch.zeros(N, 4, dtype=torch.float64, device=dev)
            self.elapsed = torch.zeros(N, dtype=torch.int32, device=dev)
            self.obs_full = torch.zeros(horizon + 1, N, 4, device=dev)
            self.act_buf = torch.zeros(horizon, N, dtype=torch.int64, device=dev)
            self.rew_buf = torch.zeros(horizon, N, device=dev)
            self.done_buf = torch.zeros(horizon, N, dtype=torch.uint8, device=dev)
            # unused successor rows the graph writes on every replay
            self._fin_scratch = fin_scratch = torch.zeros(N, 4, device=dev)

            def body():
                ext.cartpole_env_reset(self.state, self.elapsed, env_seed, 0,
                                       self.reset_ctr, self.obs_full[0])
                self.init_state.copy_(self.state)
                for t in range(horizon):
                    logits = ext.mlp_forward(self.obs_full[t], weights, biases,
                                             acts, False, compute_bf16)[0]
                    ext.categorical_sample(logits, policy_seed, t, self.ctr,
                                           self.act_buf[t])
                    ext.cartpole_env_step(
                        self.state, self.elapsed, self.act_buf[t], horizon,
                        env_seed, t, self.ctr, self.obs_full[t + 1], fin_scratch,
                        self.rew_buf[t], self.done_buf[t],
                    )
                ext.episode_reduce(self.rew_buf, self.done_buf, self.returns,
                                   self.lengths)
                self._bump(ext)

        self._capture(body)
