"""hipGraph-captured device rollouts, replay collection and evaluation.

One construction, seven classes.  The eager device loops issue 3 kernels per
env step (fused MLP forward, Philox action sample, fused env transition);
here a whole epoch (reset or state carry, steps x [forward -> sample -> env
step], the trailing nodes, one RNG-counter bump) is captured once and
replayed as a single hipGraph.  Where `_fused_gate` admits the net (fp32,
within the binding's own limits; RL_REPLICAS_AMD_ROLLOUT_FUSED=0 declines)
the steps of that graph are ONE persistent kernel that carries 16 env rows
per workgroup through every step with weights and state in LDS, using the
device functions, Philox offsets and element indices of the step kernels, so
both bodies write the same bytes.  The multi-kernel bodies share one step
loop per env (`_pendulum_epoch`, `_cartpole_epoch`).

Randomness across replays: by-value Philox offsets are frozen at capture, so
every RNG kernel adds a device-resident int64 counter to its offset, and the
graph's last node advances the counter past every offset used: each replay
draws a fresh, deterministic slice of the stream (same seed =>
bitwise-identical run).  Weights and log_std are read by pointer, so the
updates between epochs are visible to the next replay without re-capture.
Lockstep envs re-capture only when the epoch's truncation pattern (`cuts`)
changes; the samplers cap that cache.

What differs per class:

  GraphedRollout          GaussianPolicy on the synthetic DeviceVectorEnv
                          (DeviceSampler); carry in obs_full[steps];
                          `ppo_rollout_fused`.
  GraphedCartPoleRollout  CategoricalPolicy on DeviceCartPoleEnv
                          (DeviceEpisodicSampler); termination, truncation
                          and autoreset in-kernel per instance, so no cuts;
                          `cartpole_rollout_fused`.
  GraphedPendulumRollout  GaussianPolicy on DevicePendulumEnv (DeviceSampler);
                          lockstep cuts, carry in the env's fp64 `state`;
                          `pendulum_rollout_fused`.
  GraphedPendulumCollect  noised actor or uniform warm-up draw on
                          DevicePendulumEnv (DeviceReplaySampler), written
                          straight into a ReplayBuffer's HBM ring;
                          `pendulum_collect_fused`.
  GraphedSyntheticCollect the same two behaviour policies on the synthetic
                          DeviceVectorEnv (DeviceReplaySampler), any O and A
                          up to one wave; the graph owns the carry [N, O];
                          `synthetic_collect_fused`.
  GraphedPendulumEval /   whole evaluation episodes (DeviceEvaluator), only
  GraphedCartPoleEval     per-episode return, length and init state come
                          back; `pendulum_eval_fused` / `cartpole_eval_fused`.

No reference counterpart (the reference samples one env serially on
the host, batch_sampler.py:55-99).
"""
from __future__ import annotations

import os
from typing import List, Tuple

import torch

from rl_replicas_amd import ops
from rl_replicas_amd.ops import fused_onpolicy as fop
from rl_replicas_amd.ops.fused_mlp import _extract_layers


# ---------------------------------------------------------------------------
# Gates
# ---------------------------------------------------------------------------
def _env_ready(env, env_cls) -> bool:
    return (isinstance(env, env_cls) and env.device.type == "cuda"
            and ops.hip_available() and fop._graphs_common(None))


def _graph_supported(policy, env, env_cls, kind: str) -> bool:
    """A policy of `kind` over an MLP the fused-MLP kernels take, on a GPU
    env of `env_cls`, with the extension present and graphs enabled."""
    if not (_env_ready(env, env_cls) and fop._policy_kind(policy) == kind):
        return False
    mlp = fop._mlp_of(policy)
    return mlp is not None and _extract_layers(mlp) is not None


def _fused_gate(weights, extra_fp32, limits, lds_bytes, in_dim: int,
                out_dim=None, cuts=None, default: bool = True) -> bool:
    """Whether a graph's steps run as ONE persistent kernel: not declined by
    RL_REPLICAS_AMD_ROLLOUT_FUSED (`default` when unset), fp32 compute, and
    the net within `limits`, the binding's own (common.h), so gate and
    TORCH_CHECKs agree: (max_layers, max_width, [max_cuts,] max_lds).

    `weights` is the net [in_dim, ..., out_dim] (None: the body reads no
    net), `extra_fp32` what must be fp32 beside the weights, `lds_bytes`
    maps dims to the kernel's LDS need, `cuts` is checked against max_cuts
    where the limits carry one."""
    if os.environ.get("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1" if default else "0") == "0":
        return False
    if ops.compute_bf16() != 0:
        return False
    max_layers, max_width, *max_cuts, max_lds = limits
    if cuts is not None and max_cuts and len(cuts) > max_cuts[0]:
        return False
    if weights is None:
        return True
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    if (len(weights) > max_layers or max(dims) > max_width or dims[0] != in_dim
            or (out_dim is not None and dims[-1] != out_dim)):
        return False
    if any(t.dtype != torch.float32 for t in (*weights, *extra_fp32)):
        return False
    return lds_bytes(dims) <= max_lds


def _weights_of(policy):
    return _extract_layers(fop._mlp_of(policy))[0]


def make_counter(device) -> torch.Tensor:
    """Device RNG counter; base 2^40 keeps the graph streams clear of the
    host-side offsets the eager paths use under the same seeds."""
    return torch.full((1,), 1 << 40, dtype=torch.int64, device=device)


# ---------------------------------------------------------------------------
# The multi-kernel step loops
# ---------------------------------------------------------------------------
def _pendulum_epoch(ext, state, env_seed, steps: int, cuts, action, reset,
                    ctr, obs_full, rew_buf, cut_final, fin_scratch,
                    after_reset=None) -> None:
    """Issue pendulum_env_reset, then steps x (`action(t)` ->
    pendulum_env_step) on the fp64 carry `state`.  `reset` is (Philox
    offset, counter, draw a fresh state?); `action(t)` issues the step's
    action kernels and returns the [N, 1] action.  A cut step writes its
    true successor to `cut_final[slot]`; every other step's successor equals
    obs_full[t + 1], and the kernel still writes it somewhere:
    `fin_scratch`."""
    offset, reset_ctr, fresh = reset
    ext.pendulum_env_reset(state, env_seed, offset, reset_ctr, obs_full[0], fresh)
    if after_reset is not None:
        after_reset()
    cset = {c: j for j, c in enumerate(cuts)}
    for t in range(steps):
        act = action(t)
        do_reset = t in cset
        ext.pendulum_env_step(
            state, act, do_reset, env_seed, t, ctr, obs_full[t + 1],
            cut_final[cset[t]] if do_reset else fin_scratch, rew_buf[t],
        )


def _cartpole_epoch(ext, net, seeds, state, elapsed, max_steps: int, steps: int,
                    reset, ctr, obs_full, finals, act_buf, rew_buf, done_buf,
                    after_reset=None) -> None:
    """Issue cartpole_env_reset (`reset` = (Philox offset, counter)) or, with
    `reset` None, the copy of the carried state, then steps x (mlp_forward
    -> categorical_sample -> cartpole_env_step).  `finals[t]` takes step t's
    pre-autoreset successor."""
    weights, biases, acts = net
    policy_seed, env_seed = seeds
    compute_bf16 = ops.compute_bf16()
    if reset is not None:
        ext.cartpole_env_reset(state, elapsed, env_seed, *reset, obs_full[0])
    else:
        obs_full[0].copy_(state)
    if after_reset is not None:
        after_reset()
    for t in range(steps):
        logits = ext.mlp_forward(obs_full[t], list(weights), list(biases), acts,
                                 False, compute_bf16)[0]
        ext.categorical_sample(logits, policy_seed, t, ctr, act_buf[t])
        ext.cartpole_env_step(
            state, elapsed, act_buf[t], max_steps, env_seed, t, ctr,
            obs_full[t + 1], finals[t], rew_buf[t], done_buf[t],
        )


# ---------------------------------------------------------------------------
# Gaussian policy on the synthetic envs (DeviceSampler)
# ---------------------------------------------------------------------------
def supported(policy, env) -> bool:
    from rl_replicas_amd.envs.device import DeviceVectorEnv

    return _graph_supported(policy, env, DeviceVectorEnv, "gaussian")


def fused_kernel_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """ppo_rollout_fused (rollout_fused_kernels.hip) takes the epoch: a
    Gaussian policy without action clipping (the only kind `supported`
    admits), every width and the obs dim <= 64, one log_std per action."""
    ext = ops._load_extension()
    O, A = int(env.A.shape[0]), int(env.B.shape[0])
    return policy.log_std.numel() == A and _fused_gate(
        _weights_of(policy), [policy.log_std], ext.ppo_rollout_fused_limits(),
        lambda dims: ext.ppo_rollout_fused_lds_bytes(dims, O, A), O, A, cuts)


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
    from rl_replicas_amd.envs.device import DeviceCartPoleEnv

    return _graph_supported(policy, env, DeviceCartPoleEnv, "categorical")


def cartpole_fused_eligible(policy, env) -> bool:
    """cartpole_rollout_fused (cartpole_rollout_kernels.hip) takes the epoch:
    a net [4, ...] with every width <= 64."""
    ext = ops._load_extension()
    return _fused_gate(_weights_of(policy), (), ext.cartpole_rollout_fused_limits(),
                       ext.cartpole_rollout_fused_lds_bytes, 4)


class GraphedCartPoleRollout:
    """One captured epoch on a DeviceCartPoleEnv: `_cartpole_epoch` + counter
    bump; or, when `cartpole_fused_eligible`, cartpole_rollout_fused +
    counter bump.

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
        net = weights, biases, acts = _extract_layers(fop._mlp_of(policy))

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
            _cartpole_epoch(
                ext, net, (policy_seed, env_seed), env.state, env.elapsed,
                max_steps, steps, (steps, self.ctr) if start_with_reset else None,
                self.ctr, self.obs_full, self.final_obs, self.act_buf,
                self.rew_buf, self.done_buf,
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
    from rl_replicas_amd.envs.device import DevicePendulumEnv

    return _graph_supported(policy, env, DevicePendulumEnv, "gaussian")


def pendulum_fused_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """pendulum_rollout_fused (pendulum_rollout_kernels.hip) takes the epoch:
    a net [3, ..., 1] with every width <= 64, one log_std, the cut list
    within the by-value limit."""
    ext = ops._load_extension()
    return policy.log_std.numel() == 1 and _fused_gate(
        _weights_of(policy), [policy.log_std], ext.pendulum_rollout_fused_limits(),
        ext.pendulum_rollout_fused_lds_bytes, 3, 1, cuts)


class GraphedPendulumRollout:
    """One captured epoch on a DevicePendulumEnv: `_pendulum_epoch` with a
    Gaussian sample as the action + counter bump; or, when
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
        compute_bf16 = ops.compute_bf16()

        self.fused = pendulum_fused_eligible(policy, env, cuts)

        def body_fused():
            ext.pendulum_rollout_fused(
                list(weights), list(biases), acts, log_std.data, policy_seed,
                env_seed, list(cuts), start_with_reset, self.ctr, state,
                self.obs_full, self.act_buf, self.rew_buf, self.cut_final,
            )
            ext.counter_add_(self.ctr, steps + 1)

        fin_scratch = torch.zeros(N, 3, device=dev)

        def action(t):
            mean = ext.mlp_forward(self.obs_full[t], list(weights), list(biases),
                                   acts, False, compute_bf16)[0]
            ext.gaussian_sample(mean, log_std.data, policy_seed, t, -1.0, -1.0,
                                self.ctr, self.act_buf[t])
            return self.act_buf[t]

        def body():
            _pendulum_epoch(ext, state, env_seed, steps, cuts, action,
                            (steps, self.ctr, start_with_reset), self.ctr,
                            self.obs_full, self.rew_buf, self.cut_final, fin_scratch)
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

    if not _env_ready(env, DevicePendulumEnv):
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
    return 256 if os.environ.get("RL_REPLICAS_AMD_COLLECT_WG", "1024") == "256" else 1024


def pendulum_collect_fused_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """pendulum_collect_fused (pendulum_collect_kernels.hip) takes the collect
    epoch: an actor [3, ..., 1], or no net at all (the uniform draw), and a
    cut list within the binding's own limits."""
    mode = pendulum_collect_mode(policy, env)
    if mode is None:
        return False
    ext = ops._load_extension()
    # COLLECT_NOISED already means fp32 weights and biases [3, ..., 1], so the
    # gate's own dtype and width checks cannot change the answer here
    weights = _weights_of(policy.base_policy) if mode == COLLECT_NOISED else None
    return _fused_gate(weights, (), ext.pendulum_collect_fused_limits(),
                       ext.pendulum_collect_fused_lds_bytes, 3, 1, cuts,
                       default=collect_fused_default())


class GraphedPendulumCollect:
    """One captured off-policy collect epoch on a DevicePendulumEnv, written
    straight into a ReplayBuffer's HBM ring at the write position the
    buffer holds on the device.

    Fused body (`pendulum_collect_fused_eligible`): pendulum_collect_fused,
    ring_advance_, counter_add_.  Multi-kernel body: `_pendulum_epoch` whose
    action is [mlp_forward -> gaussian_sample with noise scale / limit] or
    uniform_sample, then replay_scatter, ring_advance_, counter_add_.  Both
    write the same bytes.

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
            cut_slot = torch.tensor(
                [cuts.index(t) if t in cuts else -1 for t in range(steps)],
                dtype=torch.int32, device=dev)
            fin_scratch = torch.zeros(N, 3, device=dev)

            def action(t):
                if mode == COLLECT_NOISED:
                    mean = ext.mlp_forward(self.obs_full[t], weights, biases,
                                           acts, False, compute_bf16)[0]
                    ext.gaussian_sample(mean, dummy_log_std, action_seed, t,
                                        noise_scale, limit, self.ctr,
                                        self.act_buf[t])
                else:
                    ext.uniform_sample(self.act_buf[t], low, high, action_seed,
                                       t, self.ctr)
                return self.act_buf[t]

            def body():
                _pendulum_epoch(ext, state, env_seed, steps, cuts, action,
                                (steps, self.ctr, start_with_reset), self.ctr,
                                self.obs_full, self.rew_buf, self.cut_final,
                                fin_scratch)
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
# Off-policy replay collection on the synthetic envs (DeviceReplaySampler)
# ---------------------------------------------------------------------------
def _scalar_bounds(space):
    """(low, high) of a Box every dimension of which has the same finite
    bounds, else None: the sample kernels take scalar bounds."""
    import numpy as np

    if not (hasattr(space, "low") and hasattr(space, "high")):
        return None
    lo, hi = np.asarray(space.low).reshape(-1), np.asarray(space.high).reshape(-1)
    if (lo.size < 1 or lo.size != hi.size or not np.isfinite([lo[0], hi[0]]).all()
            or lo[0] > hi[0] or (lo != lo[0]).any() or (hi != hi[0]).any()):
        return None
    return float(lo[0]), float(hi[0])


def synthetic_collect_mode(policy, env):
    """Which behaviour policy of OffPolicyAlgorithm.learn `policy` is on a
    synthetic DeviceVectorEnv with observations O and actions A wide:
    COLLECT_NOISED (a utils._NoisedPolicy over a DeterministicPolicy over an
    fp32 MLP [O, ..., A] the fused-MLP kernels take, on the env's device),
    COLLECT_UNIFORM (a RandomPolicy over a Box with one finite low and one
    finite high shared by every dimension, equal to the env's), or None."""
    from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
    from rl_replicas_amd.utils import _NoisedPolicy

    O, A = int(env.A.shape[0]), int(env.B.shape[0])
    if isinstance(policy, RandomPolicy):
        bounds = _scalar_bounds(policy.action_space)
        if (bounds is None or bounds != _scalar_bounds(env.action_space)
                or tuple(policy.action_space.shape) != (A,)):
            return None
        return COLLECT_UNIFORM
    if isinstance(policy, _NoisedPolicy) and isinstance(policy.base_policy,
                                                        DeterministicPolicy):
        mlp = fop._mlp_of(policy.base_policy)
        layers = _extract_layers(mlp) if mlp is not None else None
        if layers is None or policy.action_noise_scale < 0 or policy.action_limit < 0:
            return None
        weights, biases, _ = layers
        if (int(weights[0].shape[1]) != O or int(weights[-1].shape[0]) != A
                or any(t.dtype != torch.float32 or t.device != env.A.device
                       for t in (*weights, *biases))):
            return None
        return COLLECT_NOISED
    return None


def synthetic_collect_supported(policy, env, buffer) -> bool:
    """A behaviour policy of `learn()` on a GPU DeviceVectorEnv whose
    ReplayBuffer lives on the same device, with the extension present and
    graphs enabled."""
    from rl_replicas_amd.envs.device import DeviceVectorEnv

    if not _env_ready(env, DeviceVectorEnv):
        return False
    if buffer is None or buffer.device is None or buffer.device.type != "cuda":
        return False
    if torch.empty(0, device=buffer.device).device != env.A.device:
        return False
    return synthetic_collect_mode(policy, env) is not None


def synthetic_collect_fused_default() -> bool:
    """Which body a synthetic-env collect graph takes when
    RL_REPLICAS_AMD_ROLLOUT_FUSED is unset.  The persistent kernel is the
    default only where it beat the multi-kernel body by more than the larger
    of the two bodies' run-to-run spread at both off-policy shapes (1 x 50,
    10 x 5) and in both modes (profiles/bench_synthetic_collect_1gpu.json,
    docs/ARCHITECTURE.md)."""
    return False


def synthetic_collect_fused_eligible(policy, env, cuts: Tuple[int, ...]) -> bool:
    """synthetic_collect_fused (synthetic_collect_kernels.hip) takes the
    collect epoch: O and A at most one wave wide, an actor [O, ..., A] or no
    net at all (the uniform draw), net + env image within the LDS budget and
    a cut list within the binding's own limits."""
    mode = synthetic_collect_mode(policy, env)
    if mode is None:
        return False
    ext = ops._load_extension()
    O, A = int(env.A.shape[0]), int(env.B.shape[0])
    limits = ext.synthetic_collect_fused_limits()
    # one wave carries a row: ROLLOUT_MAX_WIDTH, as ppo_rollout_fused has it
    if max(O, A) > ext.ppo_rollout_fused_limits()[1]:
        return False
    if mode == COLLECT_UNIFORM and ext.synthetic_collect_fused_lds_bytes([], O, A) > limits[-1]:
        return False
    # COLLECT_NOISED already means fp32 weights and biases [O, ..., A], so the
    # gate's own dtype and width checks cannot change the answer here
    weights = _weights_of(policy.base_policy) if mode == COLLECT_NOISED else None
    return _fused_gate(weights, (), limits,
                       lambda dims: ext.synthetic_collect_fused_lds_bytes(dims, O, A),
                       O, A, cuts, default=synthetic_collect_fused_default())


class GraphedSyntheticCollect:
    """One captured off-policy collect epoch on a synthetic DeviceVectorEnv,
    written straight into a ReplayBuffer's HBM ring at the write position the
    buffer holds on the device.

    Fused body (`synthetic_collect_fused_eligible`): synthetic_collect_fused,
    ring_advance_, counter_add_.  Multi-kernel body: synthetic_env_reset or
    the carry copy, steps x ([mlp_forward -> gaussian_sample with noise scale
    / limit] or uniform_sample, then synthetic_env_step), then
    replay_scatter, ring_advance_, counter_add_.  Both write the same bytes.

    `DeviceVectorEnv` replaces `env.state` on every eager step, so the graph
    owns the carry: `carry` [N, O] holds the live state before a replay (the
    sampler copies it in) and after it.  Keyed (steps, cuts,
    start_with_reset, mode) by the sampler.  Philox offsets (both bodies,
    `GraphedRollout`'s layout): action of step t at `t + ctr` (action seed),
    dynamics noise at `2t + ctr`, autoreset at `2t + 1 + ctr`, epoch reset at
    `2 * steps + ctr` (env seed); the counter advances by 2 * steps + 1.
    Warm-up leaves no trace: the counter, the carry and both ring scalars are
    restored by `_CapturedLoop`, the ring rows the warm-up runs wrote are put
    back here."""

    def __init__(self, policy, env, buffer, steps: int, cuts: Tuple[int, ...],
                 start_with_reset: bool, mode: str, ctr: torch.Tensor):
        ext = ops._load_extension()
        N, O, A = env.num_envs, int(env.A.shape[0]), int(env.B.shape[0])
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
        storage, write_dev, size_dev = buffer.device_ring(O, (A,))
        env_seed = env._philox_seed
        base_seed = torch.initial_seed()
        compute_bf16 = ops.compute_bf16()
        low, high = _scalar_bounds(env.action_space) or (0.0, 0.0)
        if mode == COLLECT_NOISED:
            weights, biases, acts = _extract_layers(fop._mlp_of(policy.base_policy))
            weights, biases = list(weights), list(biases)
            action_seed = (base_seed ^ _NOISE_SALT) & 0x7FFFFFFFFFFFFFFF
            noise_scale = float(policy.action_noise_scale)
            limit = float(policy.action_limit)
            dummy_log_std = torch.zeros(A, device=dev)
        else:
            weights, biases, acts = [], [], []
            action_seed = (base_seed ^ _UNIFORM_SALT) & 0x7FFFFFFFFFFFFFFF
            noise_scale, limit = 0.0, 0.0

        self.fused = synthetic_collect_fused_eligible(policy, env, cuts)
        wide_threads = collect_wide_threads()

        if self.fused:
            self.carry = torch.zeros(N, O, device=dev)

            def body():
                ext.synthetic_collect_fused(
                    weights, biases, acts, _COLLECT_MODE_CODE[mode], noise_scale,
                    limit, low, high, action_seed, env_seed, env.A, env.B, env.w,
                    env.noise, list(cuts), start_with_reset, self.ctr, self.carry,
                    steps, storage, write_dev, size_dev, self.seg_returns,
                    wide_threads,
                )
                ext.ring_advance_(write_dev, size_dev, n, cap)
                ext.counter_add_(self.ctr, 2 * steps + 1)
        else:
            self.obs_full = torch.zeros(steps + 1, N, O, device=dev)
            self.act_buf = torch.zeros(steps, N, A, device=dev)
            self.rew_buf = torch.zeros(steps, N, device=dev)
            self.cut_final = torch.zeros(max(len(cuts), 1), N, O, device=dev)
            self.carry = self.obs_full[steps]
            cset = {c: j for j, c in enumerate(cuts)}
            cut_slot = torch.tensor([cset.get(t, -1) for t in range(steps)],
                                    dtype=torch.int32, device=dev)

            def body():
                if start_with_reset:
                    ext.synthetic_env_reset(N, O, env.A, env_seed, 2 * steps,
                                            self.ctr, self.obs_full[0])
                else:
                    self.obs_full[0].copy_(self.obs_full[steps])
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
                    ext.synthetic_env_step(
                        self.obs_full[t], self.act_buf[t], env.A, env.B, env.w,
                        env.noise, env_seed, 2 * t, do_reset, self.ctr,
                        self.obs_full[t + 1],
                        self.cut_final[cset[t]] if do_reset else self.obs_full[t + 1],
                        self.rew_buf[t],
                    )
                ext.replay_scatter(self.obs_full, self.act_buf, self.rew_buf,
                                   self.cut_final, cut_slot, len(cuts), storage,
                                   write_dev, size_dev, self.seg_returns)
                ext.ring_advance_(write_dev, size_dev, n, cap)
                # past every offset used: env 2t / 2t+1 (t<steps), reset
                # 2*steps, action t (t<steps)
                ext.counter_add_(self.ctr, 2 * steps + 1)

        # the two warm-up runs write ring rows [write, write + 2n): keep what
        # they held, so warm-up never costs a stored transition
        touched = (buffer._write + torch.arange(min(2 * n, cap), device=dev)) % cap
        kept = [t[touched] for t in storage]
        self.loop = fop._CapturedLoop(
            body, [self.ctr, self.carry, write_dev, size_dev])
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


def pendulum_eval_fused_eligible(policy) -> bool:
    """pendulum_eval_fused (eval_kernels.hip) takes the evaluation: fp32
    parameters, a net [3, ..., 1] within the binding's own limits, one fp32
    log_std for a Gaussian policy."""
    mode = pendulum_eval_mode(policy)
    if mode is None:
        return False
    if mode == EVAL_GAUSSIAN and (policy.log_std.numel() != 1
                                  or policy.log_std.dtype != torch.float32):
        return False
    ext = ops._load_extension()
    weights, biases, _ = _extract_layers(fop._mlp_of(policy))
    return _fused_gate(weights, biases, ext.pendulum_eval_fused_limits(),
                       ext.pendulum_eval_fused_lds_bytes, 3, 1,
                       default=eval_fused_default("pendulum"))


def cartpole_eval_fused_eligible(policy) -> bool:
    """cartpole_eval_fused (eval_kernels.hip) takes the evaluation: fp32
    parameters, a categorical net [4, ..., n_act] with every width <= 64,
    within the binding's own limits."""
    if fop._policy_kind(policy) != "categorical":
        return False
    mlp = fop._mlp_of(policy)
    if mlp is None or _extract_layers(mlp) is None:
        return False
    ext = ops._load_extension()
    weights, biases, _ = _extract_layers(mlp)
    return _fused_gate(weights, biases, ext.cartpole_eval_fused_limits(),
                       ext.cartpole_eval_fused_lds_bytes, 4,
                       default=eval_fused_default("cartpole"))


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
    the counter bumps.  Multi-kernel body: `_pendulum_epoch` without cuts on
    a private state tensor (copied to `init_state` after the reset), the
    action being the mean itself or a Gaussian sample around it, then
    episode_reduce and the counter bumps; it keeps `act_buf` [horizon, N, 1].
    Both write the same bytes to `returns`, `lengths` and `init_state`."""

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
            fin_scratch = torch.zeros(N, 3, device=dev)
            self._means: List[torch.Tensor] = []

            def body():
                means = []

                def action(t):
                    mean = ext.mlp_forward(self.obs_full[t], weights, biases,
                                           acts, False, compute_bf16)[0]
                    if not gaussian:
                        means.append(mean)  # the deterministic action itself
                        return mean
                    ext.gaussian_sample(mean, log_std.data, policy_seed, t,
                                        -1.0, -1.0, self.ctr, self._act_buf[t])
                    return self._act_buf[t]

                _pendulum_epoch(ext, self.state, env_seed, horizon, (), action,
                                (0, self.reset_ctr, True), self.ctr,
                                self.obs_full, self.rew_buf, None, fin_scratch,
                                after_reset=lambda: self.init_state.copy_(self.state))
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
    counter bumps.  Multi-kernel body: `_cartpole_epoch` (with autoreset) on
    private carry tensors (state copied to `init_state` after the reset),
    episode_reduce over each row's first episode, the counter bumps; it
    keeps `act_buf` [horizon, N].  Both write the same bytes to `returns`,
    `lengths` and `init_state`."""

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
            # the successor rows are unused: every step writes the same one
            finals = [torch.zeros(N, 4, device=dev)] * horizon

            def body():
                _cartpole_epoch(
                    ext, (weights, biases, acts), (policy_seed, env_seed),
                    self.state, self.elapsed, horizon, horizon,
                    (0, self.reset_ctr), self.ctr, self.obs_full, finals,
                    self.act_buf, self.rew_buf, self.done_buf,
                    after_reset=lambda: self.init_state.copy_(self.state),
                )
                ext.episode_reduce(self.rew_buf, self.done_buf, self.returns,
                                   self.lengths)
                self._bump(ext)

        self._capture(body)
