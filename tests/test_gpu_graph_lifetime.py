"""A captured graph keeps every buffer its body closed over (gpu-marked).

`_CapturedLoop` holds the body it captured, so a tensor that only the body's
closure references lives as long as the graph that reads or writes its
address.  The multi-kernel bodies (RL_REPLICAS_AMD_ROLLOUT_FUSED=0) have such
tensors: `fin_scratch` (written by every non-cut env step), `cut_slot` (read
by replay_scatter) and `dummy_log_std` (read by gaussian_sample in noised
mode).

Per class: build the graph, collect garbage, allocate 64 sentinel tensors at
each of those three byte sizes (the allocator hands out whatever the graph let
go of), replay, and check that (1) no sentinel tensor was written and (2) the
outputs equal those of an identically seeded second graph replayed with
nothing allocated in between (an overwritten `cut_slot` / `dummy_log_std`
changes what is stored).  Both hold by construction once the loop keeps its
body, whatever the allocator does.

8 envs, 4 steps, cuts (1,): a cut step and non-cut steps both occur.  Nets
[3, 16, 1]; CartPole's observation is 4 wide, so its net is [4, 16, 2]."""
import gc

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
N = 8
STEPS = 4
CUTS = (1,)
RING_CAP = 256
ENV_SEED = 5
N_SENTINELS = 64


def _gaussian_policy():
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import GaussianPolicy

    net = MLP([3, 16, 1]).to(DEVICE)
    log_std = nn.Parameter(-0.5 * torch.ones(1, device=DEVICE))
    params = list(net.parameters()) + [log_std]
    return GaussianPolicy(net, ops.make_adam(params, lr=3e-4), log_std)


def _pendulum_env():
    from rl_replicas_amd.envs import DevicePendulumEnv

    env = DevicePendulumEnv(N, device=DEVICE)
    env.seed(ENV_SEED)
    return env


def _build_rollout(fr):
    policy, env = _gaussian_policy(), _pendulum_env()
    g = fr.GraphedPendulumRollout(policy, env, STEPS, CUTS, True,
                                  fr.make_counter(DEVICE))
    return g, lambda: [g.obs_full, g.act_buf, g.rew_buf, g.cut_final], (policy, env)


def _build_collect(fr, mode):
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
    from rl_replicas_amd.replay_buffer import ReplayBuffer
    from rl_replicas_amd.utils import add_noise_to_get_action

    env = _pendulum_env()
    buf = ReplayBuffer(RING_CAP, device=DEVICE)
    if mode == fr.COLLECT_NOISED:
        net = MLP([3, 16, 1], activation_function=nn.ReLU,
                  output_activation_function=nn.Tanh).to(DEVICE)
        det = DeterministicPolicy(net, ops.make_adam(net.parameters(), lr=1e-3))
        policy = add_noise_to_get_action(det, env.action_space, 0.1)
    else:
        policy = RandomPolicy(env.action_space)
    assert fr.pendulum_collect_mode(policy, env) == mode
    storage, _, _ = buf.device_ring(3, (1,))
    for t in storage:  # torch.empty storage may hold NaNs
        t.zero_()
    g = fr.GraphedPendulumCollect(policy, env, buf, STEPS, CUTS, True, mode,
                                  fr.make_counter(DEVICE))
    return (g, lambda: [t[: N * STEPS] for t in storage] + [g.seg_returns],
            (policy, env, buf))


def _build_pendulum_eval(fr):
    policy = _gaussian_policy()
    g = fr.GraphedPendulumEval(policy, N, STEPS, ENV_SEED, fr.make_counter(DEVICE),
                               fr.make_counter(DEVICE))
    return g, lambda: [g.returns, g.lengths, g.init_state], (policy,)


def _build_cartpole_eval(fr):
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import CategoricalPolicy

    net = MLP([4, 16, 2]).to(DEVICE)
    policy = CategoricalPolicy(net, ops.make_adam(net.parameters(), lr=3e-4))
    g = fr.GraphedCartPoleEval(policy, N, STEPS, ENV_SEED, fr.make_counter(DEVICE),
                               fr.make_counter(DEVICE))
    return g, lambda: [g.returns, g.lengths, g.init_state], (policy,)


# A builder returns the graph, its outputs and what the graph's user owns
# (policy, env, ring): those stay alive here as they do in a sampler, so
# only the graph's own buffers are at stake.
# case -> (builder, observation width: fin_scratch is [N, width] fp32)
CASES = {
    "pendulum_rollout": (_build_rollout, 3),
    "pendulum_collect_noised": (lambda fr: _build_collect(fr, fr.COLLECT_NOISED), 3),
    "pendulum_collect_uniform": (lambda fr: _build_collect(fr, fr.COLLECT_UNIFORM), 3),
    "pendulum_eval": (_build_pendulum_eval, 3),
    "cartpole_eval": (_build_cartpole_eval, 4),
}


def _sentinels(obs_width):
    """64 tensors at each byte size of a buffer a body may hold alone:
    fin_scratch [N, width] fp32, cut_slot [STEPS] int32, dummy_log_std [1]
    fp32."""
    out = []
    for _ in range(N_SENTINELS):
        out.append(torch.full((N, obs_width), -7.0, device=DEVICE))
        out.append(torch.full((STEPS,), -7, dtype=torch.int32, device=DEVICE))
        out.append(torch.full((1,), -7.0, device=DEVICE))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_replay_touches_only_what_the_graph_owns(monkeypatch, case):
    from rl_replicas_amd.ops import fused_rollout as fr

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "0")
    build, obs_width = CASES[case]

    torch.manual_seed(77)
    g, outputs, owners = build(fr)
    assert not g.fused
    gc.collect()
    sentinels = _sentinels(obs_width)
    g.replay()
    torch.cuda.synchronize()
    dirty = [i for i, t in enumerate(sentinels) if not (t == -7).all()]
    got = [t.clone() for t in outputs()]

    del sentinels
    torch.manual_seed(77)
    g2, outputs2, owners2 = build(fr)
    assert not g2.fused
    g2.replay()
    torch.cuda.synchronize()
    want = outputs2()

    assert not dirty, f"the replay wrote into sentinel tensors {dirty}"
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"output {i} differs from an undisturbed graph's"
    assert any(t.abs().sum() > 0 for t in got)  # the replay stored something
