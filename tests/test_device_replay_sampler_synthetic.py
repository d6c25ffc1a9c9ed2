"""DeviceReplaySampler over a synthetic DeviceVectorEnv off the GPU: the
sampler is DeviceSampler's eager loop bit for bit, and the off-policy
benchmark builder hands it out for every device-mode env."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

from rl_replicas_amd.envs import DeviceVectorEnv
from rl_replicas_amd.networks import MLP
from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
from rl_replicas_amd.replay_buffer import ReplayBuffer
from rl_replicas_amd.samplers import DeviceReplaySampler, DeviceSampler
from rl_replicas_amd.utils import add_noise_to_get_action

N, STEPS, HORIZON, CAP = 5, 6, 4, 100
ENV_ID, O, A = "Hopper-v4", 11, 3
KEYS = ("observations", "actions", "rewards", "next_observations", "dones")


def _world(replay: bool):
    torch.manual_seed(7)
    np.random.seed(7)
    env = DeviceVectorEnv(ENV_ID, N, device="cpu", max_episode_steps=HORIZON)
    buf = ReplayBuffer(CAP)
    net = MLP([O, 32, A], activation_function=nn.ReLU, output_activation_function=nn.Tanh)
    det = DeterministicPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3))
    noised = add_noise_to_get_action(det, env.action_space, 0.1)
    if replay:
        sampler = DeviceReplaySampler(env, buf, seed=3)
    else:
        sampler = DeviceSampler(env, seed=3, is_continuous=True)
    return env, buf, sampler, RandomPolicy(env.action_space), noised


def test_cpu_fallback_equals_device_sampler():
    runs = {}
    for replay in (True, False):
        env, buf, sampler, uniform, noised = _world(replay)
        exps = []
        for policy in (uniform, uniform, noised):
            exp = sampler.sample(N * STEPS, policy)
            # the fallback: a flat cache, no marker, stored the usual way
            assert getattr(exp, "stored_in_buffer", None) is None
            assert "next_observations" in exp.to_flat_batch()
            buf.add_experience(exp)
            exps.append(exp)
        assert not sampler._graphs
        runs[replay] = (env, buf, exps)
    (env_r, buf_r, exps_r), (env_d, buf_d, exps_d) = runs[True], runs[False]
    assert buf_r._write == buf_d._write == 3 * N * STEPS
    assert buf_r.current_size == buf_d.current_size == 3 * N * STEPS
    assert buf_r._storage["observations"].shape == (CAP, O)
    assert buf_r._storage["actions"].shape == (CAP, A)
    for k in KEYS:
        assert torch.equal(buf_r._storage[k][: buf_r.current_size],
                           buf_d._storage[k][: buf_d.current_size]), k
    assert env_r._elapsed == env_d._elapsed
    assert torch.equal(env_r.state, env_d.state)
    for a, b in zip(exps_r, exps_d):
        assert a.episode_returns == b.episode_returns
        assert a.episode_lengths == b.episode_lengths
        assert all(np.array_equal(x, y) for x, y in zip(a.dones, b.dones))


def test_build_off_policy_hands_out_the_replay_sampler():
    bench_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "benchmarks")
    sys.path.insert(0, bench_dir)
    try:
        from common import build_off_policy
    finally:
        sys.path.remove(bench_dir)
    env, sampler, policy, exploration, qs, buffer, _ = build_off_policy(
        "Hopper-v4", 0, "cpu", 2, twin=True, env_mode="device")
    assert isinstance(env, DeviceVectorEnv)
    assert isinstance(sampler, DeviceReplaySampler) and sampler.is_continuous
    assert sampler.replay_buffer is buffer and sampler.env is env
    assert len(qs) == 2
    exp = sampler.sample(2 * STEPS, exploration)
    buffer.add_experience(exp)
    assert len(buffer) == 2 * STEPS
    assert buffer._storage["observations"].shape[1] == O
