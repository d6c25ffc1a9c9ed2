"""DeviceReplaySampler off the GPU: the fallback is DeviceSampler's eager
loop bit for bit, `ReplayBuffer.add_experience` honours the stored-in marker,
and host adds keep the device write mirror in step."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from rl_replicas_amd.envs import DevicePendulumEnv
from rl_replicas_amd.experience import Experience
from rl_replicas_amd.networks import MLP
from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
from rl_replicas_amd.replay_buffer import ReplayBuffer
from rl_replicas_amd.samplers import DeviceReplaySampler, DeviceSampler
from rl_replicas_amd.utils import add_noise_to_get_action

N, STEPS, HORIZON, CAP = 5, 6, 4, 100
KEYS = ("observations", "actions", "rewards", "next_observations", "dones")


def _world(replay: bool):
    torch.manual_seed(7)
    np.random.seed(7)
    env = DevicePendulumEnv(N, device="cpu", max_episode_steps=HORIZON)
    buf = ReplayBuffer(CAP)
    net = MLP([3, 32, 1], activation_function=nn.ReLU, output_activation_function=nn.Tanh)
    det = DeterministicPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3))
    noised = add_noise_to_get_action(det, env.action_space, 0.1)
    if replay:
        sampler = DeviceReplaySampler(env, buf, seed=3)
    else:
        sampler = DeviceSampler(env, seed=3, is_continuous=True)
    return env, buf, sampler, RandomPolicy(env.action_space), noised


def _numpy_experience(n, value):
    obs = [[np.full(3, value + i, dtype=np.float32) for i in range(n)]]
    return Experience(
        observations=obs,
        actions=[[np.full(1, value, dtype=np.float32) for _ in range(n)]],
        rewards=[[float(-i) for i in range(n)]],
        last_observations=[np.full(3, value + n, dtype=np.float32)],
        dones=[[False] * (n - 1) + [True]],
        episode_returns=[0.0],
        episode_lengths=[n],
    )


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
    for k in KEYS:
        assert torch.equal(buf_r._storage[k][: buf_r.current_size],
                           buf_d._storage[k][: buf_d.current_size]), k
    assert env_r._elapsed == env_d._elapsed
    assert torch.equal(env_r.state, env_d.state)
    for a, b in zip(exps_r, exps_d):
        assert a.episode_returns == b.episode_returns
        assert a.episode_lengths == b.episode_lengths
        assert all(np.array_equal(x, y) for x, y in zip(a.dones, b.dones))


def test_sampler_is_continuous_and_exported():
    import rl_replicas_amd.samplers as samplers

    env, buf, sampler, _, _ = _world(True)
    assert "DeviceReplaySampler" in samplers.__all__
    assert isinstance(sampler, DeviceSampler) and sampler.is_continuous
    assert sampler.replay_buffer is buf


def test_marker_contract():
    own, other = ReplayBuffer(16), ReplayBuffer(16)
    own.add_experience(_numpy_experience(4, 1.0))  # unmarked: stored as before
    assert len(own) == 4 and own._write == 4
    assert own._storage["dones"][:4].tolist() == [0.0, 0.0, 0.0, 1.0]
    before = {k: v.clone() for k, v in own._storage.items()}

    marked = _numpy_experience(4, 9.0)
    marked.stored_in_buffer = own
    own.add_experience(marked)  # already stored: nothing moves
    assert len(own) == 4 and own._write == 4
    for k in KEYS:
        assert torch.equal(own._storage[k][:4], before[k][:4])
    with pytest.raises(ValueError, match="another"):
        other.add_experience(marked)
    assert len(other) == 0 and other._storage is None


def test_host_add_moves_the_write_mirror_when_there_is_one():
    buf = ReplayBuffer(8)
    buf.add_experience(_numpy_experience(3, 1.0))
    assert buf._write_dev is None and buf._size_dev is None  # no-op on the CPU
    # a mirror, once there, follows every host-side move, wrap included
    buf._write_dev = torch.full((1,), -1, dtype=torch.int64)
    buf.add_experience(_numpy_experience(3, 2.0))
    assert int(buf._write_dev) == buf._write == 6
    buf._add_flat_tensors({  # the tensor route moves it too
        "observations": torch.zeros(4, 3), "actions": torch.zeros(4, 1),
        "rewards": torch.zeros(4), "next_observations": torch.zeros(4, 3),
        "step_dones": torch.zeros(4),
    })
    assert int(buf._write_dev) == buf._write == 2 and len(buf) == 8
    buf.advance_host(3)  # the host side of a device-side write
    assert buf._write == 5 and len(buf) == 8
