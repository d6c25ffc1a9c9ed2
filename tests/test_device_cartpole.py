"""DeviceCartPoleEnv + DeviceEpisodicSampler on the CPU (torch fp64 path):
dynamics against the numpy env, truncation/autoreset semantics against
VectorEnv, the sampler's episode structure on a scripted done pattern,
batch parity with the numpy flat cache, and PPO learning."""
import math
import tempfile

import numpy as np
import pytest
import torch

from rl_replicas_amd import envs
from rl_replicas_amd.algorithms import PPO
from rl_replicas_amd.envs import CartPoleEnv, DeviceCartPoleEnv, VectorEnv
from rl_replicas_amd.experience import Experience
from rl_replicas_amd.networks import MLP
from rl_replicas_amd.policies import CategoricalPolicy
from rl_replicas_amd.samplers import DeviceEpisodicSampler, VectorSampler
from rl_replicas_amd.value_function import ValueFunction


def _models(seed, hidden=(64, 64)):
    torch.manual_seed(seed)
    pnet = MLP([4, *hidden, 2])
    policy = CategoricalPolicy(pnet, torch.optim.Adam(pnet.parameters(), lr=3e-4))
    vnet = MLP([4, *hidden, 1])
    vf = ValueFunction(vnet, torch.optim.Adam(vnet.parameters(), lr=1e-3))
    return policy, vf


class TestDynamics:
    def test_matches_numpy_step(self):
        """N=37, 200 steps, random actions: state within 1e-12 of
        CartPoleEnv._step_b and terminated flags equal at every step (reset
        states are copied across at each done)."""
        N, steps = 37, 200
        torch.manual_seed(0)
        env = DeviceCartPoleEnv(N, device="cpu", max_episode_steps=None)
        env.reset(seed=3)
        ref = CartPoleEnv()
        ref.state = env.state.numpy().copy()
        rng = np.random.default_rng(5)
        worst = 0.0
        n_term = 0
        for _ in range(steps):
            actions = rng.integers(0, 2, size=N)
            _, _, terminated = ref._step_b(actions)
            _, _, done, final_obs = env.step(torch.as_tensor(actions))
            done = done.numpy()
            assert np.array_equal(done, terminated)
            ref32 = ref.state.astype(np.float32)
            assert (np.abs(final_obs.numpy() - ref32) <= np.spacing(np.abs(ref32))).all()
            live = ~done
            worst = max(worst, float(np.abs(env.state.numpy()[live] - ref.state[live]).max()))
            n_term += int(done.sum())
            ref.state[done] = env.state.numpy()[done]
        print(f"max abs state difference {worst:.3e}, {n_term} terminations")
        assert n_term > 0
        assert worst <= 1e-12


class TestSemantics:
    def test_truncation_and_reset_match_vector_env(self):
        """Same states and actions through VectorEnv and the device env:
        terminated/truncated/done, elapsed and final_obs agree; done rows
        restart inside (-0.05, 0.05) with elapsed 0."""
        N, horizon = 6, 4
        venv = VectorEnv("CartPole-v1", N)
        venv.spec.max_episode_steps = horizon
        venv.reset(seed=0)
        env = DeviceCartPoleEnv(N, device="cpu", max_episode_steps=horizon)
        env.reset(seed=1)
        start = np.zeros((N, 4))
        start[0] = [2.39, 1.0, 0.0, 0.0]   # terminates on x at step 1
        start[1] = [0.0, 0.0, 0.205, 1.0]  # terminates on theta at step 1
        venv.env.state = start.copy()
        env.state.copy_(torch.from_numpy(start))
        rng = np.random.default_rng(2)
        saw_trunc = saw_term = False
        for t in range(10):
            actions = rng.integers(0, 2, size=N)
            pre_elapsed = env.elapsed.numpy().copy()
            _, _, terminated, truncated, v_final = venv.step(actions)
            obs, reward, done, final_obs = env.step(torch.as_tensor(actions))
            done = done.numpy()
            assert np.array_equal(done, terminated | truncated)
            expect_trunc = (pre_elapsed + 1 >= horizon) & ~terminated
            assert np.array_equal(truncated, expect_trunc)
            np.testing.assert_allclose(final_obs.numpy(), v_final, rtol=0, atol=1e-6)
            assert np.array_equal(env.elapsed.numpy(), venv._elapsed)
            assert (env.elapsed.numpy()[done] == 0).all()
            st = env.state.numpy()
            assert (np.abs(st[done]) < 0.05).all()
            # obs is the post-autoreset state; final_obs the pre-reset successor
            np.testing.assert_array_equal(obs.numpy(), st.astype(np.float32))
            if done.any():
                assert (np.abs(final_obs.numpy()[done]) != np.abs(obs.numpy()[done])).any()
            assert torch.equal(reward, torch.ones(N))
            saw_trunc |= bool(truncated.any())
            saw_term |= bool(terminated.any())
            # keep the two envs on the same states after their own resets
            venv.env.state = st.copy()
        assert saw_trunc and saw_term

    def test_reset_states_in_range_and_seeded(self):
        env = DeviceCartPoleEnv(64, device="cpu")
        a = env.reset(seed=9).clone()
        assert env.state.dtype == torch.float64 and env.elapsed.dtype == torch.int32
        assert (env.state.abs() < 0.05).all() and (env.elapsed == 0).all()
        assert torch.equal(a, env.state.float())
        b = env.reset(seed=9)
        assert torch.equal(a, b)
        assert not torch.equal(a, env.reset())

    def test_lockstep_env_still_rejects_cartpole(self):
        with pytest.raises(TypeError):
            envs.DeviceVectorEnv("CartPole-v1", 2)


class _ScriptedEnv:
    """Device-env protocol with a scripted done pattern.  The observation
    of instance i after k steps is [i, k]; a done step autoresets to
    [i, 100 + k] and reports the pre-reset successor in final_obs."""

    def __init__(self, pattern):
        self.pattern = np.asarray(pattern, dtype=bool)  # [total_steps, N]
        self.num_envs = self.pattern.shape[1]
        self.device = torch.device("cpu")
        self.t = 0
        self.resets = 0

    def seed(self, seed):
        pass

    def reset(self, *, seed=None):
        self.resets += 1
        N = self.num_envs
        self.obs = torch.stack([torch.arange(N, dtype=torch.float32),
                                torch.full((N,), float(self.t))], dim=1)
        return self.obs.clone()

    def step(self, actions):
        done = torch.from_numpy(self.pattern[self.t])
        self.t += 1
        N = self.num_envs
        ids = torch.arange(N, dtype=torch.float32)
        final = torch.stack([ids, torch.full((N,), float(self.t))], dim=1)
        fresh = torch.stack([ids, torch.full((N,), 100.0 + self.t)], dim=1)
        self.obs = torch.where(done[:, None], fresh, final)
        reward = ids + 1.0
        return self.obs.clone(), reward, done, final


class _ConstPolicy:
    def get_action_tensor(self, obs):
        return (obs[:, 1].long() % 2)


# steps x instances: instance 0 is done twice (t=1, t=3), instance 1 never,
# instance 2 on the last step
_PATTERN = [
    [0, 0, 0],
    [1, 0, 0],
    [0, 0, 0],
    [1, 0, 0],
    [0, 0, 1],
]


class TestSamplerStructure:
    def test_scripted_done_pattern(self):
        env = _ScriptedEnv(_PATTERN)
        sampler = DeviceEpisodicSampler(env, seed=0)
        exp = sampler.sample(15, _ConstPolicy())
        flat = exp.to_flat_batch()
        # instance-major episodes: i0 -> [0,1], [2,3], [4] ; i1 -> [0..4] ; i2 -> [0..4]
        assert flat["episode_offsets"].tolist() == [0, 2, 4, 5, 10, 15]
        assert flat["episode_dones"].tolist() == [True, True, False, False, True]
        assert exp.episode_lengths == [2, 2, 1, 5, 5]
        assert sum(exp.episode_lengths) == 15
        assert exp.episode_dones == [True, True, False, False, True]
        assert exp.episode_returns == [2.0, 2.0, 1.0, 10.0, 15.0]
        # done episodes bootstrap from final_obs (pre-reset successor),
        # cuts from the live observation
        assert flat["last_observations"].tolist() == [
            [0.0, 2.0], [0.0, 4.0], [0.0, 5.0], [1.0, 5.0], [2.0, 5.0]
        ]
        assert flat["observations"][:, 0].tolist() == [0.0] * 5 + [1.0] * 5 + [2.0] * 5
        assert flat["observations"][:, 1].tolist() == [
            0.0, 1.0, 102.0, 3.0, 104.0, 0.0, 1.0, 2.0, 3.0, 4.0, 0.0, 1.0, 2.0, 3.0, 4.0
        ]
        # true successors: the pre-reset one on done steps
        assert flat["next_observations"][:, 1].tolist() == [
            1.0, 2.0, 3.0, 4.0, 5.0, 1.0, 2.0, 3.0, 4.0, 5.0, 1.0, 2.0, 3.0, 4.0, 5.0
        ]
        assert flat["step_dones"].tolist() == [
            0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0
        ]
        assert flat["actions"].dtype == torch.int64 and flat["actions"].shape == (15,)
        assert flat["actions"].tolist() == [0, 1, 0, 1, 0] + [0, 1, 0, 1, 0] * 2
        assert flat["rewards"].tolist() == [1.0] * 5 + [2.0] * 5 + [3.0] * 5

    def test_default_resets_each_call(self):
        env = _ScriptedEnv(np.zeros((10, 3), dtype=bool))
        sampler = DeviceEpisodicSampler(env)
        sampler.sample(15, _ConstPolicy())
        flat = sampler.sample(15, _ConstPolicy()).to_flat_batch()
        assert env.resets == 2
        assert flat["observations"][0].tolist() == [0.0, 5.0]  # fresh reset obs

    def test_is_continuous_carries_state(self):
        env = _ScriptedEnv(np.zeros((10, 3), dtype=bool))
        sampler = DeviceEpisodicSampler(env, is_continuous=True)
        first = sampler.sample(15, _ConstPolicy()).to_flat_batch()
        flat = sampler.sample(15, _ConstPolicy()).to_flat_batch()
        assert env.resets == 1
        # the second call starts from the first call's live observation
        assert torch.equal(flat["observations"][0], first["last_observations"][0])
        assert flat["observations"][:5, 1].tolist() == [5.0, 6.0, 7.0, 8.0, 9.0]

    def test_rejects_indivisible_batch(self):
        with pytest.raises(ValueError):
            DeviceEpisodicSampler(_ScriptedEnv(_PATTERN)).sample(16, _ConstPolicy())


class TestBatchParity:
    def test_prepare_batch_tensor_path_matches_numpy_path(self):
        """_prepare_batch gives equal advantages/returns from the device flat
        cache and from the same rollout as a numpy Experience."""
        env = DeviceCartPoleEnv(8, device="cpu", max_episode_steps=10)
        sampler = DeviceEpisodicSampler(env, seed=11)
        policy, vf = _models(2, hidden=(32,))
        model = PPO(policy, vf, env, sampler)

        exp = sampler.sample(320, policy)
        flat_t = exp.to_flat_batch()
        assert flat_t["episode_dones"].any() and not flat_t["episode_dones"].all()
        batch_t = model._prepare_batch(exp)

        offs = flat_t["episode_offsets"].tolist()
        exp_np = Experience()
        for e in range(len(offs) - 1):
            lo, hi = offs[e], offs[e + 1]
            exp_np.observations.append(list(flat_t["observations"][lo:hi].numpy()))
            exp_np.actions.append(list(flat_t["actions"][lo:hi].numpy()))
            exp_np.rewards.append(flat_t["rewards"][lo:hi].tolist())
            exp_np.dones.append([False] * (hi - lo - 1) + [bool(flat_t["episode_dones"][e])])
            exp_np.last_observations.append(flat_t["last_observations"][e].numpy())
            exp_np.episode_lengths.append(hi - lo)
        batch_np = model._prepare_batch(exp_np)

        for key in ("advantages", "discounted_returns"):
            torch.testing.assert_close(batch_t[key], batch_np[key], rtol=1e-5, atol=1e-5)
        assert torch.equal(batch_t["actions"], batch_np["actions"])

    def test_same_structure_as_vector_sampler(self):
        """Episode bookkeeping equals VectorSampler's own on an identical
        done pattern: feed VectorSampler's step-major record through
        _build_experience."""
        torch.manual_seed(0)
        venv = VectorEnv("CartPole-v1", 5)
        policy, _ = _models(1, hidden=(16,))
        vs = VectorSampler(venv, seed=4)
        steps = 60
        ref = vs.sample(5 * steps, policy).to_flat_batch()
        env = DeviceCartPoleEnv(5, device="cpu")
        sampler = DeviceEpisodicSampler(env)
        # rebuild the step-major buffers from the flat (instance-major) record
        offs = ref["episode_offsets"]
        done_flat = np.zeros(5 * steps, dtype=np.uint8)
        done_flat[(offs[1:] - 1)[ref["episode_dones"]]] = 1
        to_steps = lambda a: torch.as_tensor(a).view(5, steps, *a.shape[1:]).transpose(0, 1).contiguous()
        final = np.zeros((5 * steps, 4), dtype=np.float32)
        final[offs[1:] - 1] = ref["last_observations"]
        sampler._obs = torch.as_tensor(ref["last_observations"][
            np.searchsorted(offs, np.arange(1, 6) * steps) - 1])
        exp = sampler._build_experience(
            steps, to_steps(ref["observations"]), to_steps(ref["actions"]),
            to_steps(ref["rewards"]), to_steps(done_flat), to_steps(final))
        flat = exp.to_flat_batch()
        assert flat["episode_offsets"].tolist() == offs.tolist()
        assert flat["episode_dones"].tolist() == ref["episode_dones"].tolist()
        np.testing.assert_array_equal(flat["last_observations"].numpy(), ref["last_observations"])
        np.testing.assert_array_equal(flat["observations"].numpy(), ref["observations"])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ppo_learns(seed):
    """CategoricalPolicy [4,64,64,2], value net [4,64,64,1], 16 envs, 12
    epochs of 2048 steps: the mean completed-episode length over epochs
    10-12 is >= 2x that of epoch 1.  (The host VectorSampler path gives
    4.0x-6.0x at this configuration; 2x is a floor against a broken rollout,
    not a performance claim.)  The sampler is continuous: with a fresh
    reset per epoch each instance sees only 128 steps, so a policy that has
    learnt completes no episode at all and the mean is undefined."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = DeviceCartPoleEnv(16, device="cpu")
    sampler = DeviceEpisodicSampler(env, seed=seed, is_continuous=True)
    policy, vf = _models(seed)
    model = PPO(policy, vf, env, sampler)
    model._begin_learn(tempfile.mkdtemp())
    means = []
    for _ in range(12):
        exp = sampler.sample(2048, policy)
        lengths = np.asarray(exp.episode_lengths)[np.asarray(exp.episode_dones)]
        means.append(float(lengths.mean()))
        model.train(exp)
    first, last = means[0], float(np.mean(means[9:12]))
    print(f"seed {seed}: epoch-1 mean length {first:.1f}, epochs 10-12 {last:.1f}, "
          f"ratio {last / first:.2f}")
    assert math.isfinite(last) and last >= 2.0 * first
