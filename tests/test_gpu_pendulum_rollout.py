"""The device Pendulum rollout (gpu-marked): the stand-alone step / reset
kernels against the numpy env, and the persistent kernel
pendulum_rollout_fused against the multi-kernel graph body with torch.equal
(both inline the row code of rollout_steps.h and use the same Philox
offsets, so no tolerance applies).

N = 5 (less than one 16-row tile), 16 (exactly one), 37 (two tiles and a
5-row tail).  Nets [3,64,32,1] and [3,7,1], whose hidden dim is no multiple
of 4 or 16.  steps = 6 with horizon 4, so a lockstep cut falls inside the
epoch (after step 3); with is_continuous the second epoch cuts after steps
1 and 5.

Staged rows (kind = row % 7) put every branch of the transition at a known
place: torque clamp with the upper / lower speed clamp, the angle wrap from
either side, several turns, and two plain rows."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
NS = [5, 16, 37]
NETS = {"bench": [3, 64, 32, 1], "awkward": [3, 7, 1],
        # the layer-count ends of the shared forward: one layer (the output stays
        # in the first activation buffer) and five (MLP_MAX_LAYERS), ragged
        "one_layer": [3, 1], "five_layers": [3, 16, 24, 8, 40, 1]}
STEPS = 6
HORIZON = 4
CTR_BASE = 1 << 40
CUTS_FROM_RESET = (3,)
CUTS_CARRY = (1, 5)  # elapsed 2 after the first epoch


def _staged(n):
    """fp64 states [n,2] and fp32 actions [n,1]."""
    kinds = np.arange(n) % 7
    rows = np.array([
        [math.pi / 2, 7.9, 3.0],     # torque clamp, upper speed clamp
        [-math.pi / 2, -7.9, -3.0],  # torque clamp, lower speed clamp
        [4.0, 0.5, 1.5],             # wrap
        [-4.0, -0.5, -1.5],          # wrap
        [20.0, 1.0, 0.25],           # several turns
        [0.3, -0.2, -0.7],
        [3.0, 0.0, 2.5],
    ])
    state = rows[kinds, :2] + 1e-3 * np.arange(n)[:, None] * np.array([1.0, -1.0])
    actions = rows[kinds, 2:3].astype(np.float32)
    return state, actions


def _oracle(n):
    """One step of the numpy env from the staged rows, with the conditions
    that keep every row clear of a branch boundary asserted on it."""
    from rl_replicas_amd.envs import PendulumEnv

    state, actions = _staged(n)
    ref = PendulumEnv()
    ref.state = state.copy()
    obs, reward, _ = ref._step_b(actions)
    th, thdot = state.T
    u_raw = actions[:, 0].astype(np.float64)
    u = np.clip(u_raw, -2.0, 2.0)
    unclamped = thdot + (15.0 * np.sin(th) + 3.0 * u) * 0.05
    wrapped = (th + np.pi) % (2 * np.pi)
    assert (np.abs(np.abs(unclamped) - 8.0) >= 1e-6).all()
    assert (np.minimum(wrapped, 2 * np.pi - wrapped) >= 1e-6).all()
    assert (np.abs(np.abs(u_raw) - 2.0) >= 1e-6).all()
    # every branch is taken by some row
    assert (np.abs(unclamped) > 8.0).sum() == {5: 2, 16: 6, 37: 12}[n]
    assert (wrapped != th + np.pi).sum() == {5: 3, 16: 6, 37: 15}[n]
    assert (np.abs(u_raw) > 2.0).any()
    return state, actions, ref.state.copy(), obs, reward


def _ulp_close(got32, want64):
    want32 = np.asarray(want64).astype(np.float32)
    return (np.abs(got32 - want32) <= np.spacing(np.abs(want32))).all()


def _obs_of(state64):
    th, thdot = state64.T
    return np.stack([np.cos(th), np.sin(th), thdot], axis=1)


@pytest.mark.parametrize("do_reset", [False, True], ids=["step", "autoreset"])
@pytest.mark.parametrize("n", NS)
def test_step_kernel_matches_numpy(n, do_reset):
    from rl_replicas_amd.envs import DevicePendulumEnv

    state, actions, ref_state, ref_obs, ref_reward = _oracle(n)
    env = DevicePendulumEnv(n, device=DEVICE, max_episode_steps=HORIZON)
    env.reset(seed=3)
    carry = env.state
    env.state = torch.from_numpy(state)
    assert env.state is carry and env.state.dtype == torch.float64
    env._elapsed = HORIZON - 1 if do_reset else 0
    obs, reward, truncated, final_obs = env.step(torch.from_numpy(actions).to(DEVICE))
    torch.cuda.synchronize()
    assert truncated == do_reset
    assert env.state is carry and env.state.shape == (n, 2)
    new_state = env.state.cpu().numpy()
    obs, final_obs, reward = obs.cpu().numpy(), final_obs.cpu().numpy(), reward.cpu().numpy()
    assert obs.dtype == final_obs.dtype == reward.dtype == np.float32
    assert obs.shape == final_obs.shape == (n, 3) and reward.shape == (n,)
    # final_obs is the true successor either way
    assert _ulp_close(final_obs, ref_obs)
    assert _ulp_close(reward, ref_reward)
    if do_reset:
        assert (np.abs(new_state[:, 0]) < math.pi).all()
        assert (np.abs(new_state[:, 1]) < 1.0).all()
        assert env._elapsed == 0
    else:
        diff = np.abs(new_state - ref_state).max()
        print(f"n={n}: max abs state difference {diff:.3e}")
        assert diff <= 1e-12
        assert np.array_equal(obs, final_obs)
        assert env._elapsed == 1
    assert _ulp_close(obs, _obs_of(new_state))


def test_step_binding_checks_arguments():
    from rl_replicas_amd import ops

    ext = ops._load_extension()
    state = torch.zeros(5, 2, dtype=torch.float64, device=DEVICE)
    act = torch.zeros(5, 1, device=DEVICE)
    before = state.clone()
    with pytest.raises(RuntimeError):
        ext.pendulum_env_step(state.float(), act, False, 1, 0)
    with pytest.raises(RuntimeError):
        ext.pendulum_env_step(state, act[:4], False, 1, 0)
    with pytest.raises(RuntimeError):
        ext.pendulum_env_step(state, act, False, 1, 0, obs=torch.zeros(5, 2, device=DEVICE))
    with pytest.raises(RuntimeError):
        ext.pendulum_env_step(state, act, False, 1, 0,
                              offset_ctr=torch.zeros(1, dtype=torch.int32, device=DEVICE))
    with pytest.raises(RuntimeError):
        ext.pendulum_env_reset(torch.zeros(5, 4, dtype=torch.float64, device=DEVICE), 1, 0)
    torch.cuda.synchronize()
    assert torch.equal(state, before)  # nothing was launched
    # the device counter is added to the by-value offset
    c = torch.tensor([12345], dtype=torch.int64, device=DEVICE)
    a, b, d = state.clone(), state.clone(), state.clone()
    ext.pendulum_env_reset(a, 99, 3, offset_ctr=c)
    ext.pendulum_env_reset(b, 99, 3 + 12345)
    ext.pendulum_env_reset(d, 99, 3)
    assert torch.equal(a, b) and not torch.equal(a, d)


def test_reset_kernel_draws():
    from rl_replicas_amd.envs import DevicePendulumEnv

    n = 4096
    env = DevicePendulumEnv(n, device=DEVICE)
    obs = env.reset(seed=11)
    a = env.state.cpu().numpy().copy()
    assert a.dtype == np.float64 and a.shape == (n, 2)
    assert (np.abs(a[:, 0]) < math.pi).all() and (np.abs(a[:, 1]) < 1.0).all()
    assert _ulp_close(obs.cpu().numpy(), _obs_of(a))
    assert len(np.unique(a)) > 0.999 * a.size  # rows and components differ
    assert (a[0] != a[1]).all() and (a[:, 0] / math.pi != a[:, 1]).all()
    env.reset()
    b = env.state.cpu().numpy()
    assert (a != b).mean() > 0.999  # the next offset is another draw
    env.reset(seed=11)
    assert np.array_equal(env.state.cpu().numpy(), a)
    for k, width in ((0, 2 * math.pi), (1, 2.0)):
        bound = 5 * (width / math.sqrt(12)) / math.sqrt(n)
        print(f"component {k}: mean of {n} draws {a[:, k].mean():.3e}, bound {bound:.3e}")
        assert abs(a[:, k].mean()) <= bound


def _policy(dims, log_std=-0.5):
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import GaussianPolicy

    pnet = MLP(dims).to(DEVICE)
    ls = nn.Parameter(log_std * torch.ones(1, device=DEVICE))
    policy = GaussianPolicy(pnet, ops.make_adam(list(pnet.parameters()) + [ls], lr=3e-4), ls)
    return pnet, ls, policy


def _rollouts(monkeypatch, fused, dims, n_envs, continuous, epochs=2, mutate_before=None):
    """Run `epochs` sampler calls; per call a dict of the graph and clones
    of its buffers, the env carry and the counter."""
    from rl_replicas_amd.envs import DevicePendulumEnv
    from rl_replicas_amd.samplers import DeviceSampler

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1" if fused else "0")
    torch.manual_seed(77)
    env = DevicePendulumEnv(n_envs, device=DEVICE, max_episode_steps=HORIZON)
    pnet, ls, policy = _policy(dims)
    sampler = DeviceSampler(env, seed=5, is_continuous=continuous)
    carry = env.state
    out = []
    for e in range(epochs):
        if mutate_before == e:
            with torch.no_grad():  # every action becomes 1.25 +- e^-20
                for p in pnet.parameters():
                    p.zero_()
                list(pnet.parameters())[-1].fill_(1.25)
                ls.fill_(-20.0)
        exp = sampler.sample(n_envs * STEPS, policy)
        reset_epoch = e == 0 or not continuous
        if reset_epoch:
            cuts = CUTS_FROM_RESET
        else:  # horizon 4, 6 steps: the pattern has period 2 epochs
            cuts = CUTS_CARRY if e % 2 == 1 else CUTS_FROM_RESET
        g = sampler._graphs[(STEPS, cuts, reset_epoch)]
        torch.cuda.synchronize()
        assert env.state is carry
        out.append({
            "g": g, "exp": exp, "sampler": sampler, "cuts": cuts,
            "obs_full": g.obs_full.clone(), "act_buf": g.act_buf.clone(),
            "rew_buf": g.rew_buf.clone(),
            "finals": torch.stack(g.final_tensors()).clone(),
            "state": env.state.clone(), "ctr": int(sampler._graph_ctr.item()),
        })
    return out


KEYS = ("obs_full", "act_buf", "rew_buf", "finals", "state")


def _assert_same(f_run, p_run):
    for e, (f, p) in enumerate(zip(f_run, p_run)):
        assert f["g"].fused and not p["g"].fused
        assert f["ctr"] == p["ctr"] == CTR_BASE + (e + 1) * (STEPS + 1)
        for k in KEYS:
            assert torch.equal(f[k], p[k]), f"{k} differs in epoch {e}"


def _assert_invariants(r, n_envs):
    obs_full = r["obs_full"]
    assert obs_full.shape == (STEPS + 1, n_envs, 3)
    assert r["act_buf"].shape == (STEPS, n_envs, 1)
    assert r["state"].dtype == torch.float64 and r["state"].shape == (n_envs, 2)
    for k in KEYS:
        assert torch.isfinite(r[k]).all(), k
    norm = obs_full[..., 0].double() ** 2 + obs_full[..., 1].double() ** 2
    assert (norm - 1.0).abs().max() < 1e-6
    assert (obs_full[..., 2].abs() <= 8.0).all()
    assert (r["rew_buf"] <= 0).all()
    # the carry slot is the observation of the env's fp64 state
    assert torch.equal(obs_full[STEPS, :, 2], r["state"][:, 1].float())
    assert _ulp_close(obs_full[STEPS].cpu().numpy(), _obs_of(r["state"].cpu().numpy()))
    for j, c in enumerate(r["cuts"]):
        # a fresh draw follows each cut; the pre-reset successor is kept
        assert (obs_full[c + 1, :, 2].abs() <= 1.0).all()
        assert not torch.equal(r["finals"][j], obs_full[c + 1])
        n = r["finals"][j].double()
        assert ((n[:, 0] ** 2 + n[:, 1] ** 2) - 1.0).abs().max() < 1e-6


@pytest.mark.parametrize("continuous", [False, True], ids=["reset", "carry"])
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("n_envs", NS)
def test_fused_equals_multi_kernel_body(monkeypatch, n_envs, net, continuous):
    """Two consecutive epochs: every buffer, the cut finals, the env carry
    and the RNG counter are equal."""
    f = _rollouts(monkeypatch, True, NETS[net], n_envs, continuous)
    p = _rollouts(monkeypatch, False, NETS[net], n_envs, continuous)
    _assert_same(f, p)
    for r in f:
        _assert_invariants(r, n_envs)
    # the epochs draw fresh randomness
    assert not torch.equal(f[0]["act_buf"], f[1]["act_buf"])
    assert f[1]["g"].start_with_reset == (not continuous)
    if continuous:
        assert f[1]["cuts"] == CUTS_CARRY and f[1]["g"] is not f[0]["g"]
        # the second epoch starts from the first's carry
        assert torch.equal(f[1]["obs_full"][0], f[0]["obs_full"][STEPS])
        assert f[1]["sampler"].env._elapsed == 0
    else:
        assert f[1]["g"] is f[0]["g"]
        assert (f[1]["obs_full"][0, :, 2].abs() <= 1.0).all()
        assert not torch.equal(f[1]["obs_full"][0], f[0]["obs_full"][STEPS])
        assert f[1]["sampler"].env._elapsed == 2


def test_identically_seeded_runs_are_bit_equal(monkeypatch):
    a = _rollouts(monkeypatch, True, NETS["bench"], 37, True)
    b = _rollouts(monkeypatch, True, NETS["bench"], 37, True)
    for ra, rb in zip(a, b):
        assert ra["ctr"] == rb["ctr"]
        for k in KEYS:
            assert torch.equal(ra[k], rb[k])
        fa, fb = ra["exp"].to_flat_batch(), rb["exp"].to_flat_batch()
        for k in fa:
            assert torch.equal(fa[k], fb[k]), k


def test_weights_are_read_by_pointer(monkeypatch):
    """Parameters and log_std changed in place between replays of ONE graph:
    both routes see the change and stay equal."""
    f = _rollouts(monkeypatch, True, NETS["bench"], 37, False, epochs=3, mutate_before=1)
    p = _rollouts(monkeypatch, False, NETS["bench"], 37, False, epochs=3, mutate_before=1)
    _assert_same(f, p)
    assert len(f[0]["sampler"]._graphs) == 1 and f[2]["g"] is f[0]["g"]
    assert (f[0]["act_buf"] - 1.25).abs().max() > 0.1
    for e in (1, 2):
        assert (f[e]["act_buf"] - 1.25).abs().max() < 1e-6


def test_flat_cache_matches_graph_buffers(monkeypatch):
    n = 37
    for r in _rollouts(monkeypatch, True, NETS["bench"], n, True):
        flat = r["exp"].to_flat_batch()
        cuts = r["cuts"]
        assert torch.equal(flat["observations"].view(n, STEPS, 3),
                           r["obs_full"][:STEPS].transpose(0, 1))
        assert torch.equal(flat["actions"].view(n, STEPS, 1), r["act_buf"].transpose(0, 1))
        assert torch.equal(flat["rewards"].view(n, STEPS), r["rew_buf"].t())
        nxt = flat["next_observations"].view(n, STEPS, 3)
        dones = flat["step_dones"].view(n, STEPS)
        for t in range(STEPS):
            if t in cuts:  # the pre-reset successor, done = 1
                assert torch.equal(nxt[:, t], r["finals"][cuts.index(t)])
                assert (dones[:, t] == 1).all()
            else:
                assert torch.equal(nxt[:, t], r["obs_full"][t + 1])
                assert (dones[:, t] == 0).all()
        ends = [c + 1 for c in cuts]
        lengths = [b - a for a, b in zip([0] + ends, ends + ([STEPS] if ends[-1] < STEPS else []))]
        assert r["exp"].episode_lengths == lengths * n
        last = flat["last_observations"].view(n, len(lengths), 3)
        for j in range(len(cuts)):
            assert torch.equal(last[:, j], r["finals"][j])
        if len(lengths) > len(cuts):
            assert torch.equal(last[:, -1], r["obs_full"][STEPS])


def test_gate(monkeypatch):
    from rl_replicas_amd import ops
    from rl_replicas_amd.envs import DeviceVectorEnv, DevicePendulumEnv
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.ops import fused_rollout
    from rl_replicas_amd.policies import DeterministicPolicy
    from rl_replicas_amd.samplers import DeviceSampler

    # outside the tile limit: the multi-kernel body
    (r,) = _rollouts(monkeypatch, True, [3, 128, 1], 16, False, epochs=1)
    assert not r["g"].fused
    _assert_invariants(r, 16)

    env = DevicePendulumEnv(8, device=DEVICE)
    _, _, gauss = _policy([3, 16, 1])
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    assert fused_rollout.pendulum_supported(gauss, env)
    assert fused_rollout.pendulum_fused_eligible(gauss, env, (3,))
    assert not fused_rollout.pendulum_fused_eligible(gauss, env, tuple(range(17)))
    assert not fused_rollout.pendulum_supported(gauss, DevicePendulumEnv(8, device="cpu"))
    assert not fused_rollout.supported(gauss, env)  # the synthetic gate is unchanged
    denv = DeviceVectorEnv("HalfCheetah-v4", num_envs=8, device=DEVICE)
    assert not fused_rollout.pendulum_supported(gauss, denv)
    dnet = MLP([3, 16, 1], output_activation_function=nn.Tanh).to(DEVICE)
    det = DeterministicPolicy(dnet, ops.make_adam(dnet.parameters(), lr=1e-3))
    assert not fused_rollout.pendulum_supported(det, env)

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "0")
    assert fused_rollout.pendulum_supported(gauss, env)
    assert not fused_rollout.pendulum_fused_eligible(gauss, env, (3,))
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")

    # bf16 compute: the multi-kernel body, and it runs
    monkeypatch.setenv("RL_REPLICAS_AMD_COMPUTE_DTYPE", "bf16")
    assert not fused_rollout.pendulum_fused_eligible(gauss, env, (3,))
    (r,) = _rollouts(monkeypatch, True, NETS["bench"], 16, False, epochs=1)
    assert not r["g"].fused
    _assert_invariants(r, 16)
    monkeypatch.delenv("RL_REPLICAS_AMD_COMPUTE_DTYPE")

    # graphs disabled: the eager loop, one env kernel per step
    monkeypatch.setenv("RL_REPLICAS_AMD_DISABLE_GRAPHS", "1")
    assert not fused_rollout.pendulum_supported(gauss, env)
    torch.manual_seed(3)
    eenv = DevicePendulumEnv(16, device=DEVICE, max_episode_steps=HORIZON)
    sampler = DeviceSampler(eenv, seed=5, is_continuous=True)
    carry = eenv.state
    for want in ([4, 2], [2, 4]):
        exp = sampler.sample(16 * STEPS, gauss)
        assert not sampler._graphs
        assert exp.episode_lengths == want * 16
        assert eenv.state is carry
    flat = exp.to_flat_batch()
    assert torch.isfinite(flat["observations"]).all() and (flat["rewards"] <= 0).all()
    assert _ulp_close(sampler._obs.cpu().numpy(), _obs_of(eenv.state.cpu().numpy()))


def test_ppo_end_to_end(tmp_path):
    """PPO + GaussianPolicy + DeviceSampler through the default path: 3
    epochs x 400 steps at N = 20."""
    from rl_replicas_amd import ops
    from rl_replicas_amd.algorithms import PPO
    from rl_replicas_amd.envs import DevicePendulumEnv
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.samplers import DeviceSampler
    from rl_replicas_amd.value_function import ValueFunction

    torch.manual_seed(21)
    env = DevicePendulumEnv(20, device=DEVICE)
    pnet, ls, policy = _policy([3, 64, 32, 1])
    vnet = MLP([3, 64, 32, 1]).to(DEVICE)
    vf = ValueFunction(vnet, ops.make_adam(vnet.parameters(), lr=1e-3))
    sampler = DeviceSampler(env, seed=3, is_continuous=True)
    model = PPO(policy, vf, env, sampler, num_policy_gradients=2, num_value_gradients=2)
    model.learn(num_epochs=3, batch_size=400, output_dir=str(tmp_path))
    torch.cuda.synchronize()
    assert model.current_total_steps == 1200
    assert sampler._graphs  # the captured epoch, not the eager loop
    assert env._elapsed == 60
    for p in list(pnet.parameters()) + [ls] + list(vnet.parameters()):
        assert torch.isfinite(p).all()


def test_ddpg_epoch_on_the_eager_loop(tmp_path):
    """Off-policy use (a noised DeterministicPolicy) stays on the eager loop
    and steps the GPU env one kernel at a time."""
    from rl_replicas_amd import ops
    from rl_replicas_amd.algorithms import DDPG
    from rl_replicas_amd.envs import DevicePendulumEnv
    from rl_replicas_amd.evaluator import Evaluator
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy
    from rl_replicas_amd.q_function import QFunction
    from rl_replicas_amd.replay_buffer import ReplayBuffer
    from rl_replicas_amd.samplers import DeviceSampler

    torch.manual_seed(0)
    env = DevicePendulumEnv(10, device=DEVICE)
    pnet = MLP([3, 32, 1], activation_function=nn.ReLU,
               output_activation_function=nn.Tanh).to(DEVICE)
    policy = DeterministicPolicy(pnet, ops.make_adam(pnet.parameters(), lr=1e-3))
    qnet = MLP([4, 32, 1], activation_function=nn.ReLU).to(DEVICE)
    q = QFunction(qnet, ops.make_adam(qnet.parameters(), lr=1e-3))
    sampler = DeviceSampler(env, seed=3, is_continuous=True)
    model = DDPG(policy, RandomPolicy(env.action_space), q, env, sampler,
                 ReplayBuffer(1024, device=DEVICE), Evaluator(seed=4))
    model.learn(num_epochs=1, batch_size=50, minibatch_size=16, num_start_steps=0,
                num_steps_before_update=50, num_train_steps=2,
                num_evaluation_episodes=0, output_dir=str(tmp_path))
    torch.cuda.synchronize()
    assert model.current_total_steps == 50
    assert not sampler._graphs
    assert env._elapsed == 5 and env._philox_offset == 6  # one reset, five steps
    for p in list(pnet.parameters()) + list(qnet.parameters()):
        assert torch.isfinite(p).all()


def test_binding_refuses_cuts_that_do_not_ascend():
    """pendulum_rollout_fused takes the cut list lockstep_cuts produces:
    strictly ascending steps of the epoch.  Anything else is refused before
    the launch, so slot j of cut_final belongs to cuts[j] alone."""
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.ops.fused_mlp import _extract_layers

    ext = ops._load_extension()
    n, steps = 5, 6
    weights, biases, acts = _extract_layers(MLP(NETS["awkward"]).to(DEVICE))
    log_std = torch.zeros(1, device=DEVICE)

    def call(cuts):
        obs_full = torch.full((steps + 1, n, 3), -777.0, device=DEVICE)
        ext.pendulum_rollout_fused(
            list(weights), list(biases), acts, log_std, 11, 12, list(cuts), True,
            torch.full((1,), 1 << 40, dtype=torch.int64, device=DEVICE),
            torch.zeros(n, 2, dtype=torch.float64, device=DEVICE), obs_full,
            torch.zeros(steps, n, 1, device=DEVICE), torch.zeros(steps, n, device=DEVICE),
            torch.zeros(2, n, 3, device=DEVICE))
        torch.cuda.synchronize()
        return obs_full

    assert (call((1, 3)) != -777.0).all()
    for cuts in ((3, 1), (2, 2)):  # unsorted, repeated
        with pytest.raises(RuntimeError, match="ascending"):
            call(cuts)
    for cuts in ((6,), (-1,)):
        with pytest.raises(RuntimeError, match="out of range"):
            call(cuts)
