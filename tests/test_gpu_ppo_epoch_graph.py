"""The fused PPO epoch (gpu-marked): ppo_ingest_rows, the GAE / normalize
out-variants, ppo_epoch_epilogue, and the whole train side of an epoch as one
eager launch + one graph replay (_GraphedPPOEpoch) against the path it
replaces.  Every kernel runs the arithmetic of the launch it stands in for on
the same values, so every comparison here is torch.equal or == — no tolerance.

Shapes are the smallest at which the kernels can go wrong.  Episode lengths
[5, 16, 1, 15] (T = 37, E = 4: the third 16-row tile holds step rows, all four
bootstrap rows and padding), [16] (the bootstrap row opens a tile) and [3];
the bench pair [17,64,32,6] / [17,64,32,1] and an awkward pair [5,8,3] /
[5,16,8,1] whose input width is no multiple of 4, whose head is narrower than
a tile and whose depths differ.  All inputs come from a CPU generator."""
import copy
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NET_PAIRS = {
    "bench": ([17, 64, 32, 6], [17, 64, 32, 1]),
    "awkward": ([5, 8, 3], [5, 16, 8, 1]),
}
EPISODES = {"mixed_tile": [5, 16, 1, 15], "boot_opens_tile": [16], "short": [3]}
GAMMA, LAM = 0.99, 0.97


@pytest.fixture(scope="module")
def ext():
    from rl_replicas_amd import ops

    assert ops.hip_available()
    return ops._load_extension()


def make_net(dims, seed):
    """tanh hidden layers, identity head; weights from a CPU generator."""
    g = torch.Generator().manual_seed(seed)
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        ws.append((torch.randn(o, i, generator=g) / float(i) ** 0.5).cuda())
        bs.append((0.1 * torch.randn(o, generator=g)).cuda())
    acts = [1] * (len(dims) - 2) + [0]
    return ws, bs, acts


def episode_index(lengths):
    """int32 offsets [E + 1] and mixed done flags [E]."""
    offsets = torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0).to(torch.int32)
    dones = torch.tensor([(e + 1) % 2 for e in range(len(lengths))], dtype=torch.int32)
    return offsets.cuda(), dones.cuda()


def bits(t):
    """Bit pattern of an fp32 tensor: tells -0.0 from 0.0, which == does not."""
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------
# 1. the ingest kernel against mlp_forward on the cat + gaussian_logp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("episodes", list(EPISODES))
@pytest.mark.parametrize("pair", list(NET_PAIRS))
def test_ingest_equals_present_bindings(ext, pair, episodes):
    pdims, vdims = NET_PAIRS[pair]
    lengths = EPISODES[episodes]
    T, E, O, A = sum(lengths), len(lengths), pdims[0], pdims[-1]
    g = torch.Generator().manual_seed(44)
    obs = torch.randn(T, O, generator=g).cuda()
    last_obs = torch.randn(E, O, generator=g).cuda()
    actions = torch.randn(T, A, generator=g).cuda()
    rewards = torch.randn(T, generator=g).cuda()
    offsets, dones = episode_index(lengths)
    pw, pb, pacts = make_net(pdims, 41)
    vw, vb, vacts = make_net(vdims, 42)
    # an old policy that is NOT the policy: a kernel reading the wrong net or
    # the wrong log_std cannot pass
    ow = [w + 0.03 * torch.randn(w.shape, generator=g).cuda() for w in pw]
    ob = [b + 0.03 * torch.randn(b.shape, generator=g).cuda() for b in pb]
    log_std = (-0.5 + 0.1 * torch.randn(A, generator=g)).cuda()
    old_log_std = (log_std + 0.07).contiguous()

    nan = float("nan")  # an element the kernel leaves out cannot compare equal
    obs_out = torch.full((T, O), nan, device="cuda")
    act_out = torch.full((T, A), nan, device="cuda")
    rew_out = torch.full((T,), nan, device="cuda")
    off_out = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    dones_out = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    values_all = torch.full((T + E,), nan, device="cuda")
    old_logp = torch.full((T,), nan, device="cuda")
    logp_now = torch.full((T,), nan, device="cuda")
    ext.ppo_ingest_rows(obs, last_obs, actions, rewards, offsets, dones,
                        vw, vb, vacts, pw, pb, pacts, log_std, ow, ob, old_log_std,
                        obs_out, act_out, rew_out, off_out, dones_out, values_all,
                        old_logp, logp_now)

    rows = torch.cat([obs, last_obs], dim=0)
    want_values = ext.mlp_forward(rows, vw, vb, vacts, False, 0)[0].flatten()
    want_now = ext.gaussian_logp(ext.mlp_forward(obs, pw, pb, pacts, False, 0)[0],
                                 actions, log_std)
    want_old = ext.gaussian_logp(ext.mlp_forward(obs, ow, ob, pacts, False, 0)[0],
                                 actions, old_log_std)
    torch.cuda.synchronize()
    assert not torch.equal(want_now, want_old)
    assert torch.equal(values_all, want_values)
    assert torch.equal(logp_now, want_now)
    assert torch.equal(old_logp, want_old)
    assert torch.equal(obs_out, obs)
    assert torch.equal(act_out, actions)
    assert torch.equal(rew_out, rewards)
    assert torch.equal(off_out, offsets)
    assert torch.equal(dones_out, dones)


# ---------------------------------------------------------------------------
# 2. GAE and normalize into the caller's buffers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("episodes", list(EPISODES))
def test_gae_and_normalize_out_equal_present_bindings(ext, episodes):
    lengths = EPISODES[episodes]
    T, E = sum(lengths), len(lengths)
    g = torch.Generator().manual_seed(46)
    rewards = torch.randn(T, generator=g).cuda()
    values_all = torch.randn(T + E, generator=g).cuda()
    offsets, dones = episode_index(lengths)
    adv_raw = torch.full((T,), float("nan"), device="cuda")
    ret = torch.full((T,), float("nan"), device="cuda")
    adv = torch.full((T,), float("nan"), device="cuda")
    ext.segmented_gae_out(rewards, values_all, offsets, dones, GAMMA, LAM, adv_raw, ret)
    ext.normalize_out(adv_raw, adv)

    want_adv, want_ret = ext.segmented_gae(
        rewards, values_all[:T].contiguous(), values_all[T:].contiguous(), offsets,
        dones, GAMMA, LAM)
    want_norm = ext.normalize(want_adv)
    torch.cuda.synchronize()
    assert torch.equal(adv_raw, want_adv)
    assert torch.equal(ret, want_ret)
    assert torch.equal(bits(adv), bits(want_norm))  # NaN-safe (T = 1 never occurs)


# ---------------------------------------------------------------------------
# 3. the epilogue kernel against the five operations it replaces
# ---------------------------------------------------------------------------
# (gate on entry, flushed KL, threshold)
EPILOGUE_CASES = {
    "gate_open": (1.0, 0.01, 1.0),
    "gate_closes_on_flushed_kl": (1.0, 0.5, 0.1),
    "gate_already_closed": (0.0, 0.5, 0.1),
}


@pytest.mark.parametrize("case", list(EPILOGUE_CASES))
def test_epilogue_equals_the_five_operations(ext, case):
    gate0, kl0, thr = EPILOGUE_CASES[case]
    rows, stride, fb, num_v = 5, 70, 67, 6.0  # 2 row blocks; fb spans 2 chunks
    g = torch.Generator().manual_seed(47)
    partials = torch.randn(rows, stride, generator=g).cuda()
    src = [torch.randn(n, generator=g).cuda() for n in (17 * 64, 64, 300, 1, 6)]
    src[2][5] = -0.0
    src[3][0] = -0.0

    def side():
        return dict(
            gate=torch.full((1,), gate0, device="cuda"),
            kl=torch.full((1,), kl0, device="cuda"),
            kl_final=torch.full((1,), 0.125, device="cuda"),
            iters_done=torch.full((1,), 4.0, device="cuda"),
            pol_steps=[torch.full((), 3.0, device="cuda") for _ in range(7)],
            val_steps=[torch.full((), 11.0, device="cuda") for _ in range(6)],
            dst=[torch.full_like(s, 9.0) for s in src],
        )

    a, b = side(), side()
    iters_out = torch.full((1,), float("nan"), device="cuda")
    losses = torch.full((rows,), float("nan"), device="cuda")
    ext.ppo_epoch_epilogue_(a["gate"], a["kl"], a["kl_final"], a["iters_done"],
                            iters_out, thr, a["pol_steps"], a["val_steps"], num_v,
                            partials, fb, losses, src, a["dst"])

    ext.ppo_gate_update_(b["gate"], b["kl"], b["kl_final"], b["iters_done"], thr)
    ext.adam_bump_dev_(b["pol_steps"], b["iters_done"])
    ext.adam_bump_(b["val_steps"], num_v)
    want_losses = ext.value_loss_finalize(partials, fb)
    for d, s in zip(b["dst"], src):
        d.copy_(s)
    torch.cuda.synchronize()

    assert float(b["gate"]) == (0.0 if case != "gate_open" else 1.0)
    assert float(b["iters_done"]) == (4.0 if case == "gate_already_closed" else 5.0)
    assert torch.equal(iters_out, b["iters_done"])
    assert torch.equal(a["kl_final"], b["kl_final"])
    for x, y in zip(a["pol_steps"] + a["val_steps"], b["pol_steps"] + b["val_steps"]):
        assert torch.equal(x, y)
    assert torch.equal(losses, want_losses)
    for x, y, s in zip(a["dst"], b["dst"], src):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(s))
    assert math.copysign(1.0, float(a["dst"][3][0])) == -1.0
    # what the next replay finds
    assert float(a["gate"]) == 1.0 and float(a["iters_done"]) == 0.0


# ---------------------------------------------------------------------------
# 4. PPO.train: the fused epoch against RL_REPLICAS_AMD_PPO_EPOCH_GRAPH=0
# ---------------------------------------------------------------------------
N_ENVS, STEPS, HORIZON = 8, 20, 30


def _make_ppo(num_p, num_v, max_kl, policy_kind="gaussian"):
    import tempfile

    import torch.nn as nn

    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.algorithms import PPO
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import CategoricalPolicy, GaussianPolicy
    from rl_replicas_amd.samplers import DeviceSampler
    from rl_replicas_amd.value_function import ValueFunction

    torch.manual_seed(5)
    pnet = MLP([17, 64, 32, 6]).to("cuda")
    if policy_kind == "gaussian":
        log_std = nn.Parameter(-0.5 * torch.ones(6, device="cuda"))
        policy = GaussianPolicy(
            pnet, ops.make_adam(list(pnet.parameters()) + [log_std], lr=3e-4), log_std
        )
    else:
        policy = CategoricalPolicy(pnet, ops.make_adam(pnet.parameters(), lr=3e-4))
    vnet = MLP([17, 64, 32, 1]).to("cuda")
    vf = ValueFunction(vnet, ops.make_adam(vnet.parameters(), lr=1e-3))
    denv = envs.DeviceVectorEnv("HalfCheetah-v4", num_envs=N_ENVS, device="cuda")
    denv.spec = copy.copy(denv.spec)
    denv.spec.max_episode_steps = HORIZON
    model = PPO(policy, vf, denv, DeviceSampler(denv, seed=3, is_continuous=True),
                max_kl_divergence=max_kl, num_policy_gradients=num_p,
                num_value_gradients=num_v)
    model._begin_learn(tempfile.mkdtemp())
    model.metrics_manager.stdout = False
    recorded = []
    model.metrics_manager.record_scalar = (
        lambda tag, value, *a, **k: recorded.append((tag, value)))
    return model, recorded


def _optimizer_state(opt):
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state[p]
            out += [st["step"], st["exp_avg"], st["exp_avg_sq"]]
    return out


def _model_state(m):
    state = [p.data for p in m.policy.parameters()]
    state += [p.data for p in m.value_function.parameters()]
    state += [p.data for p in m.old_policy.parameters()]
    state += _optimizer_state(m.policy.optimizer)
    state += _optimizer_state(m.value_function.optimizer)
    return state


# (P, V, max_kl_divergence).  The stop fires when the approximate KL exceeds
# 1.5 * max_kl.  The estimate mean(old_logp - logp) may come out negative, but
# after Adam steps of lr 3e-4 its size is 1e-4 to 1e-2 (the rehearsal in
# test_gpu_ppo_twin_iter.py), so -1.0 lies below it and the stop fires after
# update 1 of every epoch; 1e9 lies above every KL, so all P updates run.
EPOCH_CASES = {
    "stop_before_p": (4, 6, -1.0),
    "never_stops_p_lt_v": (4, 6, 1e9),
    "never_stops_p_eq_v": (3, 3, 1e9),
}


@pytest.mark.parametrize("case", list(EPOCH_CASES))
def test_fused_epoch_equals_present_path(ext, monkeypatch, case):
    """Three consecutive experiences of 8 envs x 20 steps through PPO.train
    on two identical models, one per path.  The horizon of 30 puts a
    truncation cut into the second experience (E = 16 instead of 8: the graph
    is re-keyed) and closes the third one's episodes with done = 1."""
    num_p, num_v, max_kl = EPOCH_CASES[case]
    fused, rec_f = _make_ppo(num_p, num_v, max_kl)
    present, rec_p = _make_ppo(num_p, num_v, max_kl)
    n_eps = []
    for epoch in range(3):
        experience = fused.sampler.sample(N_ENVS * STEPS, fused.policy)
        flat = experience.to_flat_batch()
        n_eps.append(int(flat["last_observations"].shape[0]))
        monkeypatch.setenv("RL_REPLICAS_AMD_PPO_EPOCH_GRAPH", "1")
        fused.train(experience)
        monkeypatch.setenv("RL_REPLICAS_AMD_PPO_EPOCH_GRAPH", "0")
        present.train(experience)
        torch.cuda.synchronize()
        for n, (x, y) in enumerate(zip(_model_state(fused), _model_state(present))):
            assert torch.equal(x, y), f"{case}, epoch {epoch}: state tensor {n} differs"
    print(f"{case}: episodes per epoch {n_eps}; metrics {rec_f}")
    assert n_eps == [8, 16, 8]
    assert fused.epoch_graph_replays == 3 and len(fused._ppo_epoch_graphs) == 2
    assert getattr(present, "epoch_graph_replays", 0) == 0
    assert getattr(present, "_ppo_twin_graph", None) is not None
    assert len(rec_f) == 15 and rec_f == rec_p
    kls = [v for tag, v in rec_f if tag == "policy/kl_divergence"]
    steps = float(fused.policy.optimizer.state[fused.policy.log_std]["step"])
    assert steps == (3.0 if case == "stop_before_p" else 3.0 * num_p), (steps, kls)
    # the old policy follows the policy (a plain copy, bit for bit)
    for p, o in zip(fused.policy.parameters(), fused.old_policy.parameters()):
        assert torch.equal(bits(p.data), bits(o.data))


# ---------------------------------------------------------------------------
# 5. eligibility: who takes the fused epoch
# ---------------------------------------------------------------------------
def _install_dp_hooks(model, mode):
    """What enable_data_parallel installs on a rank (parallel/ddp.py), with
    the collectives of a world of one."""
    from rl_replicas_amd import ops

    if mode == "replicate":
        model._gather_global_batch = types.MethodType(
            lambda self, obs, actions, adv, ret: (obs, actions, adv, ret), model)
        model._dp_replicate = True
    model._normalize_advantages = types.MethodType(
        lambda self, adv: ops.normalize(adv), model)
    model._reduce_scalar_mean = types.MethodType(lambda self, x: x, model)
    model._dp_enabled = True


ELIGIBILITY_CASES = ["single_process", "dp_replicate", "dp_allreduce", "categorical",
                     "bf16", "env_off"]


@pytest.mark.parametrize("case", ELIGIBILITY_CASES)
def test_who_takes_the_fused_epoch(ext, monkeypatch, case):
    from rl_replicas_amd.ops import fused_onpolicy as fop

    monkeypatch.setenv("RL_REPLICAS_AMD_PPO_EPOCH_GRAPH", "1")
    kind = "categorical" if case == "categorical" else "gaussian"
    model, _ = _make_ppo(2, 2, 1e9, policy_kind=kind)
    g = torch.Generator().manual_seed(48)
    if case.startswith("dp_"):
        _install_dp_hooks(model, case[3:])
    if case == "bf16":
        monkeypatch.setenv("RL_REPLICAS_AMD_COMPUTE_DTYPE", "bf16")
    if case == "env_off":
        monkeypatch.setenv("RL_REPLICAS_AMD_PPO_EPOCH_GRAPH", "0")

    if kind == "gaussian":
        experience = model.sampler.sample(N_ENVS * STEPS, model.policy)
    else:
        # the lockstep sampler draws Gaussian actions only: a hand-made flat
        # batch of class indices, shaped like its own
        from rl_replicas_amd.experience import Experience

        T = N_ENVS * STEPS
        experience = Experience()
        experience.set_flat_cache({
            "observations": torch.randn(T, 17, generator=g).cuda(),
            "actions": torch.randint(0, 6, (T,), generator=g).cuda(),
            "rewards": torch.randn(T, generator=g).cuda(),
            "episode_offsets": torch.arange(0, T + 1, STEPS, dtype=torch.int32).cuda(),
            "episode_dones": torch.zeros(N_ENVS, dtype=torch.int32).cuda(),
            "last_observations": torch.randn(N_ENVS, 17, generator=g).cuda(),
        })
    obs = experience.to_flat_batch()["observations"]
    want = case == "single_process"
    assert fop.ppo_epoch_eligible(model, obs) == want
    model.train(experience)
    torch.cuda.synchronize()
    assert getattr(model, "epoch_graph_replays", 0) == (1 if want else 0)
    assert (len(getattr(model, "_ppo_epoch_graphs", {})) == 1) == want
    # which path ran instead: the twin graph wherever it is eligible
    # (replicate-mode DP captures whole; all-reduce DP splits the loops, bf16
    # has no fused iteration)
    twin = getattr(model, "_ppo_twin_graph", None) is not None
    assert twin == (case in ("dp_replicate", "categorical", "env_off"))
    if case in ("dp_allreduce", "bf16"):
        assert getattr(model, "_ppo_policy_graph", None) is not None
    for p in model.policy.parameters():
        assert torch.isfinite(p).all()
