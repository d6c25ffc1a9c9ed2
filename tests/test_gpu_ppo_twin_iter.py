"""The twin PPO update (gpu-marked): policy iteration i and value
iteration i in one kernel pair (gaussian_ppo_value_twin_iter), and the
whole-epoch graph built from it.  Each net's arithmetic is that of its own
binding, so every comparison here is torch.equal — no tolerance.

Shapes are the smallest at which the kernels can go wrong: batch 33 (two
row blocks, ragged tail), 100 (4 blocks), 160 (5 blocks: odd count), 1000
(32 blocks); the bench pair [17,64,32,6] / [17,64,32,1] and an awkward pair
[5,24,3] / [5,16,8,1] whose depths differ and whose widths are no multiple
of 16 — halves that read each other's argument block cannot agree with
the separate bindings there.  All inputs come from a CPU generator."""
import pytest
import torch

pytestmark = pytest.mark.gpu

P_HP = (3e-4, 0.9, 0.999, 1e-8, 0.0)  # lr, beta1, beta2, eps, weight_decay
V_HP = (1e-3, 0.9, 0.999, 1e-8, 0.0)
NET_PAIRS = {
    "bench": ([17, 64, 32, 6], [17, 64, 32, 1]),
    "awkward": ([5, 24, 3], [5, 16, 8, 1]),
}
BATCHES = [33, 100, 160, 1000]
OPEN, SHUT = 1e9, -1e9  # thresholds no KL exceeds / every KL exceeds
# per iteration (step_delta 0, 1, 2): (first_iter, threshold)
GATE_CASES = {
    # iteration 0 never gates; the next two find the gate open and leave it so
    "first_iter": [(True, OPEN), (False, OPEN), (False, OPEN)],
    # iteration 1 enters with the gate open and closes it in that very call;
    # iteration 2 then finds it closed
    "closes_in_call": [(True, OPEN), (False, SHUT), (False, OPEN)],
    # gate closed before the first call: the policy half is frozen throughout
    "closed_on_entry": [(False, OPEN), (False, SHUT), (False, OPEN)],
}


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


def zeros_like_all(ts):
    return [torch.zeros_like(t) for t in ts]


class _Side:
    """One copy of both nets' parameters, Adam state and bookkeeping."""

    def __init__(self, ext, pdims, vdims, batch, gate_open):
        self.ext = ext
        d = pdims[-1]
        self.pw, self.pb, self.pacts = make_net(pdims, 41)
        self.vw, self.vb, self.vacts = make_net(vdims, 42)
        g = torch.Generator().manual_seed(43)
        self.obs = torch.randn(batch, pdims[0], generator=g).cuda()
        self.actions = torch.randn(batch, d, generator=g).cuda()
        self.adv = torch.randn(batch, generator=g).cuda()
        self.ret = torch.randn(batch, generator=g).cuda()
        self.log_std = (-0.5 * torch.ones(d)).cuda()
        mean = ext.mlp_forward(self.obs, list(self.pw), list(self.pb), self.pacts,
                               False)[0]
        # a stale old policy, so that ratios differ from 1 and the KL from 0
        self.old_logp = ext.gaussian_logp(mean + 0.05, self.actions, self.log_std)
        self.pm, self.pv = zeros_like_all(self.pw + self.pb), zeros_like_all(self.pw + self.pb)
        self.ls_m, self.ls_v = torch.zeros(d).cuda(), torch.zeros(d).cuda()
        self.vm, self.vv = zeros_like_all(self.vw + self.vb), zeros_like_all(self.vw + self.vb)
        self.pstep = torch.zeros((), device="cuda")
        self.vstep = torch.zeros((), device="cuda")
        self.gate = torch.full((1,), 1.0 if gate_open else 0.0, device="cuda")
        self.kl_final = torch.zeros(1, device="cuda")
        self.iters_done = torch.zeros(1, device="cuda")
        self.loss_out = torch.zeros(1, device="cuda")
        fb = int(ext.value_loss_partials_blocks(batch))
        self.partials = torch.zeros(3, fb, device="cuda")

    def policy_args(self, i, first_iter, thr):
        return (self.obs, list(self.pw), list(self.pb), self.pacts, self.actions,
                self.old_logp, self.adv, self.log_std, 0.2, self.pm, self.pv,
                self.ls_m, self.ls_v, self.pstep, *P_HP, float(i), self.gate,
                self.kl_final, self.iters_done, float(thr), self.loss_out,
                first_iter)

    def twin(self, i, first_iter, thr):
        self.ext.gaussian_ppo_value_twin_iter(
            *self.policy_args(i, first_iter, thr), self.obs, list(self.vw),
            list(self.vb), self.vacts, self.ret, self.partials[i], self.vm,
            self.vv, self.vstep, *V_HP, float(i))

    def separate(self, i, first_iter, thr):
        self.ext.gaussian_ppo_policy_iter(*self.policy_args(i, first_iter, thr))
        self.ext.value_mlp_backward(
            self.obs, list(self.vw), list(self.vb), [],
            torch.empty(0, device="cuda"), self.vacts, self.ret, 0,
            self.partials[i], self.vm, self.vv, self.vstep, *V_HP, float(i), True)

    def policy_state(self):
        return (self.pw + self.pb + [self.log_std] + self.pm + self.pv
                + [self.ls_m, self.ls_v, self.gate, self.kl_final,
                   self.iters_done, self.loss_out])

    def value_state(self):
        return self.vw + self.vb + self.vm + self.vv + [self.partials]


def assert_all_equal(got, want, what):
    for n, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: tensor {n} differs"


@pytest.mark.parametrize("case", list(GATE_CASES))
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("pair", list(NET_PAIRS))
def test_twin_iter_equals_separate_bindings(ext, pair, batch, case):
    pdims, vdims = NET_PAIRS[pair]
    gate_open = case != "closed_on_entry"
    a = _Side(ext, pdims, vdims, batch, gate_open)
    b = _Side(ext, pdims, vdims, batch, gate_open)
    policy0 = [t.clone() for t in a.policy_state()]
    value_prev = [t.clone() for t in a.value_state()]
    for i, (first_iter, thr) in enumerate(GATE_CASES[case]):
        a.twin(i, first_iter, thr)
        b.separate(i, first_iter, thr)
        torch.cuda.synchronize()
        assert_all_equal(a.policy_state(), b.policy_state(), f"policy, iteration {i}")
        assert_all_equal(a.value_state(), b.value_state(), f"value, iteration {i}")
        # the value half runs whatever the gate says
        assert not any(torch.equal(p, q) for p, q in
                       zip(a.vw + a.vb, value_prev[: len(a.vw + a.vb)]))
        value_prev = [t.clone() for t in a.value_state()]
        if case == "closed_on_entry":
            assert_all_equal(a.policy_state(), policy0, f"frozen policy, iteration {i}")
    if case == "first_iter":
        assert float(a.gate) == 1.0 and float(a.iters_done) == 2.0
    elif case == "closes_in_call":
        assert float(a.gate) == 0.0 and float(a.iters_done) == 1.0


# ---------------------------------------------------------------------------
# whole-epoch graph against the separate loops
# ---------------------------------------------------------------------------
def _make_ppo(num_p, num_v, max_kl):
    import torch.nn as nn

    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.algorithms import PPO
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import GaussianPolicy
    from rl_replicas_amd.samplers import VectorSampler
    from rl_replicas_amd.value_function import ValueFunction

    torch.manual_seed(5)
    pnet = MLP([17, 64, 32, 6]).to("cuda")
    log_std = nn.Parameter(-0.5 * torch.ones(6, device="cuda"))
    policy = GaussianPolicy(
        pnet, ops.make_adam(list(pnet.parameters()) + [log_std], lr=3e-4), log_std
    )
    vnet = MLP([17, 64, 32, 1]).to("cuda")
    vf = ValueFunction(vnet, ops.make_adam(vnet.parameters(), lr=1e-3))
    venv = envs.VectorEnv("HalfCheetah-v4", num_envs=10)
    return PPO(policy, vf, venv, VectorSampler(venv, seed=0),
               max_kl_divergence=max_kl, num_policy_gradients=num_p,
               num_value_gradients=num_v)


def _optimizer_state(opt):
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state[p]
            out += [st["step"], st["exp_avg"], st["exp_avg_sq"]]
    return out


def _run_two_epochs(num_p, num_v, max_kl):
    """Fresh model, two epochs of the update as OnPolicyAlgorithm.train
    issues it; returns (state tensors, metrics per epoch, iters_done per
    epoch, whether the twin graph ran)."""
    g = torch.Generator().manual_seed(55)
    batch = 160
    obs = torch.randn(batch, 17, generator=g).cuda()
    actions = torch.randn(batch, 6, generator=g).cuda()
    adv = torch.randn(batch, generator=g).cuda()
    returns = torch.randn(batch, generator=g).cuda()
    m = _make_ppo(num_p, num_v, max_kl)
    metrics, iters = [], []
    for _ in range(2):
        joint = m._update_policy_and_value(obs, actions, adv, returns)
        if joint is None:
            joint = (m._update_policy(obs, actions, adv),
                     m._update_value_function(obs, returns))
        metrics.append(joint)
        twin = getattr(m, "_ppo_twin_graph", None)
        graph = twin if twin is not None else m._ppo_policy_graph
        iters.append(int(graph[1].iters_done))
    state = [p.data.clone() for p in m.policy.parameters()]
    state += [p.data.clone() for p in m.value_function.parameters()]
    state += [t.clone() for t in _optimizer_state(m.policy.optimizer)]
    state += [t.clone() for t in _optimizer_state(m.value_function.optimizer)]
    return state, metrics, iters, twin is not None


# max_kl_divergence of the early-stop case: the stop fires when the KL
# exceeds 1.5x this.  See the note in test_epoch_graph_equals_separate_loops.
EARLY_STOP_MAX_KL = 1.5e-3
LOOP_CASES = {
    "no_stop": (7, 7, 1e9),
    "early_stop": (7, 7, EARLY_STOP_MAX_KL),
    "value_tail": (3, 7, 1e9),
    "fallback_p_gt_v": (7, 3, 1e9),
}


@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_epoch_graph_equals_separate_loops(ext, monkeypatch, case):
    """Two epochs with RL_REPLICAS_AMD_PPO_TWIN=1 and =0 from identical
    fresh models: parameters, Adam state and metrics are equal.

    Early stop: in a float32 CPU rehearsal of this case (same seeds,
    torch autograd, Adam lr 3e-4) the approximate KL after updates 1..4 of
    epoch 1 is 6.3e-4, 1.2e-3, 1.8e-3, 2.9e-3 and after updates 1..2 of
    epoch 2 it is 1.6e-3, 3.4e-3.  The stop threshold 1.5 * 1.5e-3 =
    2.25e-3 lies at least 20 % away from each of them, so the stop fires
    after 4 updates, then after 2: inside 1 <= iters_done < 7."""
    num_p, num_v, max_kl = LOOP_CASES[case]
    monkeypatch.setenv("RL_REPLICAS_AMD_PPO_TWIN", "1")
    s1, m1, it1, twin1 = _run_two_epochs(num_p, num_v, max_kl)
    monkeypatch.setenv("RL_REPLICAS_AMD_PPO_TWIN", "0")
    s0, m0, it0, twin0 = _run_two_epochs(num_p, num_v, max_kl)
    print(f"{case}: iters_done twin {it1} separate {it0}; metrics {m1}")
    assert not twin0
    assert twin1 == (num_p <= num_v)
    if case == "early_stop":
        assert all(1 <= n < num_p for n in it1 + it0)
    else:
        assert all(n == num_p for n in it1 + it0)
    assert it1 == it0
    assert m1 == m0
    assert_all_equal(s1, s0, case)
