"""The trimmed PPO update iteration (gpu-marked): fused-Adam value step
without an input gradient, the two-kernel Gaussian-PPO policy iteration
(gate bookkeeping inside the reduce+Adam kernel, gate-frozen iterations
skipped) and the rebalanced wgrad loop.

Shapes are the smallest at which these kernels can go wrong: batch 33
(2 row blocks, ragged tail, two empty reduce quarters), 100 (4 blocks),
160 (5 blocks: odd count, uneven quarters), 1000 (32 blocks); networks
[17,64,32,1] / [17,64,32,6] (the bench nets) and [5,24,1] (widths no
multiple of 16, element count no multiple of 64 or 16).  Batch 24608
(769 blocks) is the first size past the LDS-staged reduce's
partial-count limit of 768, where the direct-read reduce takes over.
All inputs come from a CPU generator and are copied to the device."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "update_iter_trim_value3_b160.npy")
ADAM_HP = (1e-3, 0.9, 0.999, 1e-8, 0.0)  # lr, beta1, beta2, eps, weight_decay
VALUE_NETS = [[17, 64, 32, 1], [5, 24, 1]]
BATCHES = [33, 100, 160, 1000]


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


def make_value_batch(dims, batch, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(batch, dims[0], generator=g).cuda()
    ret = torch.randn(batch, generator=g).cuda()
    return obs, ret


def zeros_like_all(ts):
    return [torch.zeros_like(t) for t in ts]


def clone_all(ts):
    return [t.clone() for t in ts]


def fused_value_step(ext, obs, ret, ws, bs, acts, m, v, step0, delta,
                     fwd_in_kernel=True):
    """One fused-Adam value step; returns the binding's output list."""
    if fwd_in_kernel:
        hidden, final = [], torch.empty(0, device="cuda")
    else:
        outs = ext.mlp_forward(obs, list(ws), list(bs), acts, True)
        hidden, final = list(outs[1:]), outs[0]
    return ext.value_mlp_backward(obs, list(ws), list(bs), hidden, final, acts,
                                  ret, 0, None, m, v, step0, *ADAM_HP,
                                  float(delta), fwd_in_kernel)


def autograd_reference(ws, bs, obs, seed_fn):
    """float64 CPU autograd through the same tanh MLP; seed_fn maps the
    net output to a scalar loss.  Returns (loss, dx, dws, dbs)."""
    x = obs.double().cpu().requires_grad_(True)
    pw = [w.double().cpu().requires_grad_(True) for w in ws]
    pb = [b.double().cpu().requires_grad_(True) for b in bs]
    h = x
    for l, (w, b) in enumerate(zip(pw, pb)):
        h = h @ w.t() + b
        if l < len(pw) - 1:
            h = torch.tanh(h)
    loss = seed_fn(h)
    loss.backward()
    f32 = lambda t: t.float().cuda()  # noqa: E731
    return (f32(loss.detach()), f32(x.grad), [f32(w.grad) for w in pw],
            [f32(b.grad) for b in pb])


class TestFusedAdamValueStepNoDx:
    @pytest.mark.parametrize("fwd_in_kernel", [True, False])
    @pytest.mark.parametrize("batch", BATCHES + [24608])
    @pytest.mark.parametrize("dims", VALUE_NETS, ids=["bench", "awkward"])
    def test_matches_separate_chain(self, ext, dims, batch, fwd_in_kernel):
        """Fused value step (no dx) == forward -> value_mlp_backward
        without Adam -> FusedAdam.step, at the tolerances of
        test_fwd_in_kernel_adam_step_matches_separate."""
        from rl_replicas_amd.ops.fused_adam import FusedAdam

        ws, bs, acts = make_net(dims, 7)
        obs, ret = make_value_batch(dims, batch, 8)

        # separate chain on its own copy of the parameters
        ps = [torch.nn.Parameter(t.clone()) for t in ws + bs]
        n = len(ws)
        w_s, b_s = [p.data for p in ps[:n]], [p.data for p in ps[n:]]
        outs = ext.mlp_forward(obs, list(w_s), list(b_s), acts, True)
        grads = ext.value_mlp_backward(obs, list(w_s), list(b_s), list(outs[1:]),
                                       outs[0], acts, ret)
        assert grads[0].shape == obs.shape  # the non-Adam mode still returns dx
        for p, g in zip(ps, list(grads[1 : 1 + 2 * n])):
            p.grad = g
        FusedAdam(ps, lr=ADAM_HP[0]).step()

        m, v = zeros_like_all(ws + bs), zeros_like_all(ws + bs)
        step0 = torch.zeros((), device="cuda")
        out = fused_value_step(ext, obs, ret, ws, bs, acts, m, v, step0, 0,
                               fwd_in_kernel)
        assert out[0].numel() == 0  # dx slot is empty
        torch.testing.assert_close(out[-1][0], grads[-1][0], rtol=1e-5, atol=1e-7)
        for p_f, p_s in zip(ws + bs, ps):
            torch.testing.assert_close(p_f, p_s.data, rtol=1e-5, atol=1e-7)

    def test_golden_from_parent_commit(self, ext):
        """Parameters after three fused-Adam value steps at batch 160,
        [17,64,32,1], recorded on MI355X with the commit before the
        update iteration was trimmed: bitwise equal."""
        dims = [17, 64, 32, 1]
        ws, bs, acts = make_net(dims, 1234)
        obs, ret = make_value_batch(dims, 160, 4321)
        m, v = zeros_like_all(ws + bs), zeros_like_all(ws + bs)
        step0 = torch.zeros((), device="cuda")
        for i in range(3):
            fused_value_step(ext, obs, ret, ws, bs, acts, m, v, step0, i)
        got = torch.cat([t.reshape(-1) for t in ws + bs]).cpu().numpy()
        want = np.load(GOLDEN)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


class TestNonAdamGradients:
    """The paths that still return dx and dW/db, against autograd at the
    existing tolerances (rtol 5e-4, atol 5e-5)."""

    @pytest.mark.parametrize("batch", BATCHES)
    @pytest.mark.parametrize("dims", VALUE_NETS, ids=["bench", "awkward"])
    def test_value_mlp_backward(self, ext, dims, batch):
        ws, bs, acts = make_net(dims, 11)
        obs, ret = make_value_batch(dims, batch, 12)
        outs = ext.mlp_forward(obs, list(ws), list(bs), acts, True)
        grads = ext.value_mlp_backward(obs, list(ws), list(bs), list(outs[1:]),
                                       outs[0], acts, ret)
        ret64 = ret.double().cpu()
        loss, dx, dws, dbs = autograd_reference(
            ws, bs, obs, lambda h: torch.mean((h.squeeze(-1) - ret64) ** 2))
        n = len(ws)
        torch.testing.assert_close(grads[-1][0], loss, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(grads[0], dx, rtol=5e-4, atol=5e-5)
        for got, want in zip(grads[1 : 1 + 2 * n], dws + dbs):
            torch.testing.assert_close(got, want, rtol=5e-4, atol=5e-5)

    @pytest.mark.parametrize("batch", BATCHES)
    def test_mlp_backward_policy_net(self, ext, batch):
        dims = [17, 64, 32, 6]
        ws, bs, acts = make_net(dims, 13)
        g = torch.Generator().manual_seed(14)
        obs = torch.randn(batch, dims[0], generator=g).cuda()
        dy = (torch.randn(batch, dims[-1], generator=g) / batch).cuda()
        outs = ext.mlp_forward(obs, list(ws), list(bs), acts, True)
        grads = ext.mlp_backward(dy, obs, list(ws), list(bs), list(outs[1:]),
                                 outs[0], acts)
        dy64 = dy.double().cpu()
        _, dx, dws, dbs = autograd_reference(
            ws, bs, obs, lambda h: torch.sum(h * dy64))
        torch.testing.assert_close(grads[0], dx, rtol=5e-4, atol=5e-5)
        for got, want in zip(grads[1:], dws + dbs):
            torch.testing.assert_close(got, want, rtol=5e-4, atol=5e-5)
        only_dx = ext.mlp_backward(dy, obs, list(ws), list(bs), list(outs[1:]),
                                   outs[0], acts, input_grad_only=True)
        assert torch.equal(only_dx[0], grads[0])


class _PolicyIter:
    """State for direct gaussian_ppo_policy_iter calls on [17,64,32,6]."""

    def __init__(self, ext, batch):
        self.ext = ext
        dims = [17, 64, 32, 6]
        self.ws, self.bs, self.acts = make_net(dims, 21)
        g = torch.Generator().manual_seed(22)
        self.obs = torch.randn(batch, 17, generator=g).cuda()
        self.actions = torch.randn(batch, 6, generator=g).cuda()
        self.adv = torch.randn(batch, generator=g).cuda()
        self.log_std = (-0.5 * torch.ones(6)).cuda()
        self.old_logp = ext.gaussian_logp(self.mean(), self.actions, self.log_std)
        self.m, self.v = zeros_like_all(self.ws + self.bs), zeros_like_all(self.ws + self.bs)
        self.ls_m, self.ls_v = torch.zeros(6).cuda(), torch.zeros(6).cuda()
        self.step0 = torch.zeros((), device="cuda")
        self.gate = torch.ones(1, device="cuda")
        self.kl_final = torch.zeros(1, device="cuda")
        self.iters_done = torch.zeros(1, device="cuda")
        self.loss_out = torch.zeros(1, device="cuda")

    def mean(self):
        return self.ext.mlp_forward(self.obs, list(self.ws), list(self.bs),
                                    self.acts, False)[0]

    def kl_now(self):
        return self.ext.gaussian_kl(self.mean(), self.actions, self.log_std,
                                    self.old_logp)

    def call(self, i, thr, first_iter):
        out = self.ext.gaussian_ppo_policy_iter(
            self.obs, list(self.ws), list(self.bs), self.acts, self.actions,
            self.old_logp, self.adv, self.log_std, 0.2, self.m, self.v,
            self.ls_m, self.ls_v, self.step0, 3e-4, 0.9, 0.999, 1e-8, 0.0,
            float(i), self.gate, self.kl_final, self.iters_done, float(thr),
            self.loss_out, first_iter)
        torch.cuda.synchronize()
        assert out.numel() == 0  # dx slot is empty
        return out

    def updated(self):
        """Everything the Adam update touches."""
        return (self.ws + self.bs + [self.log_std] + self.m + self.v
                + [self.ls_m, self.ls_v])

    def scalars(self):
        return [self.gate, self.kl_final, self.iters_done, self.loss_out]


def all_equal(before, after):
    return all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("batch", [100, 160])
class TestPolicyIterDirect:
    def test_first_iteration(self, ext, batch):
        s = _PolicyIter(ext, batch)
        params0 = clone_all(s.ws + s.bs + [s.log_std])
        # old == current policy: ratio 1, loss = -mean(adv).  |logp| is
        # ~10-20 here, so two fp32 evaluations of it differ by a few ulp
        # (~1e-6 each) and the ratio by as much: the loss is off by at
        # most a few 1e-6 * mean|adv| -> atol 1e-5
        want_loss = -s.adv.double().mean().float()
        s.call(0, -1e9, True)  # a threshold that would gate any later call
        torch.testing.assert_close(s.loss_out[0], want_loss, rtol=1e-4, atol=1e-5)
        assert float(s.gate) == 1.0 and float(s.iters_done) == 0.0
        assert float(s.kl_final) == 0.0
        for p0, p in zip(params0, s.ws + s.bs + [s.log_std]):
            assert not torch.equal(p0, p)

    def test_open_gate_applies_update(self, ext, batch):
        s = _PolicyIter(ext, batch)
        s.call(0, 1e9, True)
        kl = float(s.kl_now())
        before = clone_all(s.updated())
        loss0 = s.loss_out.clone()
        s.call(1, 1e9, False)
        assert float(s.gate) == 1.0 and float(s.iters_done) == 1.0
        assert abs(float(s.kl_final) - kl) <= 1e-6
        assert torch.equal(s.loss_out, loss0)  # only iteration 0 writes it
        assert not any(torch.equal(a, b) for a, b in zip(before, s.updated()))

    def test_threshold_crossed_closes_gate(self, ext, batch):
        s = _PolicyIter(ext, batch)
        s.call(0, 1e9, True)
        kl = float(s.kl_now())
        before = clone_all(s.updated())
        s.call(1, -1e9, False)
        assert float(s.gate) == 0.0 and float(s.iters_done) == 1.0
        assert abs(float(s.kl_final) - kl) <= 1e-6
        assert all_equal(before, s.updated())  # bitwise: nothing was applied

    def test_gate_closed_on_entry_is_a_noop(self, ext, batch):
        s = _PolicyIter(ext, batch)
        s.call(0, 1e9, True)
        s.gate.zero_()
        s.kl_final.fill_(123.0)
        s.iters_done.fill_(7.0)
        s.loss_out.fill_(-5.0)
        before = clone_all(s.updated() + s.scalars())
        for thr in (1e9, -1e9):
            s.call(2, thr, False)  # still returns
            assert all_equal(before, s.updated() + s.scalars())


def _make_ppo(seed, dims_v=(17, 64, 32, 1)):
    import torch.nn as nn

    from rl_replicas_amd import envs, ops
    from rl_replicas_amd.algorithms import PPO
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import GaussianPolicy
    from rl_replicas_amd.samplers import VectorSampler
    from rl_replicas_amd.value_function import ValueFunction

    torch.manual_seed(seed)
    pnet = MLP([17, 64, 32, 6]).to("cuda")
    log_std = nn.Parameter(-0.5 * torch.ones(6, device="cuda"))
    policy = GaussianPolicy(
        pnet, ops.make_adam(list(pnet.parameters()) + [log_std], lr=3e-4), log_std
    )
    vnet = MLP(list(dims_v)).to("cuda")
    vf = ValueFunction(vnet, ops.make_adam(vnet.parameters(), lr=1e-3))
    venv = envs.VectorEnv("HalfCheetah-v4", num_envs=10)
    return PPO(policy, vf, venv, VectorSampler(venv, seed=0),
               num_policy_gradients=5, num_value_gradients=5)


class TestCapturedLoops:
    @pytest.mark.parametrize("batch", [160, 1000])
    def test_two_fresh_runs_are_bitwise_equal(self, ext, batch):
        """Five captured value iterations and five captured policy
        iterations, twice from scratch: torch.equal parameters."""
        from rl_replicas_amd.ops import fused_onpolicy as fop

        g = torch.Generator().manual_seed(31)
        obs = torch.randn(batch, 17, generator=g).cuda()
        actions = torch.randn(batch, 6, generator=g).cuda()
        adv = torch.randn(batch, generator=g).cuda()
        returns = torch.randn(batch, generator=g).cuda()
        runs = []
        for _ in range(2):
            m = _make_ppo(3)
            m.max_kl_divergence = 1e9  # all five policy iterations execute
            fop.ppo_update(m, obs, actions, adv)
            fop.value_update(m, obs, returns, 5)
            assert getattr(m, "_ppo_policy_graph", None) is not None
            assert int(m._ppo_policy_graph[1].iters_done) == 5
            runs.append(clone_all(list(m.policy.parameters())
                                  + list(m.value_function.parameters())))
        assert all_equal(runs[0], runs[1])

    def test_deep_narrow_value_net_falls_back(self, ext):
        """[64,64,64,64,1] passes the narrow-net gate but its in-kernel
        forward does not fit the LDS budget at 32-row tiles: value_update
        must complete through the separate-forward form, not raise."""
        from rl_replicas_amd.ops import fused_onpolicy as fop

        m = _make_ppo(4, dims_v=(64, 64, 64, 64, 1))
        g = torch.Generator().manual_seed(32)
        obs = torch.randn(100, 64, generator=g).cuda()
        returns = torch.randn(100, generator=g).cuda()
        before = clone_all(list(m.value_function.parameters()))
        loss = fop.value_update(m, obs, returns, 5)
        assert np.isfinite(loss)
        for p0, p in zip(before, m.value_function.parameters()):
            assert torch.isfinite(p).all() and not torch.equal(p0, p)
