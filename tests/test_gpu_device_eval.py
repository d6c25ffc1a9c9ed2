"""GPU-resident policy evaluation (gpu-marked): the persistent kernels
pendulum_eval_fused / cartpole_eval_fused against the captured multi-kernel
body with torch.equal (both inline the row code of rollout_steps.h and use
the same Philox offsets, so no tolerance applies), the multi-kernel body
against the numpy envs, the early exit, seeding, live weights, isolation,
the gates, the bindings' argument checks, and DDPG / TD3 end to end.

N = 5 (less than one 16-row tile), 16 (exactly one), 37 (two tiles and a
5-row tail).  Pendulum horizon 12, CartPole horizon 20."""
import csv

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
NS = [5, 16, 37]
H_PENDULUM = 12
H_CARTPOLE = 20
CTR_BASE = 1 << 40
ENV_SEED = 0x1234ABCD
SENTINEL = -777
PENDULUM_CASES = [
    ("deterministic", [3, 7, 1]), ("deterministic", [3, 64, 32, 1]),
    ("deterministic", [3, 70, 256, 1]), ("deterministic", [3, 256, 256, 1]),
    ("gaussian", [3, 7, 1]), ("gaussian", [3, 64, 32, 1]),
    # the layer-count ends of the shared forward: one layer (the output stays in
    # the first activation buffer), five (MLP_MAX_LAYERS) ragged, and five wide
    # with narrow layers in between
    ("deterministic", [3, 1]), ("deterministic", [3, 16, 24, 8, 40, 1]),
    ("deterministic", [3, 70, 8, 256, 12, 1]),
    ("gaussian", [3, 1]), ("gaussian", [3, 16, 24, 8, 40, 1]),
]
CARTPOLE_NETS = [[4, 7, 2], [4, 64, 32, 2], [4, 2], [4, 16, 24, 8, 40, 2]]
X_THRESHOLD = 2.4
THETA_THRESHOLD = 12 * 2 * np.pi / 360


def _ids(cases):
    return ["%s-%s" % (m, "x".join(map(str, d))) for m, d in cases]


def _pendulum_policy(mode, dims, torch_seed=77):
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import DeterministicPolicy, GaussianPolicy

    torch.manual_seed(torch_seed)
    if mode == "deterministic":
        net = MLP(dims, activation_function=nn.ReLU,
                  output_activation_function=nn.Tanh).to(DEVICE)
        return DeterministicPolicy(net, ops.make_adam(net.parameters(), lr=1e-3))
    net = MLP(dims).to(DEVICE)
    log_std = nn.Parameter(-0.5 * torch.ones(1, device=DEVICE))
    params = list(net.parameters()) + [log_std]
    return GaussianPolicy(net, ops.make_adam(params, lr=3e-4), log_std)


def _cartpole_policy(dims, torch_seed=77):
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import CategoricalPolicy

    torch.manual_seed(torch_seed)
    net = MLP(dims).to(DEVICE)
    return CategoricalPolicy(net, ops.make_adam(net.parameters(), lr=3e-4))


def _graph(monkeypatch, kind, policy, n, horizon, fused, advance_reset=False):
    """One evaluation graph with counters of its own at the base value."""
    from rl_replicas_amd.ops import fused_rollout as fr

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1" if fused else "0")
    cls = fr.GraphedPendulumEval if kind == "pendulum" else fr.GraphedCartPoleEval
    g = cls(policy, n, horizon, ENV_SEED, fr.make_counter(DEVICE),
            fr.make_counter(DEVICE), advance_reset=advance_reset)
    assert g.fused == fused
    return g


def _run(g):
    g.replay()
    torch.cuda.synchronize()
    return {"returns": g.returns.clone(), "lengths": g.lengths.clone(),
            "init_state": g.init_state.clone(), "ctr": g.ctr.clone(),
            "reset_ctr": g.reset_ctr.clone()}


def _assert_same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------
# 1. persistent kernel == multi-kernel body
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", PENDULUM_CASES, ids=_ids(PENDULUM_CASES))
@pytest.mark.parametrize("n", NS)
def test_pendulum_fused_equals_multi_kernel_body(monkeypatch, n, case):
    mode, dims = case
    policy = _pendulum_policy(mode, dims)
    gf = _graph(monkeypatch, "pendulum", policy, n, H_PENDULUM, True, advance_reset=True)
    gm = _graph(monkeypatch, "pendulum", policy, n, H_PENDULUM, False, advance_reset=True)
    first = None
    for call in range(2):
        f, m = _run(gf), _run(gm)
        _assert_same(f, m)
        assert int(f["ctr"]) == CTR_BASE + (call + 1) * H_PENDULUM
        assert int(f["reset_ctr"]) == CTR_BASE + call + 1
        assert (f["lengths"] == H_PENDULUM).all()
        assert torch.isfinite(f["returns"]).all() and (f["returns"] < 0).all()
        if first is not None:  # fresh init states on the second call
            assert not torch.equal(first["init_state"], f["init_state"])
            assert not torch.equal(first["returns"], f["returns"])
        first = f


@pytest.mark.parametrize("dims", CARTPOLE_NETS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("n", NS)
def test_cartpole_fused_equals_multi_kernel_body(monkeypatch, n, dims):
    policy = _cartpole_policy(dims)
    gf = _graph(monkeypatch, "cartpole", policy, n, H_CARTPOLE, True, advance_reset=True)
    gm = _graph(monkeypatch, "cartpole", policy, n, H_CARTPOLE, False, advance_reset=True)
    for call in range(2):
        f, m = _run(gf), _run(gm)
        _assert_same(f, m)
        assert int(f["ctr"]) == CTR_BASE + (call + 1) * H_CARTPOLE
        assert int(f["reset_ctr"]) == CTR_BASE + call + 1
        assert ((f["lengths"] >= 1) & (f["lengths"] <= H_CARTPOLE)).all()
        assert torch.equal(f["returns"], f["lengths"].double())
        assert (f["init_state"].abs() < 0.05).all()


# ---------------------------------------------------------------------------
# 2. the multi-kernel body against the host envs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["deterministic", "gaussian"])
def test_pendulum_body_matches_the_host_env(monkeypatch, mode):
    """init_state and the recorded actions replayed through
    PendulumEnv._step_b in float64.  The body adds fp32 rewards into a
    double: each carries at most 2**-24 relative rounding, the factor 2
    covers the per-step 1e-12 agreement of the stand-alone kernels."""
    from rl_replicas_amd.envs import PendulumEnv

    n = 37
    g = _graph(monkeypatch, "pendulum", _pendulum_policy(mode, [3, 7, 1]), n,
               H_PENDULUM, False)
    out = _run(g)
    actions = g.act_buf.cpu().numpy()
    assert actions.shape == (H_PENDULUM, n, 1)
    if mode == "gaussian":
        assert np.unique(actions).size > n  # sampled, not one value per row
    ref = PendulumEnv()
    ref.state = out["init_state"].cpu().numpy().copy()
    total, total_abs = np.zeros(n), np.zeros(n)
    for t in range(H_PENDULUM):
        _, reward, _ = ref._step_b(actions[t])
        total += reward
        total_abs += np.abs(reward)
    err = np.abs(out["returns"].cpu().numpy() - total)
    print("max err", err.max(), "min bound", (2.0 ** -23 * total_abs).min())
    assert (err <= 2.0 ** -23 * total_abs).all()


def _cartpole_oracle(init_state, actions, horizon):
    """Per-row first-episode length of CartPoleEnv._step_b under `actions`
    [horizon, n], and the smallest |margin| to a termination threshold over
    the steps of that episode."""
    from rl_replicas_amd.envs import CartPoleEnv

    n = init_state.shape[0]
    ref = CartPoleEnv()
    ref.state = init_state.copy()
    lengths = np.zeros(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    closest = np.full(n, np.inf)
    for t in range(horizon):
        _, _, terminated = ref._step_b(actions[t])
        margin = np.minimum(X_THRESHOLD - np.abs(ref.state[:, 0]),
                            THETA_THRESHOLD - np.abs(ref.state[:, 2]))
        assert ((margin < 0) == terminated).all()
        closest = np.where(live, np.minimum(closest, np.abs(margin)), closest)
        lengths += live
        live &= ~terminated
    return lengths, closest


def test_cartpole_body_matches_the_host_env(monkeypatch):
    """Lengths equal the host env's under the recorded actions, claimed only
    because the oracle's own trajectory stays farther than 1e-9 from both
    thresholds on every step of every first episode (the terminating step
    and the one before it included), which is asserted; the stand-alone
    kernels match the host env to 1e-12 per step."""
    n = 37
    g = _graph(monkeypatch, "cartpole", _cartpole_policy([4, 7, 2]), n, H_CARTPOLE, False)
    out = _run(g)
    actions = g.act_buf.cpu().numpy()
    assert actions.shape == (H_CARTPOLE, n)
    lengths, closest = _cartpole_oracle(out["init_state"].cpu().numpy(), actions,
                                        H_CARTPOLE)
    assert (closest > 1e-9).all()
    # both kinds of ending are in the case
    assert (lengths < H_CARTPOLE).any() and (lengths == H_CARTPOLE).any()
    assert np.array_equal(out["lengths"].cpu().numpy(), lengths)
    assert np.array_equal(out["returns"].cpu().numpy(), lengths.astype(np.float64))


# ---------------------------------------------------------------------------
# 3. early exit
# ---------------------------------------------------------------------------
def test_cartpole_early_exit(monkeypatch):
    """An untrained net keeps no pole up for 200 steps (2000 random-action
    host episodes ended by step 90), so horizons 500 and 200 from the same
    seeds are the same episodes, and the horizon-500 loop leaves through the
    all-rows-finished exit."""
    policy = _cartpole_policy([4, 64, 32, 2])
    long = _run(_graph(monkeypatch, "cartpole", policy, 37, 500, True))
    short = _run(_graph(monkeypatch, "cartpole", policy, 37, 200, True))
    assert (long["lengths"] < 200).all() and (long["lengths"] >= 1).all()
    for k in ("returns", "lengths", "init_state"):
        assert torch.equal(long[k], short[k]), k
    assert int(long["ctr"]) == CTR_BASE + 500 and int(short["ctr"]) == CTR_BASE + 200


# ---------------------------------------------------------------------------
# 4. seeding and streams (through the public class)
# ---------------------------------------------------------------------------
def _pendulum_env(n=1, horizon=H_PENDULUM):
    from rl_replicas_amd.envs import DevicePendulumEnv

    return DevicePendulumEnv(n, device=DEVICE, max_episode_steps=horizon)


def _cartpole_env(n=1, horizon=H_CARTPOLE):
    from rl_replicas_amd.envs import DeviceCartPoleEnv

    return DeviceCartPoleEnv(n, device=DEVICE, max_episode_steps=horizon)


def _counters(ev):
    (ctr, reset_ctr), = ev._counters.values()
    return int(ctr.item()), int(reset_ctr.item())


def test_seeding_and_streams(monkeypatch):
    from rl_replicas_amd.evaluator import DeviceEvaluator

    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", raising=False)
    env = _pendulum_env()
    gauss = _pendulum_policy("gaussian", [3, 7, 1])
    ev = DeviceEvaluator(seed=3)
    r0, l0 = ev.evaluate(gauss, env, 16)
    assert ev.last_path == "fused" and l0 == [H_PENDULUM] * 16
    s0 = ev.last_initial_state.clone()
    r1, _ = ev.evaluate(gauss, env, 16)
    assert torch.equal(s0, ev.last_initial_state)  # reseed-on-every-call
    assert r0 != r1                                # fresh actions
    assert _counters(ev) == (CTR_BASE + 2 * H_PENDULUM, CTR_BASE)

    det = _pendulum_policy("deterministic", [3, 7, 1])
    ev = DeviceEvaluator(seed=3)
    a = ev.evaluate(det, env, 16)
    assert torch.equal(s0, ev.last_initial_state)  # the seed alone fixes them
    b = ev.evaluate(det, env, 16)
    assert a == b

    ev = DeviceEvaluator(seed=None)
    ev.evaluate(det, env, 16)
    u0 = ev.last_initial_state.clone()
    ev.evaluate(det, env, 16)
    assert not torch.equal(u0, ev.last_initial_state)
    assert _counters(ev) == (CTR_BASE + 2 * H_PENDULUM, CTR_BASE + 2)

    cat = _cartpole_policy([4, 7, 2])
    ev = DeviceEvaluator(seed=3)
    returns, lengths = ev.evaluate(cat, _cartpole_env(), 16)
    assert ev.last_path == "fused"
    assert returns == [float(length) for length in lengths]
    c0 = ev.last_initial_state.clone()
    ev.evaluate(cat, _cartpole_env(), 16)
    assert torch.equal(c0, ev.last_initial_state)


# ---------------------------------------------------------------------------
# 5. live weights
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_weights_are_read_by_pointer(monkeypatch, fused):
    from rl_replicas_amd.evaluator import DeviceEvaluator

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1" if fused else "0")
    policy = _pendulum_policy("deterministic", [3, 64, 32, 1])
    env = _pendulum_env()
    ev = DeviceEvaluator(seed=3)
    before = ev.evaluate(policy, env, 16)
    assert ev.last_path == ("fused" if fused else "graph")
    with torch.no_grad():
        for p in policy.parameters():
            p.mul_(-1.5)
    after = ev.evaluate(policy, env, 16)
    assert len(ev._graphs) == 1  # the cached graph
    fresh = DeviceEvaluator(seed=3).evaluate(policy, env, 16)
    assert after == fresh
    assert after != before


# ---------------------------------------------------------------------------
# 6. isolation
# ---------------------------------------------------------------------------
def test_evaluation_leaves_training_state_alone(monkeypatch):
    from rl_replicas_amd.evaluator import DeviceEvaluator
    from rl_replicas_amd.policies import RandomPolicy
    from rl_replicas_amd.replay_buffer import ReplayBuffer
    from rl_replicas_amd.samplers import DeviceReplaySampler

    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", raising=False)
    env = _pendulum_env(5, horizon=4)
    buf = ReplayBuffer(256, device=DEVICE)
    sampler = DeviceReplaySampler(env, buf, seed=5)
    buf.add_experience(sampler.sample(5 * 6, RandomPolicy(env.action_space)))
    torch.cuda.synchronize()
    assert sampler._graph_ctr is not None
    keep = {
        "state": env.state.clone(), "elapsed": env._elapsed,
        "offset": env._philox_offset, "ctr": sampler._graph_ctr.clone(),
        "write_dev": buf._write_dev.clone(), "size_dev": buf._size_dev.clone(),
        "ring": {k: v[:30].clone() for k, v in buf._storage.items()},
    }
    ev = DeviceEvaluator(seed=3)
    ev.evaluate(_pendulum_policy("deterministic", [3, 7, 1]), env, 16)
    assert ev.last_path == "fused"
    torch.cuda.synchronize()
    assert torch.equal(env.state, keep["state"])
    assert env._elapsed == keep["elapsed"] and env._philox_offset == keep["offset"]
    assert torch.equal(sampler._graph_ctr, keep["ctr"])
    assert torch.equal(buf._write_dev, keep["write_dev"])
    assert torch.equal(buf._size_dev, keep["size_dev"])
    for k, v in keep["ring"].items():
        assert torch.equal(buf._storage[k][:30], v), k

    cenv = _cartpole_env(5)
    cenv.reset(seed=9)
    cenv.step(torch.ones(5, dtype=torch.int64, device=DEVICE))
    state, elapsed = cenv.state.clone(), cenv.elapsed.clone()
    ev.evaluate(_cartpole_policy([4, 7, 2]), cenv, 16)
    assert ev.last_path == "fused"
    assert torch.equal(cenv.state, state) and torch.equal(cenv.elapsed, elapsed)


# ---------------------------------------------------------------------------
# 7. gates
# ---------------------------------------------------------------------------
def test_gates(monkeypatch):
    from rl_replicas_amd.evaluator import DeviceEvaluator
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.ops import fused_rollout as fr
    from rl_replicas_amd.policies import DeterministicPolicy, RandomPolicy

    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", raising=False)
    env, cenv = _pendulum_env(), _cartpole_env()
    det = _pendulum_policy("deterministic", [3, 64, 32, 1])
    gauss = _pendulum_policy("gaussian", [3, 7, 1])
    cat = _cartpole_policy([4, 64, 32, 2])
    assert fr.pendulum_eval_mode(det) == "deterministic"
    assert fr.pendulum_eval_mode(gauss) == "gaussian"
    assert fr.pendulum_eval_mode(cat) is None
    assert fr.pendulum_eval_mode(RandomPolicy(env.action_space)) is None
    assert fr.pendulum_eval_fused_eligible(det) and fr.pendulum_eval_fused_eligible(gauss)
    assert fr.cartpole_eval_fused_eligible(cat) and not fr.cartpole_eval_fused_eligible(det)

    def path(policy, e, n=5, **kw):
        ev = DeviceEvaluator(seed=3, **kw)
        _, lengths = ev.evaluate(policy, e, n)
        assert len(lengths) == n
        return ev.last_path

    assert path(det, env) == "fused" and path(cat, cenv) == "fused"
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "0")
    assert path(det, env) == "graph" and path(cat, cenv) == "graph"
    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED")

    monkeypatch.setenv("RL_REPLICAS_AMD_COMPUTE_DTYPE", "bf16")
    assert path(det, env) == "graph" and path(cat, cenv) == "graph"
    monkeypatch.delenv("RL_REPLICAS_AMD_COMPUTE_DTYPE")

    # a wide categorical net: the CartPole kernel is narrow-only
    assert path(_cartpole_policy([4, 70, 2]), cenv) == "graph"

    from rl_replicas_amd.envs import PendulumEnv

    host = PendulumEnv()
    host.spec.max_episode_steps = H_PENDULUM
    assert path(det, host) == "fused"
    # nets no fused-MLP kernel takes run as the host Evaluator does (which
    # steps host envs only)
    for dims in ([3, 300, 1], [3, 8, 8, 8, 8, 8, 1]):  # width 300, 6 layers
        net = MLP(dims, activation_function=nn.ReLU,
                  output_activation_function=nn.Tanh).to(DEVICE)
        wide = DeterministicPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3))
        assert path(wide, host) == "host"
    assert path(RandomPolicy(host.action_space), host) == "host"
    assert path(det, host, device="cpu") == "host"  # the policy is on another device

    monkeypatch.setenv("RL_REPLICAS_AMD_DISABLE_GRAPHS", "1")
    assert path(det, env) == "eager" and path(cat, cenv) == "eager"
    monkeypatch.delenv("RL_REPLICAS_AMD_DISABLE_GRAPHS")

    # at most 8 graphs: the ninth distinct key runs eager, cached ones still replay
    ev = DeviceEvaluator(seed=3)
    tiny = _pendulum_env(horizon=3)
    for n in range(1, 9):
        ev.evaluate(det, tiny, n)
        assert ev.last_path == "fused"
    ninth = ev.evaluate(det, tiny, 9)
    assert ev.last_path == "eager" and len(ev._graphs) == 8
    assert ninth[1] == [3] * 9
    ev.evaluate(det, tiny, 8)
    assert ev.last_path == "fused"


# ---------------------------------------------------------------------------
# 8. the bindings check their arguments before launching
# ---------------------------------------------------------------------------
def test_bindings_check_arguments_before_launching():
    from rl_replicas_amd import ops
    from rl_replicas_amd.ops import fused_rollout as fr
    from rl_replicas_amd.ops.fused_mlp import _extract_layers

    ext = ops._load_extension()
    n = 5

    def outputs(state_dim):
        return [torch.full((n,), float(SENTINEL), dtype=torch.float64, device=DEVICE),
                torch.full((n,), SENTINEL, dtype=torch.int32, device=DEVICE),
                torch.full((n, state_dim), float(SENTINEL), dtype=torch.float64,
                           device=DEVICE)]

    def layers(policy):
        w, b, acts = _extract_layers(policy.network)
        return [t.detach() for t in w], [t.detach() for t in b], list(acts)

    ctr, reset_ctr = fr.make_counter(DEVICE), fr.make_counter(DEVICE)
    w3, b3, a3 = layers(_pendulum_policy("deterministic", [3, 7, 1]))
    w4, b4, a4 = layers(_cartpole_policy([4, 7, 2]))
    log_std = torch.zeros(1, device=DEVICE)

    def pendulum(out, w=w3, b=b3, acts=a3, mode=0, ls=None, horizon=4, c=ctr, rc=reset_ctr,
                 wide=1024):
        ext.pendulum_eval_fused(w, b, acts, mode, ls, 1, 2, horizon, c, rc, *out, wide)

    def cartpole(out, w=w4, b=b4, acts=a4, horizon=4, c=ctr, rc=reset_ctr):
        ext.cartpole_eval_fused(w, b, acts, 1, 2, horizon, c, rc, *out)

    def swapped(out, i, t):
        return [t if j == i else o for j, o in enumerate(out)]

    po, co = outputs(2), outputs(4)
    wide4, bwide4, awide4 = layers(_cartpole_policy([4, 70, 2]))
    bad = [
        # wrong dtype
        lambda: pendulum(po, w=[w3[0].double()] + w3[1:]),
        lambda: cartpole(co, b=[b4[0].half()] + b4[1:]),
        lambda: pendulum(swapped(po, 0, po[0].float())),
        lambda: cartpole(swapped(co, 1, co[1].long())),
        lambda: pendulum(swapped(po, 2, po[2].float())),
        lambda: pendulum(po, c=ctr.int()),
        lambda: pendulum(po, mode=1, ls=log_std.double()),
        # CPU tensors
        lambda: pendulum(po, w=[w3[0].cpu()] + w3[1:]),
        lambda: cartpole(swapped(co, 0, co[0].cpu())),
        lambda: cartpole(co, rc=reset_ctr.cpu()),
        lambda: pendulum(po, mode=1, ls=log_std.cpu()),
        # dims[0] / dims[L]
        lambda: pendulum(po, w=w4, b=b4, acts=a4),   # [4, 7, 2]
        lambda: cartpole(co, w=w3, b=b3, acts=a3),   # [3, 7, 1]
        lambda: pendulum(po, w=w3[:1], b=b3[:1], acts=a3[:1]),  # head 7 wide
        # a wide net to the CartPole kernel
        lambda: cartpole(co, w=wide4, b=bwide4, acts=awide4),
        # mis-sized outputs
        lambda: pendulum(swapped(po, 0, po[0][:4])),
        lambda: cartpole(swapped(co, 1, torch.cat([co[1], co[1]]))),
        lambda: pendulum(swapped(po, 2, co[2])),
        lambda: cartpole(swapped(co, 2, po[2])),
        # horizon, mode, log_std, workgroup size
        lambda: pendulum(po, horizon=0),
        lambda: cartpole(co, horizon=0),
        lambda: pendulum(po, mode=2),
        lambda: pendulum(po, mode=1),
        lambda: pendulum(po, mode=1, ls=torch.zeros(2, device=DEVICE)),
        lambda: pendulum(po, wide=512),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        for t in po + co:
            assert (t == SENTINEL).all(), i
    assert int(ctr.item()) == CTR_BASE and int(reset_ctr.item()) == CTR_BASE

    rew = torch.ones(4, n, device=DEVICE)
    done = torch.zeros(4, n, dtype=torch.uint8, device=DEVICE)
    ret, length = po[0], po[1]
    bad_reduce = [
        lambda: ext.episode_reduce(rew.double(), done, ret, length),
        lambda: ext.episode_reduce(rew.cpu(), done, ret, length),
        lambda: ext.episode_reduce(rew, done.float(), ret, length),
        lambda: ext.episode_reduce(rew, done[:3], ret, length),
        lambda: ext.episode_reduce(rew, done, ret.float(), length),
        lambda: ext.episode_reduce(rew, done, ret, length[:4]),
        lambda: ext.episode_reduce(rew[0], None, ret, length),
    ]
    for i, call in enumerate(bad_reduce):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert (ret == SENTINEL).all() and (length == SENTINEL).all(), i

    # and the good calls do write
    pendulum(po)
    cartpole(co)
    torch.cuda.synchronize()
    assert (po[1] == 4).all() and (po[0] < 0).all()
    assert ((co[1] >= 1) & (co[1] <= 4)).all()
    done[1, 2] = 1
    rew[:, 0] = torch.tensor([0.5, 0.25, 2.0, 4.0], device=DEVICE)
    ext.episode_reduce(rew, done, ret, length)
    assert length.tolist() == [4, 4, 2, 4, 4] and ret.tolist() == [6.75, 4.0, 2.0, 4.0, 4.0]
    ext.episode_reduce(rew, None, ret, length)
    assert length.tolist() == [4] * 5


def test_limits_match_the_gates():
    from rl_replicas_amd import ops

    ext = ops._load_extension()
    layers, width, lds = ext.pendulum_eval_fused_limits()
    assert (layers, width) == tuple(ext.fused_mlp_limits()[:2])
    assert ext.pendulum_eval_fused_lds_bytes([3, 256, 256, 1]) <= lds
    assert ext.pendulum_eval_fused_lds_bytes([3, 64, 32, 1]) <= lds
    layers, width, lds = ext.cartpole_eval_fused_limits()
    assert width == 64
    assert ext.cartpole_eval_fused_lds_bytes([4, 64, 32, 2]) <= lds
    with pytest.raises(RuntimeError):
        ext.cartpole_eval_fused_lds_bytes([4, 70, 2])


# ---------------------------------------------------------------------------
# 9. end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_off_policy_end_to_end(tmp_path, monkeypatch, algo):
    from rl_replicas_amd import ops
    from rl_replicas_amd.algorithms import DDPG, TD3
    from rl_replicas_amd.evaluator import DeviceEvaluator
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import RandomPolicy
    from rl_replicas_amd.q_function import QFunction
    from rl_replicas_amd.replay_buffer import ReplayBuffer
    from rl_replicas_amd.samplers import DeviceReplaySampler

    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", raising=False)
    torch.manual_seed(0)
    env = _pendulum_env(1, horizon=10)
    policy = _pendulum_policy("deterministic", [3, 32, 1], torch_seed=0)
    qnets = [MLP([4, 32, 1], activation_function=nn.ReLU).to(DEVICE)
             for _ in range(2 if algo == "td3" else 1)]
    qs = [QFunction(q, ops.make_adam(q.parameters(), lr=1e-3)) for q in qnets]
    buf = ReplayBuffer(1024, device=DEVICE)
    sampler = DeviceReplaySampler(env, buf, seed=3)
    ev = DeviceEvaluator(seed=4)
    calls = []
    evaluate = ev.evaluate

    def spy(*args):
        out = evaluate(*args)
        calls.append((out, ev.last_path))
        return out

    ev.evaluate = spy
    cls = TD3 if algo == "td3" else DDPG
    model = cls(policy, RandomPolicy(env.action_space), *qs, env, sampler, buf, ev)
    # learn() evaluates in a host env made from the id: give it the horizon
    model.evaluation_env.spec.max_episode_steps = 10
    model.learn(num_epochs=3, batch_size=10, minibatch_size=8, num_start_steps=10,
                num_steps_before_update=10, num_train_steps=2,
                num_evaluation_episodes=5, evaluation_interval=10,
                output_dir=str(tmp_path))
    torch.cuda.synchronize()
    assert len(calls) == 3
    for (returns, lengths), path in calls:
        assert path == "fused"
        assert lengths == [10] * 5
        assert len(returns) == 5 and all(np.isfinite(returns)) and all(r < 0 for r in returns)
    assert calls[0][0] != calls[2][0]  # the actor moved between evaluations
    assert len(ev._graphs) == 1
    with open(tmp_path / "metrics.csv") as f:
        tags = [row[0] for row in csv.reader(f)]
    assert tags.count("evaluation/average_episode_return") == 3
    assert tags.count("evaluation/average_episode_length") == 3
    assert tags.count("phase_ms/evaluate") == 3
