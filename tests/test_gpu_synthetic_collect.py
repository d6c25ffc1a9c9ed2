"""Device-side replay collection on the synthetic DeviceVectorEnv (gpu-marked):
the persistent kernel synthetic_collect_fused against the captured
multi-kernel body with torch.equal (both inline the row code of
rollout_steps.h and use the same Philox offsets, so no tolerance applies),
ring placement, the transition against the numpy env, the two behaviour
policies, the gate, the bindings' argument checks, mixing with eager epochs
and host adds, and DDPG / TD3 end to end.

N = 5 (less than one 16-row tile), 16 (exactly one), 37 (two tiles and a
5-row tail); steps = 6 with horizon 4, so the first epoch cuts after step 3
and the carried second one after steps 1 and 5.  Envs: Ant-v4 (27, 8), a
test-registered (5, 3) and a test-registered (64, 2) whose lane 63 owns a
state column.  Nets (ReLU, Tanh head): narrow [27,64,32,8], [5,8,3], [5,3]
(one layer), [5,16,24,8,40,3] (five, MLP_MAX_LAYERS), [64,8,2]; wide
[27,256,256,8] (the benchmark actor), [5,70,256,3] (K = 5 has 4-block and
tail, K = 70 8-blocks, the 4-block and a tail, K = 256 8-blocks only) and
[5,70,8,256,12,3] (wide with narrow layers in between)."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
NS = [5, 16, 37]
AWKWARD_ID = "CollectAwkward-v0"   # (5, 3)
LANE63_ID = "CollectLane63-v0"     # (64, 2)
OVER_ID = "CollectOverBudget-v0"   # (64, 12): wide tiles + env image > 100 KiB
SHAPES = {"Ant-v4": (27, 8), AWKWARD_ID: (5, 3), LANE63_ID: (64, 2), OVER_ID: (64, 12)}
NETS = {"bench_narrow": ("Ant-v4", [27, 64, 32, 8]),
        "awkward": (AWKWARD_ID, [5, 8, 3]),
        "one_layer": (AWKWARD_ID, [5, 3]),
        "five_layers": (AWKWARD_ID, [5, 16, 24, 8, 40, 3]),
        "lane63": (LANE63_ID, [64, 8, 2]),
        "bench_wide": ("Ant-v4", [27, 256, 256, 8]),
        "ragged_wide": (AWKWARD_ID, [5, 70, 256, 3]),
        "five_layers_wide": (AWKWARD_ID, [5, 70, 8, 256, 12, 3])}
WIDE = ["bench_wide", "ragged_wide", "five_layers_wide"]
# the uniform draw reads no net: one net per env
CASES = [(net, "noised") for net in NETS] + [
    (net, "uniform") for net in ("bench_narrow", "awkward", "lane63")]
STEPS = 6
HORIZON = 4
CTR_BASE = 1 << 40
CUTS_FROM_RESET = (3,)
CUTS_CARRY = (1, 5)  # elapsed 2 after the first epoch
RING = ("observations", "actions", "rewards", "next_observations", "dones")
SENTINEL = -777.0
LIMIT = 1.0  # the synthetic envs' Box(-1, 1)


def _register():
    from rl_replicas_amd.envs.core import register, registered_ids
    from rl_replicas_amd.envs.synthetic import SyntheticEnv

    for env_id in (AWKWARD_ID, LANE63_ID, OVER_ID):
        if env_id not in registered_ids():
            o, a = SHAPES[env_id]
            register(env_id, lambda env_id=env_id, o=o, a=a, **kw: SyntheticEnv(env_id, o, a, **kw))


def _actor(dims, dtype=None):
    from rl_replicas_amd import ops
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import DeterministicPolicy

    net = MLP(dims, activation_function=nn.ReLU,
              output_activation_function=nn.Tanh).to(DEVICE)
    if dtype is not None:
        net.to(dtype)
    return net, DeterministicPolicy(net, ops.make_adam(net.parameters(), lr=1e-3))


class World:
    def __init__(self, n, net="awkward", cap=4096, noise=0.1, torch_seed=77, seed=5,
                 horizon=HORIZON, env_device=DEVICE, env_noise=None):
        from rl_replicas_amd.envs import DeviceVectorEnv
        from rl_replicas_amd.policies import RandomPolicy
        from rl_replicas_amd.replay_buffer import ReplayBuffer
        from rl_replicas_amd.samplers import DeviceReplaySampler
        from rl_replicas_amd.utils import add_noise_to_get_action

        _register()
        torch.manual_seed(torch_seed)
        env_id, dims = NETS[net] if isinstance(net, str) else net
        self.n = n
        self.O, self.A = SHAPES[env_id]
        env_kw = {} if env_noise is None else {"noise": env_noise}
        self.env = DeviceVectorEnv(env_id, n, device=env_device,
                                   max_episode_steps=horizon, **env_kw)
        self.buf = ReplayBuffer(cap, device=DEVICE)
        self.sampler = DeviceReplaySampler(self.env, self.buf, seed=seed)
        self.net, self.det = _actor(dims)
        self.policies = {
            "noised": add_noise_to_get_action(self.det, self.env.action_space, noise),
            "uniform": RandomPolicy(self.env.action_space),
        }
        # torch.empty storage may hold NaNs: whole-ring compares need values
        storage, _, _ = self.buf.device_ring(self.O, (self.A,))
        for t in storage:
            t.fill_(SENTINEL)

    def epoch(self, mode, steps=STEPS):
        """One sample() + add_experience(); a snapshot of everything."""
        before = set(self.sampler._graphs)
        write_before = self.buf._write
        policy = self.policies[mode] if isinstance(mode, str) else mode
        exp = self.sampler.sample(self.n * steps, policy)
        self.buf.add_experience(exp)
        torch.cuda.synchronize()
        snap = {
            "exp": exp, "write_before": write_before, "write": self.buf._write,
            "len": len(self.buf), "new_keys": set(self.sampler._graphs) - before,
            "state": self.env.state.clone(),
            "ring": {k: v.clone() for k, v in self.buf._storage.items()},
            "write_dev": int(self.buf._write_dev.item()),
            "size_dev": int(self.buf._size_dev.item()),
        }
        if self.sampler._graph_ctr is not None:
            snap["ctr"] = int(self.sampler._graph_ctr.item())
        return snap

    def graph(self, cuts, reset, mode, steps=STEPS):
        return self.sampler._graphs[(steps, cuts, reset, mode)]


def _two_epochs(monkeypatch, fused, n, net, mode, **kw):
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1" if fused else "0")
    w = World(n, net, **kw)
    out = []
    for cuts, reset in ((CUTS_FROM_RESET, True), (CUTS_CARRY, False)):
        snap = w.epoch(mode)
        # on the code before this feature no graph exists and this lookup fails
        g = w.graph(cuts, reset, mode)
        snap["g"] = g
        snap["seg_returns"] = g.seg_returns.clone()
        snap["carry"] = g.carry.clone()
        out.append(snap)
    return w, out


def _rows(snap, n, steps=STEPS, cap=None):
    """The epoch's transitions as [n, steps, ...] views of the ring clone."""
    cap = cap or snap["ring"]["rewards"].shape[0]
    idx = (snap["write_before"] + torch.arange(n * steps, device=DEVICE)) % cap
    return {k: v[idx].view(n, steps, *v.shape[1:]) for k, v in snap["ring"].items()}


# ---------------------------------------------------------------------------
# 1. fused equals multi-kernel body
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("net,mode", CASES)
@pytest.mark.parametrize("n", NS)
def test_fused_equals_multi_kernel_body(monkeypatch, n, net, mode):
    wf, f = _two_epochs(monkeypatch, True, n, net, mode)
    _, p = _two_epochs(monkeypatch, False, n, net, mode)
    for e, (a, b) in enumerate(zip(f, p)):
        assert a["g"].fused and not b["g"].fused
        assert a["g"].mode == b["g"].mode == mode
        assert a["ctr"] == b["ctr"] == CTR_BASE + (e + 1) * (2 * STEPS + 1)
        for k in RING:
            assert torch.equal(a["ring"][k], b["ring"][k]), f"{k} differs in epoch {e}"
        for k in ("state", "seg_returns", "carry"):
            assert torch.equal(a[k], b[k]), f"{k} differs in epoch {e}"
        assert torch.equal(a["state"], a["carry"])
        for k in ("write", "len", "write_dev", "size_dev"):
            assert a[k] == b[k] == (e + 1) * n * STEPS, k
        ea, eb = a["exp"], b["exp"]
        assert ea.episode_returns == eb.episode_returns
        assert ea.episode_lengths == eb.episode_lengths
        assert all(np.array_equal(x, y) for x, y in zip(ea.dones, eb.dones))
        assert ea.stored_in_buffer is wf.buf and getattr(ea, "_flat_cache", None) is None
    # the structure DeviceSampler._build_experience gives
    assert f[0]["exp"].episode_lengths == [4, 2] * n
    assert f[1]["exp"].episode_lengths == [2, 4] * n
    assert [d.tolist() for d in f[0]["exp"].dones[:2]] == [[False] * 3 + [True],
                                                           [False, False]]
    assert f[0]["exp"].episode_returns == [
        float(x) for x in f[0]["seg_returns"].cpu().numpy().reshape(-1)]
    # the epochs draw fresh randomness
    assert not torch.equal(_rows(f[0], n)["actions"], _rows(f[1], n)["actions"])
    for k in RING:
        assert torch.isfinite(f[1]["ring"][k][: 2 * n * STEPS]).all(), k
        assert (f[1]["ring"][k][: 2 * n * STEPS] != SENTINEL).all(), k


@pytest.mark.parametrize("net", WIDE)
def test_wide_workgroup_sizes_agree(monkeypatch, net):
    """The wide regime at 1024 threads (one column tile and one env row per
    wave) writes the bytes it writes at 256 (four of each per wave)."""
    n = 37
    monkeypatch.setenv("RL_REPLICAS_AMD_COLLECT_WG", "256")
    _, a = _two_epochs(monkeypatch, True, n, net, "noised")
    monkeypatch.setenv("RL_REPLICAS_AMD_COLLECT_WG", "1024")
    _, b = _two_epochs(monkeypatch, True, n, net, "noised")
    for x, y in zip(a, b):
        assert x["g"].fused and y["g"].fused
        for k in RING:
            assert torch.equal(x["ring"][k], y["ring"][k]), k
        for k in ("state", "seg_returns", "carry"):
            assert torch.equal(x[k], y[k]), k


# ---------------------------------------------------------------------------
# 2. ring placement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap_kind", ["exact", "wrap_mid_row", "large"])
@pytest.mark.parametrize("n", [5, 37])
def test_ring_placement(monkeypatch, n, cap_kind):
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    ne = n * STEPS
    cap = {"exact": ne, "wrap_mid_row": ne * 3 // 2, "large": 4 * ne + 3}[cap_kind]
    ref_w = World(n, "bench_narrow", cap=4096)
    ref = [ref_w.epoch("noised"), ref_w.epoch("noised")]
    w = World(n, "bench_narrow", cap=cap)
    got = [w.epoch("noised"), w.epoch("noised")]
    assert all(g.fused for g in w.sampler._graphs.values()) and len(w.sampler._graphs) == 2
    owner = torch.full((cap,), -1, dtype=torch.int64)  # epoch that wrote the slot
    for e in range(2):
        assert got[e]["write_before"] == (e * ne) % cap
        want = _rows(ref[e], n)
        have = _rows(got[e], n, cap=cap)
        for k in RING:  # slot of (row, t) = (write_before + row * steps + t) % cap
            assert torch.equal(want[k], have[k]), (k, e)
        owner[(got[e]["write_before"] + torch.arange(ne)) % cap] = e
        assert got[e]["len"] == got[e]["size_dev"] == min((e + 1) * ne, cap)
        assert got[e]["write"] == got[e]["write_dev"] == ((e + 1) * ne) % cap
    assert len(w.buf) == got[1]["len"]
    final = got[1]["ring"]
    if cap_kind == "wrap_mid_row":
        row, t = divmod(cap - ne, STEPS)
        assert t != 0 and 0 < row < n  # the wrap falls inside a row
        assert (owner == 0).sum() == cap - ne and (owner == -1).sum() == 0
    if cap_kind == "exact":
        assert (owner == 1).all()
    # slots the second epoch left alone still hold the first epoch's rows ...
    first = _rows(ref[0], n)
    kept = torch.nonzero(owner[:ne] == 0).flatten().to(DEVICE)
    for k in RING:
        flat = first[k].reshape(ne, *first[k].shape[2:])
        assert torch.equal(final[k][kept], flat[kept]), k
    # ... and the ones nobody wrote keep the sentinel
    untouched = torch.nonzero(owner == -1).flatten().to(DEVICE)
    assert (cap_kind == "large") == (untouched.numel() > 0)
    for k in RING:
        assert (final[k][untouched] == SENTINEL).all(), k


def test_more_transitions_than_the_ring_holds_falls_back(monkeypatch):
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    n = 5
    cap = n * STEPS - 1
    w = World(n, cap=cap)
    snap = w.epoch("noised")
    assert not w.sampler._graphs
    exp = snap["exp"]
    assert getattr(exp, "stored_in_buffer", None) is None
    flat = exp.to_flat_batch()
    assert snap["len"] == snap["size_dev"] == cap and snap["write"] == snap["write_dev"] == 0
    for ring_key, flat_key in zip(RING, ("observations", "actions", "rewards",
                                         "next_observations", "step_dones")):
        assert torch.equal(snap["ring"][ring_key], flat[flat_key][-cap:]), ring_key


# ---------------------------------------------------------------------------
# 3. transition semantics against the host env
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["bench_narrow", "bench_wide", "lane63"])
def test_transitions_match_the_host_env(monkeypatch, net):
    """Every stored (obs, act) through ONE SyntheticEnv._step_b (dynamics
    noise 0): the stored successor and reward within atol 1e-5, the
    tolerance tests/test_device_env.py uses for this step.  Nothing
    accumulates: each transition starts from the stored fp32 row."""
    from rl_replicas_amd.envs import make

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    n = 37
    w = World(n, net, noise=0.5, env_noise=0.0)
    assert w.env.noise == 0.0
    snaps = [w.epoch("noised"), w.epoch("noised")]
    assert w.graph(CUTS_FROM_RESET, True, "noised").fused
    assert w.graph(CUTS_CARRY, False, "noised").fused
    ref = make(NETS[net][0], noise=0.0)
    ref.reset(seed=0)
    worst_s = worst_r = 0.0
    for snap in snaps:
        rows = {k: v.cpu().numpy() for k, v in _rows(snap, n).items()}
        obs = rows["observations"].reshape(n * STEPS, w.O)
        act = rows["actions"].reshape(n * STEPS, w.A)
        ref.state = obs.copy()
        nxt, rew, _ = ref._step_b(act)
        ds = np.abs(nxt - rows["next_observations"].reshape(n * STEPS, w.O)).max()
        dr = np.abs(rew - rows["rewards"].reshape(-1)).max()
        worst_s, worst_r = max(worst_s, ds), max(worst_r, dr)
    print(f"{net}: max |successor diff| {worst_s:.3e}, max |reward diff| {worst_r:.3e}")
    assert worst_s <= 1e-5 and worst_r <= 1e-5


@pytest.mark.parametrize("net", ["bench_narrow", "lane63"])
def test_chaining_and_cuts(monkeypatch, net):
    """Default dynamics noise: off the cuts the stored successor IS the next
    stored observation; on a cut done = 1 and the next observation is a
    fresh 0.1 * normal draw, not the stored successor."""
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    n = 37
    w = World(n, net, noise=0.5)
    first = w.epoch("noised")
    second = w.epoch("noised")
    assert w.graph(CUTS_CARRY, False, "noised").fused
    r1 = _rows(first, n)
    # the epoch reset is a fresh draw too, and the carried epoch starts from
    # the first epoch's carry
    assert (r1["observations"][:, 0].abs() < 1.0).all()
    rows = _rows(second, n)
    assert torch.equal(rows["observations"][:, 0], first["state"])
    for t in range(STEPS):
        nxt = rows["next_observations"][:, t]
        after = rows["observations"][:, t + 1] if t + 1 < STEPS else second["state"]
        if t in CUTS_CARRY:
            assert (rows["dones"][:, t] == 1.0).all()
            assert (after.abs() < 1.0).all()
            assert not torch.equal(after, nxt)
            assert (after != nxt).any(dim=1).all()
        else:
            assert (rows["dones"][:, t] == 0.0).all()
            assert torch.equal(after, nxt), t
    assert (rows["next_observations"].abs() <= 1.0).all()  # tanh


# ---------------------------------------------------------------------------
# 4. actions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "multi"])
@pytest.mark.parametrize("net", list(NETS))
def test_noise_zero_actions_are_the_actor_forward(monkeypatch, net, fused):
    from rl_replicas_amd import ops
    from rl_replicas_amd.ops.fused_mlp import _extract_layers

    n = 37
    w, snaps = _two_epochs(monkeypatch, fused, n, net, "noised", noise=0.0)
    weights, biases, acts = _extract_layers(w.net)
    ext = ops._load_extension()
    for snap in snaps:
        assert snap["g"].fused == fused
        rows = _rows(snap, n)
        obs = rows["observations"].reshape(-1, w.O).contiguous()
        mean = ext.mlp_forward(obs, list(weights), list(biases), acts, False, 0)[0]
        want = mean.clamp(-LIMIT, LIMIT)
        assert torch.equal(rows["actions"].reshape(-1, w.A), want)
        assert want.abs().max() > 0


def test_noised_actions_are_clipped_to_the_limit(monkeypatch):
    n = 37
    _, snaps = _two_epochs(monkeypatch, True, n, "bench_wide", "noised", noise=10.0)
    acts = torch.cat([_rows(s, n)["actions"].flatten() for s in snaps])
    assert (acts >= -LIMIT).all() and (acts <= LIMIT).all()
    assert (acts == LIMIT).any() and (acts == -LIMIT).any()
    assert ((acts > -LIMIT) & (acts < LIMIT)).any()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "multi"])
def test_uniform_actions(monkeypatch, fused):
    n = 37
    w, snaps = _two_epochs(monkeypatch, fused, n, "bench_narrow", "uniform")
    draws = []
    for snap in snaps:
        assert snap["g"].fused == fused
        a = _rows(snap, n)["actions"]
        assert (a > -1.0).all() and (a < 1.0).all()  # strictly inside (low, high)
        # no two of the N * steps * A draws of an epoch are equal
        assert a.flatten().unique().numel() == n * STEPS * w.A
        # the element index is row * A + d: the columns of one row differ
        cols = a.reshape(-1, w.A)
        assert (cols[:, 1:] != cols[:, :1]).all()
        draws.append(a.flatten())
    a = torch.cat(draws).double()
    count = a.numel()
    assert count >= 2000
    bound = 5 * (2 / math.sqrt(12)) / math.sqrt(count)
    print(f"mean of {count} uniform draws {a.mean().item():.3e}, bound {bound:.3e}")
    assert abs(a.mean().item()) <= bound
    assert a.min() < -0.95 and a.max() > 0.95


def test_noised_columns_of_a_row_differ(monkeypatch):
    """A zero net and noise 0.3: every action is pure noise, keyed by
    row * A + d, so no two columns of a row and no two rows agree."""
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    n = 16
    w = World(n, "bench_narrow", noise=0.3)
    with torch.no_grad():
        for p in w.net.parameters():
            p.zero_()
    a = _rows(w.epoch("noised"), n)["actions"]
    assert w.graph(CUTS_FROM_RESET, True, "noised").fused
    assert a.flatten().unique().numel() == n * STEPS * w.A


# ---------------------------------------------------------------------------
# 5. episode returns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "multi"])
def test_episode_returns_are_the_segment_sums(monkeypatch, fused):
    n = 37
    _, snaps = _two_epochs(monkeypatch, fused, n, "bench_narrow", "noised")
    for snap, cuts in zip(snaps, (CUTS_FROM_RESET, CUTS_CARRY)):
        rew = _rows(snap, n)["rewards"].double().cpu().numpy()
        ends = [c + 1 for c in cuts]
        bounds = list(zip([0] + ends, ends + ([STEPS] if ends[-1] < STEPS else [])))
        seg = snap["seg_returns"].cpu().numpy()
        assert seg.shape == (n, len(bounds))
        for j, (s, e) in enumerate(bounds):
            want = rew[:, s:e].sum(axis=1)
            tol = 2 * (e - s) * 2.0 ** -24 * np.abs(rew[:, s:e]).sum(axis=1)
            assert (np.abs(seg[:, j] - want) <= tol).all(), (j, s, e)
        assert snap["exp"].episode_returns == [float(x) for x in seg.reshape(-1)]


# ---------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------
def test_identically_seeded_runs_are_bit_equal(monkeypatch):
    n = 37
    runs = [_two_epochs(monkeypatch, True, n, "bench_wide", "noised")[1] for _ in range(2)]
    other = _two_epochs(monkeypatch, True, n, "bench_wide", "noised", seed=6)[1]
    for e in range(2):
        a, b = runs[0][e], runs[1][e]
        assert a["ctr"] == b["ctr"]
        for k in RING:
            assert torch.equal(a["ring"][k], b["ring"][k])
        assert torch.equal(a["state"], b["state"])
        assert a["exp"].episode_returns == b["exp"].episode_returns
        assert not torch.equal(a["ring"]["observations"], other[e]["ring"]["observations"])


def test_weights_are_read_by_pointer(monkeypatch):
    """The net changed in place between replays of ONE graph: the next
    epoch's actions follow it (noise 0)."""
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    n = 16
    for net in ("bench_narrow", "bench_wide"):
        w = World(n, net, noise=0.0, horizon=None)
        w.epoch("noised")
        before = w.epoch("noised")
        with torch.no_grad():
            for p in w.net.parameters():
                p.zero_()
            list(w.net.parameters())[-1].fill_(0.5)
        after = w.epoch("noised")
        assert len(w.sampler._graphs) == 2 and not after["new_keys"]
        assert w.graph((), False, "noised").fused
        a0 = _rows(before, n)["actions"]
        a1 = _rows(after, n)["actions"]
        assert (a0 - math.tanh(0.5)).abs().max() > 1e-3
        assert (a1 - math.tanh(0.5)).abs().max() < 1e-6


# ---------------------------------------------------------------------------
# 7. gate
# ---------------------------------------------------------------------------
def _noised(dims, env, dtype=None):
    from rl_replicas_amd.utils import add_noise_to_get_action

    _, det = _actor(dims, dtype)
    return add_noise_to_get_action(det, env.action_space, 0.1)


def test_gate(monkeypatch):
    """`synthetic_collect_fused_eligible` is false in each case, and sample()
    still fills the ring: through the captured multi-kernel body where the
    collect path applies, through DeviceSampler's eager loop and
    add_experience where it does not.  Three cases have no route at all: no
    code path feeds an [N, O] fp32 observation to a net whose input is not O
    wide or whose weights are fp64, and a head that is not A wide cannot act
    on the env, so for them only the gate is checked."""
    from rl_replicas_amd import ops
    from rl_replicas_amd.envs import DeviceVectorEnv
    from rl_replicas_amd.envs.spaces import Box
    from rl_replicas_amd.ops import fused_rollout
    from rl_replicas_amd.policies import RandomPolicy
    from rl_replicas_amd.replay_buffer import ReplayBuffer

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    ext = ops._load_extension()
    max_layers, max_width, max_cuts, max_lds = ext.synthetic_collect_fused_limits()
    lds = ext.synthetic_collect_fused_lds_bytes
    # the worked example: five [16][260] tiles + the Ant env image, ~87 KB
    assert lds(NETS["bench_wide"][1], 27, 8) == 4 * (5 * 16 * 260 + 27 * 27 + 8 * 27 + 27)
    assert lds(NETS["bench_wide"][1], 27, 8) <= max_lds
    assert lds([27, 64, 64, 64, 64, 8], 27, 8) > lds(NETS["bench_narrow"][1], 27, 8)
    assert lds([], 27, 8) == 4 * (5 * 16 * 68 + 27 * 27 + 8 * 27 + 27)
    n = 16
    few = (3,)

    def filled(w, mode="noised", steps=STEPS, route="graph"):
        snap = w.epoch(mode, steps)
        assert snap["len"] == snap["size_dev"] == n * steps
        assert torch.isfinite(snap["ring"]["rewards"][: n * steps]).all()
        assert (snap["ring"]["rewards"][: n * steps] != SENTINEL).all()
        if route == "graph":
            (g,) = w.sampler._graphs.values()
            assert not g.fused and snap["exp"].stored_in_buffer is w.buf
        else:
            assert not w.sampler._graphs
            assert getattr(snap["exp"], "stored_in_buffer", None) is None

    w = World(n, "bench_wide")
    pol, uni = w.policies["noised"], w.policies["uniform"]
    assert fused_rollout.synthetic_collect_supported(pol, w.env, w.buf)
    assert fused_rollout.synthetic_collect_supported(uni, w.env, w.buf)
    assert fused_rollout.synthetic_collect_fused_eligible(pol, w.env, few)
    assert fused_rollout.synthetic_collect_fused_eligible(uni, w.env, few)
    # unset: the measured default decides
    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED")
    assert (fused_rollout.synthetic_collect_fused_eligible(pol, w.env, few)
            == fused_rollout.synthetic_collect_fused_default())

    # RL_REPLICAS_AMD_ROLLOUT_FUSED=0: the multi-kernel body
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "0")
    assert not fused_rollout.synthetic_collect_fused_eligible(pol, w.env, few)
    assert not fused_rollout.synthetic_collect_fused_eligible(uni, w.env, few)
    filled(w)
    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")

    # bf16 compute: the multi-kernel body
    monkeypatch.setenv("RL_REPLICAS_AMD_COMPUTE_DTYPE", "bf16")
    w = World(n, "bench_narrow")
    assert not fused_rollout.synthetic_collect_fused_eligible(w.policies["noised"], w.env, few)
    filled(w)
    monkeypatch.delenv("RL_REPLICAS_AMD_COMPUTE_DTYPE")

    # one layer / one column too many for the kernels: DeviceSampler's loop
    for dims in ([5] + [8] * max_layers + [3], [5, max_width + 1, 3]):
        w = World(n, (AWKWARD_ID, dims))
        pol = w.policies["noised"]
        assert not fused_rollout.synthetic_collect_fused_eligible(pol, w.env, few)
        assert not fused_rollout.synthetic_collect_supported(pol, w.env, w.buf)
        filled(w, route="eager")

    # one cut too many for the by-value list: the multi-kernel body
    steps = max_cuts + 1
    w = World(n, "bench_narrow", horizon=1)
    many = tuple(range(steps))
    assert fused_rollout.synthetic_collect_fused_eligible(w.policies["noised"], w.env, many[:-1])
    assert not fused_rollout.synthetic_collect_fused_eligible(w.policies["noised"], w.env, many)
    assert not fused_rollout.synthetic_collect_fused_eligible(w.policies["uniform"], w.env, many)
    filled(w, steps=steps)
    assert w.graph(many, True, "noised", steps).n_segs == steps
    assert (w.buf._storage["dones"][: n * steps] == 1.0).all()

    # an input that is not O wide, a head that is not A wide, an fp64 weight:
    # the gate only (docstring)
    w = World(n)
    for pol in (_noised([6, 16, 3], w.env), _noised([5, 16, 4], w.env),
                _noised([5, 16, 3], w.env, torch.float64)):
        assert not fused_rollout.synthetic_collect_fused_eligible(pol, w.env, few)
        assert not fused_rollout.synthetic_collect_supported(pol, w.env, w.buf)

    # an LDS need over the budget: declined by the fused gate alone
    _register()
    wide_env = DeviceVectorEnv(OVER_ID, n, device=DEVICE)
    big = _noised([64, 256, 12], wide_env)
    assert lds([64, 256, 12], 64, 12) > max_lds >= lds([64, 256, 2], 64, 2)
    assert fused_rollout.synthetic_collect_supported(big, wide_env, w.buf)
    assert not fused_rollout.synthetic_collect_fused_eligible(big, wide_env, few)
    assert fused_rollout.synthetic_collect_fused_eligible(
        _noised([64, 8, 12], wide_env), wide_env, few)

    # a bare DeterministicPolicy, a RandomPolicy over unequal bounds: the loop
    pol = w.policies["noised"]
    w2 = World(n)
    assert not fused_rollout.synthetic_collect_supported(w2.det, w2.env, w2.buf)
    filled(w2, mode=w2.det, route="eager")
    w2 = World(n)
    lopsided = RandomPolicy(Box(np.array([-1.0, -1.0, -0.5], dtype=np.float32),
                                np.array([1.0, 1.0, 1.0], dtype=np.float32)))
    assert not fused_rollout.synthetic_collect_supported(lopsided, w2.env, w2.buf)
    assert not fused_rollout.synthetic_collect_fused_eligible(lopsided, w2.env, few)
    filled(w2, mode=lopsided, route="eager")
    narrower = RandomPolicy(Box(-0.5, 0.5, shape=(3,), dtype=np.float32))
    assert not fused_rollout.synthetic_collect_supported(narrower, w2.env, w2.buf)

    # a CPU env
    w2 = World(n, env_device="cpu")
    assert not fused_rollout.synthetic_collect_supported(w2.policies["uniform"], w2.env, w2.buf)
    snap_exp = w2.sampler.sample(n * STEPS, w2.policies["uniform"])
    w2.buf.add_experience(snap_exp)
    assert not w2.sampler._graphs and len(w2.buf) == n * STEPS
    assert (w2.buf._storage["rewards"][: n * STEPS] != SENTINEL).all()

    # a CPU buffer: the sampler refuses to pair one with a GPU env, so the
    # sampler's buffer is swapped after construction
    w2 = World(n)
    cpu_buf = ReplayBuffer(256)
    assert not fused_rollout.synthetic_collect_supported(pol, w.env, cpu_buf)
    w2.sampler.replay_buffer = w2.buf = cpu_buf
    exp = w2.sampler.sample(n * STEPS, w2.policies["noised"])
    cpu_buf.add_experience(exp)
    assert not w2.sampler._graphs and len(cpu_buf) == n * STEPS
    assert getattr(exp, "stored_in_buffer", None) is None
    assert torch.isfinite(cpu_buf._storage["rewards"][: n * STEPS]).all()

    # graphs disabled
    monkeypatch.setenv("RL_REPLICAS_AMD_DISABLE_GRAPHS", "1")
    w2 = World(n)
    assert not fused_rollout.synthetic_collect_supported(w2.policies["noised"], w2.env, w2.buf)
    filled(w2, route="eager")


# ---------------------------------------------------------------------------
# 8. binding argument checks
# ---------------------------------------------------------------------------
def test_bindings_check_arguments_before_launching():
    from rl_replicas_amd import ops
    from rl_replicas_amd.ops.fused_mlp import _extract_layers

    ext = ops._load_extension()
    n, steps, cap, O, A = 5, 6, 64, 5, 3
    net, _ = _actor(NETS["awkward"][1])
    weights, biases, acts = _extract_layers(net)
    weights, biases = list(weights), list(biases)

    def fresh(cap=cap):
        torch.manual_seed(0)
        return {
            "carry": torch.zeros(n, O, device=DEVICE),
            "ctr": torch.full((1,), CTR_BASE, dtype=torch.int64, device=DEVICE),
            "env": [torch.randn(O, O, device=DEVICE) * 0.3,
                    torch.randn(A, O, device=DEVICE), torch.randn(O, device=DEVICE)],
            "storage": [torch.full((cap, O), SENTINEL, device=DEVICE),
                        torch.full((cap, A), SENTINEL, device=DEVICE),
                        torch.full((cap,), SENTINEL, device=DEVICE),
                        torch.full((cap, O), SENTINEL, device=DEVICE),
                        torch.full((cap,), SENTINEL, device=DEVICE)],
            "write_dev": torch.zeros(1, dtype=torch.int64, device=DEVICE),
            "size_dev": torch.zeros(1, dtype=torch.int64, device=DEVICE),
            "seg_returns": torch.zeros(n, 2, device=DEVICE),
        }

    def fused(a, cuts=(3,), w=None, b=None, mode=0, steps=steps, wg=256, reset=True,
              net_in_uniform=False):
        w = weights if w is None else w
        b = biases if b is None else b
        use_net = mode == 0 or net_in_uniform
        ext.synthetic_collect_fused(
            w if use_net else [], b if use_net else [], acts[: len(w)] if use_net else [],
            mode, 0.1, 1.0, -1.0, 1.0, 11, 12, a["env"][0], a["env"][1], a["env"][2],
            0.05, list(cuts), reset, a["ctr"], a["carry"], steps, a["storage"],
            a["write_dev"], a["size_dev"], a["seg_returns"], wg)

    def scatter(a, obs_full=None):
        ext.replay_scatter(
            obs_full if obs_full is not None else torch.zeros(steps + 1, n, O, device=DEVICE),
            torch.zeros(steps, n, A, device=DEVICE), torch.zeros(steps, n, device=DEVICE),
            torch.zeros(1, n, O, device=DEVICE),
            torch.full((steps,), -1, dtype=torch.int32, device=DEVICE), 0,
            a["storage"], a["write_dev"], a["size_dev"], torch.zeros(n, 1, device=DEVICE))

    def untouched(a):
        torch.cuda.synchronize()
        return (all((t == SENTINEL).all() for t in a["storage"])
                and (a["carry"] == 0).all() and int(a["write_dev"]) == 0)

    bad = []
    a = fresh(); a["storage"][2] = a["storage"][2].double(); bad.append(a)   # dtype
    a = fresh(); a["storage"][0] = a["storage"][0].cpu(); bad.append(a)      # device
    a = fresh(); a["write_dev"] = a["write_dev"].cpu(); bad.append(a)        # device
    a = fresh(); a["size_dev"] = a["size_dev"].int(); bad.append(a)          # dtype
    a = fresh()                                                              # layout
    a["storage"][3] = torch.full((cap, 2 * O), SENTINEL, device=DEVICE)[:, ::2]
    assert not a["storage"][3].is_contiguous()
    bad.append(a)
    a = fresh(); a["storage"][1] = a["storage"][1][: cap - 1].contiguous(); bad.append(a)
    a = fresh()                                                # an actions ring of A - 1
    a["storage"][1] = torch.full((cap, A - 1), SENTINEL, device=DEVICE); bad.append(a)
    a = fresh()                                           # an observations ring of O + 1
    a["storage"][0] = torch.full((cap, O + 1), SENTINEL, device=DEVICE); bad.append(a)
    bad.append(fresh(cap=n * steps - 1))                                     # N*steps > cap
    for a in bad:
        for call in (fused, scatter):
            with pytest.raises(RuntimeError):
                call(a)
        with pytest.raises(RuntimeError):
            fused(a, mode=1)
        assert untouched(a)
    a = fresh()
    for cuts in ((3, 1), (2, 2), (6,), (-1,)):  # unsorted, repeated, out of range
        with pytest.raises(RuntimeError):
            fused(a, cuts=cuts)
    with pytest.raises(RuntimeError):  # the head must be A wide
        fused(a, w=[weights[0]], b=[biases[0]])
    with pytest.raises(RuntimeError):  # the input must be O wide
        fused(a, w=[torch.zeros(A, O + 1, device=DEVICE)], b=[torch.zeros(A, device=DEVICE)])
    with pytest.raises(RuntimeError):  # seg_returns sized for two segments
        fused(a, cuts=())
    with pytest.raises(RuntimeError):  # uniform mode takes no net
        fused(a, mode=1, net_in_uniform=True)
    with pytest.raises(RuntimeError):  # a workgroup size the kernel is not built for
        fused(a, wg=512)
    with pytest.raises(RuntimeError):  # an unknown mode
        fused(a, mode=2)
    # env matrices of the wrong shape, dtype or device
    for i, t in ((0, torch.zeros(O, O + 1, device=DEVICE)),
                 (0, torch.zeros(O + 1, O + 1, device=DEVICE)),
                 (1, torch.zeros(A, O + 1, device=DEVICE)),
                 (1, torch.zeros(A * O, device=DEVICE)),
                 (2, torch.zeros(O + 1, device=DEVICE)),
                 (2, torch.zeros(O, dtype=torch.float64, device=DEVICE)),
                 (0, torch.zeros(O, O))):
        b = fresh()
        b["env"][i] = t
        with pytest.raises(RuntimeError):
            fused(b)
        with pytest.raises(RuntimeError):
            fused(b, mode=1)
        assert untouched(b)
    b = fresh()  # B [A + 1, O]: the action dim no longer matches the ring and the head
    b["env"][1] = torch.zeros(A + 1, O, device=DEVICE)
    with pytest.raises(RuntimeError):
        fused(b)
    b = fresh(); b["carry"] = torch.zeros(n, O, dtype=torch.float64, device=DEVICE)
    with pytest.raises(RuntimeError):
        fused(b)
    b = fresh(); b["carry"] = torch.zeros(n, 2 * O, device=DEVICE)[:, ::2]
    with pytest.raises(RuntimeError):
        fused(b)
    b = fresh(); b["seg_returns"] = torch.zeros(n, 2)
    with pytest.raises(RuntimeError):
        fused(b)
    with pytest.raises(RuntimeError):
        ext.synthetic_collect_fused_lds_bytes([65, 8, 2], 65, 2)
    with pytest.raises(RuntimeError):
        scatter(a, obs_full=torch.zeros(steps + 1, n, O + 1, device=DEVICE))
    assert untouched(a)

    # a write scalar outside the ring is reduced, never used as it stands
    for mode in (0, 1):
        a = fresh()
        a["write_dev"].fill_(cap * 1000 + 7)
        a["size_dev"].fill_(cap - 3)
        fused(a, mode=mode)
        ext.ring_advance_(a["write_dev"], a["size_dev"], n * steps, cap)
        torch.cuda.synchronize()
        assert int(a["write_dev"]) == (7 + n * steps) % cap and int(a["size_dev"]) == cap
        want = sorted((7 + np.arange(n * steps)) % cap)
        for t in a["storage"]:
            flat = t.reshape(cap, -1)
            written = (flat != SENTINEL).all(dim=1).nonzero().flatten().cpu().tolist()
            partly = (flat != SENTINEL).any(dim=1).nonzero().flatten().cpu().tolist()
            assert written == partly == want


# ---------------------------------------------------------------------------
# 9. mixing device collects, host adds and eager epochs
# ---------------------------------------------------------------------------
def test_device_collects_host_adds_and_eager_epochs_mix(monkeypatch):
    from rl_replicas_amd.experience import Experience

    monkeypatch.setenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", "1")
    n, ne, host_n = 5, 5 * STEPS, 4
    w = World(n, cap=4096, horizon=None)
    O, A = w.O, w.A
    first = w.epoch("uniform")
    assert first["new_keys"] == {(STEPS, (), True, "uniform")}
    host = Experience(
        observations=[[np.full(O, 100.0 + i, dtype=np.float32) for i in range(host_n)]],
        actions=[[np.full(A, 0.5, dtype=np.float32)] * host_n],
        rewards=[[-1.0] * host_n],
        last_observations=[np.full(O, 200.0, dtype=np.float32)],
        dones=[[False] * (host_n - 1) + [True]],
        episode_returns=[-4.0], episode_lengths=[host_n],
    )
    w.buf.add_experience(host)
    assert w.buf._write == ne + host_n and int(w.buf._write_dev.item()) == ne + host_n
    second = w.epoch("uniform")
    assert second["new_keys"] == {(STEPS, (), False, "uniform")}
    assert second["write_before"] == ne + host_n
    # an eager DeviceSampler-route epoch in between: graphs disabled
    monkeypatch.setenv("RL_REPLICAS_AMD_DISABLE_GRAPHS", "1")
    third = w.epoch("uniform")
    monkeypatch.delenv("RL_REPLICAS_AMD_DISABLE_GRAPHS")
    assert not third["new_keys"]
    assert getattr(third["exp"], "stored_in_buffer", None) is None
    fourth = w.epoch("uniform")
    assert not fourth["new_keys"] and fourth["exp"].stored_in_buffer is w.buf
    total = 4 * ne + host_n
    assert fourth["write"] == fourth["write_dev"] == total
    assert fourth["len"] == fourth["size_dev"] == total
    ring = fourth["ring"]
    # nothing lost: epoch, host rows, epoch, eager epoch, epoch, in a row
    for k in RING:
        assert torch.equal(ring[k][:ne], first["ring"][k][:ne]), k
        assert torch.equal(ring[k][: 3 * ne + host_n], third["ring"][k][: 3 * ne + host_n]), k
        assert (ring[k][:total] != SENTINEL).all(), k
        assert (ring[k][total:] == SENTINEL).all(), k
    assert ring["observations"][ne : ne + host_n, 0].tolist() == [100.0, 101.0, 102.0, 103.0]
    assert ring["dones"][ne : ne + host_n].tolist() == [0.0, 0.0, 0.0, 1.0]
    # every epoch continues from the live state: there is no cut, so each
    # epoch's first observation is the successor the one before it stored
    starts = [0, ne + host_n, 2 * ne + host_n, 3 * ne + host_n]
    obs = [ring["observations"][s : s + ne].view(n, STEPS, O) for s in starts]
    nxt = [ring["next_observations"][s : s + ne].view(n, STEPS, O) for s in starts]
    for e in range(1, 4):
        assert torch.equal(obs[e][:, 0], nxt[e - 1][:, STEPS - 1]), e
    assert torch.equal(fourth["state"], nxt[3][:, STEPS - 1])
    assert w.env._elapsed == 4 * STEPS

    # the fused gather draws below the new size only
    mb = w.buf.gather_minibatch_fused(4096, seed=9, offset=0)
    torch.cuda.synchronize()
    assert (mb["rewards"] != SENTINEL).all() and (mb["observations"] != SENTINEL).all()
    assert mb["observations"].shape == (4096, O) and mb["actions"].shape == (4096, A)
    stored = set(ring["rewards"][:total].tolist())
    assert set(mb["rewards"].tolist()) <= stored
    assert len(set(mb["rewards"].tolist())) > ne  # reaches past the first epoch


# ---------------------------------------------------------------------------
# 10. end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_off_policy_end_to_end(tmp_path, monkeypatch, algo):
    from rl_replicas_amd import ops
    from rl_replicas_amd.algorithms import DDPG, TD3
    from rl_replicas_amd.envs import DeviceVectorEnv
    from rl_replicas_amd.evaluator import Evaluator
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.policies import RandomPolicy
    from rl_replicas_amd.q_function import QFunction
    from rl_replicas_amd.replay_buffer import ReplayBuffer
    from rl_replicas_amd.samplers import DeviceReplaySampler

    monkeypatch.delenv("RL_REPLICAS_AMD_ROLLOUT_FUSED", raising=False)
    torch.manual_seed(0)
    env = DeviceVectorEnv("Hopper-v4", 10, device=DEVICE)
    pnet, policy = _actor([11, 32, 3])
    qnets = [MLP([14, 32, 1], activation_function=nn.ReLU).to(DEVICE)
             for _ in range(2 if algo == "td3" else 1)]
    qs = [QFunction(q, ops.make_adam(q.parameters(), lr=1e-3)) for q in qnets]
    buf = ReplayBuffer(1024, device=DEVICE)
    sampler = DeviceReplaySampler(env, buf, seed=3)
    cls = TD3 if algo == "td3" else DDPG
    model = cls(policy, RandomPolicy(env.action_space), *qs, env, sampler, buf,
                Evaluator(seed=4))
    model.learn(num_epochs=3, batch_size=50, minibatch_size=16, num_start_steps=50,
                num_steps_before_update=50, num_train_steps=2,
                num_evaluation_episodes=0, output_dir=str(tmp_path))
    torch.cuda.synchronize()
    assert set(sampler._graphs) == {(5, (), True, "uniform"), (5, (), False, "noised")}
    assert model.current_total_steps == 150
    assert len(buf) == 150 and buf._write == 150
    assert int(buf._write_dev.item()) == 150 and int(buf._size_dev.item()) == 150
    assert env._elapsed == 15
    assert buf._storage["observations"].shape == (1024, 11)
    assert buf._storage["actions"].shape == (1024, 3)
    for k in RING:
        assert torch.isfinite(buf._storage[k][:150]).all(), k
    for p in list(pnet.parameters()) + [p for q in qnets for p in q.parameters()]:
        assert torch.isfinite(p).all()
