"""The host layer of the fused-MLP kernels (gpu-marked): which kernel a net
is sent to, what the bindings refuse, and that Python's gates are the
extension's own.

Shapes are the smallest that sit on each side of a gate.  With 32-row
backward tiles of stride 68 and a 100 KiB budget (25600 floats) the
whole-net backward holds a weight image of 25600 - 3*2176 = 19072 floats,
and with the forward in the kernel 25600 - (3 + L)*2176; a layer's image is
out * (in + 1) floats.  Batch 33 is two row blocks with a 1-row tail."""
import types

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BATCH = 33
HP = (1e-3, 0.9, 0.999, 1e-8, 0.0)  # lr, beta1, beta2, eps, weight_decay


@pytest.fixture(scope="module")
def ext():
    from rl_replicas_amd import ops

    assert ops.hip_available()
    return ops._load_extension()


def image_floats(dims):
    return sum(o * (i + 1) for i, o in zip(dims[:-1], dims[1:]))


# ---------------------------------------------------------------------------
# 1. per-layer narrow backward and its whole-net neighbour
# ---------------------------------------------------------------------------
PER_LAYER = [64, 64, 64, 64, 64, 64]  # image 20800 > 19072: one kernel per layer
WHOLE_NET = [64, 64, 64, 64, 64, 37]  # image 19045 <= 19072: whole-net kernel


def test_pair_sits_on_both_sides_of_the_backward_gate(ext):
    assert image_floats(PER_LAYER) == 20800 and image_floats(WHOLE_NET) == 19045
    assert not ext.fused_bwd_fits(PER_LAYER)[0]
    assert ext.fused_bwd_fits(WHOLE_NET)[0]


@pytest.mark.parametrize("sizes", [PER_LAYER, WHOLE_NET], ids=["per_layer", "whole_net"])
def test_five_layer_narrow_grads_match_autograd(ext, sizes):
    from rl_replicas_amd.networks import MLP

    torch.manual_seed(0)
    mlp_f = MLP(sizes).to("cuda")
    mlp_e = MLP(sizes).to("cuda")
    mlp_e.load_state_dict(mlp_f.state_dict())
    x0 = torch.randn(BATCH, sizes[0], device="cuda")
    grad_out = torch.randn(BATCH, sizes[-1], device="cuda")

    def fused_run():
        mlp_f.zero_grad()
        x = x0.clone().requires_grad_(True)
        out = mlp_f(x)  # fused training path
        out.backward(grad_out)
        return [out.detach(), x.grad] + [p.grad.clone() for p in mlp_f.parameters()]

    first, second = fused_run(), fused_run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)

    xe = x0.clone().requires_grad_(True)
    out_e = mlp_e.network(xe)  # eager autograd oracle
    out_e.backward(grad_out)
    torch.testing.assert_close(first[0], out_e, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(first[1], xe.grad, rtol=5e-4, atol=5e-5)
    for got, (name, p_e) in zip(first[2:], mlp_e.named_parameters()):
        torch.testing.assert_close(got, p_e.grad, rtol=5e-4, atol=5e-5,
                                   msg=lambda m: f"{name}: {m}")


# ---------------------------------------------------------------------------
# 2. gate parity: the answers of the hand-mirrored gates, recorded before
#    they were rewritten on top of the extension's query
# ---------------------------------------------------------------------------
# value net dims -> (value_mode, _fwd_in_kernel_fits); fits None = not
# compared (_fwd_in_kernel_fits is only ever asked about narrow nets)
VALUE_TABLE = [
    ([64, 64, 64, 31, 1], "narrow", True),    # image 10367: one float to spare
    ([64, 64, 64, 32, 1], "narrow", False),   # image 10433
    ([17, 64, 32, 1], "narrow", True),
    ([17, 256, 256, 1], "wide", False),
    ([64, 64, 64, 64, 64, 1], "narrow", False),
    ([17, 64, 32, 2], None, True),            # not a 1-output head
    ([65, 64, 1], "wide", None),              # input wider than 64
]
# policy net dims -> _mega_eligible
POLICY_TABLE = [
    ([17, 64, 32, 6], True),
    ([64, 64, 64, 31, 6], False),
    ([64, 64, 64, 32, 6], False),
    ([17, 64, 64, 64, 64, 6], False),  # five layers: no slot left for log_std
    ([17, 256, 256, 6], False),
    ([65, 64, 6], False),
    ([64, 64, 64, 30, 64], False),
]


def value_holder(dims, adam):
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.value_function import ValueFunction

    net = MLP(dims).to("cuda")
    holder = types.SimpleNamespace(
        value_function=ValueFunction(net, adam(net.parameters(), lr=1e-3)),
        _all_reduce_gradients=lambda module: None,
    )
    return holder, net


def test_gates_answer_as_recorded(ext):
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.ops import fused_onpolicy as fop
    from rl_replicas_amd.ops.fused_mlp import _extract_layers
    from rl_replicas_amd.policies import GaussianPolicy

    assert image_floats(VALUE_TABLE[0][0]) == 10367
    assert image_floats(VALUE_TABLE[1][0]) == 10433
    for dims, mode, fits in VALUE_TABLE:
        holder, net = value_holder(dims, torch.optim.Adam)
        obs = torch.zeros(BATCH, dims[0], device="cuda")
        assert fop.value_mode(holder, obs) == mode, dims
        if fits is not None:
            assert fop._fwd_in_kernel_fits(_extract_layers(net)[0]) == fits, dims
    for dims, mega in POLICY_TABLE:
        net = MLP(dims).to("cuda")
        log_std = nn.Parameter(torch.zeros(dims[-1], device="cuda"))
        policy = GaussianPolicy(net, None, log_std)
        obs = torch.zeros(BATCH, dims[0], device="cuda")
        assert fop._mega_eligible(policy, "gaussian", obs) == mega, dims


@pytest.mark.parametrize("dims", [[64, 64, 64, 31, 1], [64, 64, 64, 32, 1]],
                         ids=["fwd_in_kernel", "separate_fwd"])
def test_graphed_value_update_agrees_with_its_binding(ext, monkeypatch, dims):
    """On either side of the in-kernel-forward boundary the captured loop
    picks a form the binding accepts, and gives what the ungraphed loop
    gives."""
    from rl_replicas_amd import ops
    from rl_replicas_amd.ops import fused_onpolicy as fop

    g = torch.Generator().manual_seed(5)
    obs = torch.randn(BATCH, dims[0], generator=g).cuda()
    returns = torch.randn(BATCH, generator=g).cuda()
    results = []
    for graphs in (True, False):
        if graphs:
            monkeypatch.delenv("RL_REPLICAS_AMD_DISABLE_GRAPHS", raising=False)
        else:
            monkeypatch.setenv("RL_REPLICAS_AMD_DISABLE_GRAPHS", "1")
        torch.manual_seed(7)
        holder, net = value_holder(dims, ops.make_adam)
        loss = fop.value_update(holder, obs, returns, 2)
        torch.cuda.synchronize()
        assert hasattr(holder, "_value_graph") == graphs
        results.append((loss, [p.detach().clone() for p in net.parameters()]))
    (loss_g, params_g), (loss_e, params_e) = results
    print("value loss graphed/ungraphed:", loss_g, loss_e)
    for a, b in zip(params_g, params_e):
        assert torch.equal(a, b)
    assert loss_g == loss_e


# ---------------------------------------------------------------------------
# 3. validation: every bad net is refused before anything is launched
# ---------------------------------------------------------------------------
def make_net(dims, seed):
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(o, i, generator=g) / float(i) ** 0.5).cuda()
          for i, o in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * torch.randn(o, generator=g)).cuda() for o in dims[1:]]
    return {"dims": dims, "w": ws, "b": bs, "acts": [1] * (len(dims) - 2) + [0],
            "hidden": [torch.zeros(BATCH, d, device="cuda") for d in dims[1:-1]],
            "out": torch.zeros(BATCH, dims[-1], device="cuda")}


def six_layers(net):
    d = net["dims"]
    return make_net([d[0]] + [8] * 5 + [d[-1]], 11)


def broken_chain(net):
    w = net["w"][1]
    net["w"][1] = torch.zeros(w.shape[0], w.shape[1] + 1, device="cuda")
    return net


def transposed(net):
    net["w"][1] = net["w"][1].t().contiguous().t()
    assert not net["w"][1].is_contiguous()
    return net


def short_bias(net):
    net["b"][1] = net["b"][1][:-1].contiguous()
    return net


def wrong_hidden(net):
    net["hidden"] = net["hidden"][:-1]
    return net


def fp64_weight(net):
    net["w"][1] = net["w"][1].double()
    return net


BAD_NETS = [six_layers, broken_chain, transposed, short_bias, fp64_weight]


def adam_state(net):
    """(m, v, step) shaped like the net as it was before it was broken."""
    ps = net["w"] + net["b"]
    return ([torch.full_like(p, 0.25, dtype=torch.float32) for p in ps],
            [torch.full_like(p, 0.5, dtype=torch.float32) for p in ps],
            torch.ones((), device="cuda"))


def policy_iter_args(pol, m, v, step, extra):
    return (extra["obs"], list(pol["w"]), list(pol["b"]), pol["acts"],
            extra["actions"], extra["old_logp"], extra["adv"], extra["log_std"],
            0.2, m, v, extra["ls_m"], extra["ls_v"], step, *HP, 0.0,
            extra["gate"], extra["kl_final"], extra["iters_done"], 1e9,
            extra["loss_out"], True)


def policy_extra(d_in, d_out):
    g = torch.Generator().manual_seed(3)
    return {
        "obs": torch.randn(BATCH, d_in, generator=g).cuda(),
        "actions": torch.randn(BATCH, d_out, generator=g).cuda(),
        "old_logp": torch.randn(BATCH, generator=g).cuda(),
        "adv": torch.randn(BATCH, generator=g).cuda(),
        "log_std": torch.full((d_out,), -0.5, device="cuda"),
        "ls_m": torch.full((d_out,), 0.25, device="cuda"),
        "ls_v": torch.full((d_out,), 0.5, device="cuda"),
        "gate": torch.ones(1, device="cuda"),
        "kl_final": torch.full((1,), 3.0, device="cuda"),
        "iters_done": torch.full((1,), 4.0, device="cuda"),
        "loss_out": torch.full((1,), 5.0, device="cuda"),
        "returns": torch.randn(BATCH, generator=g).cuda(),
        "partials": torch.full((2,), 6.0, device="cuda"),
    }


def call_mlp_backward(ext, net, extra):
    m, v, step = extra["adam"]
    grad_out = torch.ones(BATCH, net["dims"][-1], device="cuda")
    ext.mlp_backward(grad_out, extra["obs"], list(net["w"]), list(net["b"]),
                     list(net["hidden"]), net["out"], net["acts"], 0, m, v, step,
                     *HP, 0.0)


def call_value_mlp_backward(ext, net, extra):
    m, v, step = extra["adam"]
    ext.value_mlp_backward(extra["obs"], list(net["w"]), list(net["b"]),
                           list(net["hidden"]), net["out"], net["acts"],
                           extra["returns"], 0, extra["partials"], m, v, step,
                           *HP, 0.0)


def call_policy_iter(ext, net, extra):
    ext.gaussian_ppo_policy_iter(*policy_iter_args(net, *extra["adam"], extra))


def call_twin_iter(ext, net, extra):
    """The policy half is sound; `net` is the value half."""
    pol = extra["good_policy"]
    m, v, step = extra["adam"]
    ext.gaussian_ppo_value_twin_iter(
        *policy_iter_args(pol, *extra["policy_adam"], extra), extra["obs"],
        list(net["w"]), list(net["b"]), net["acts"], extra["returns"],
        extra["partials"], m, v, step, *HP, 0.0)


# binding -> (caller, head width of the net it takes, whether it reads hidden)
BINDINGS = {
    "mlp_backward": (call_mlp_backward, 3, True),
    "value_mlp_backward": (call_value_mlp_backward, 1, True),
    "gaussian_ppo_policy_iter": (call_policy_iter, 3, False),
    "gaussian_ppo_value_twin_iter": (call_twin_iter, 1, False),
}
CASES = [(name, bad) for name, (_, _, reads_hidden) in BINDINGS.items()
         for bad in BAD_NETS + ([wrong_hidden] if reads_hidden else [])]


def tensors_of(obj):
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, dict):
        obj = list(obj.values())
    if isinstance(obj, (list, tuple)):
        return [t for o in obj for t in tensors_of(o)]
    return []


@pytest.mark.parametrize("name,bad", CASES,
                         ids=[f"{n}-{b.__name__}" for n, b in CASES])
def test_bad_net_is_refused_before_any_launch(ext, name, bad):
    call, head, _ = BINDINGS[name]
    dims = [5, 8, 4, head]
    extra = policy_extra(5, 3)
    extra["good_policy"] = make_net([5, 8, 4, 3], 1)
    extra["policy_adam"] = adam_state(extra["good_policy"])
    good = make_net(dims, 2)
    call(ext, good, dict(extra, adam=adam_state(good)))  # the sound call runs
    torch.cuda.synchronize()

    net = bad(make_net(dims, 2))
    extra["adam"] = adam_state(make_net(net["dims"], 2))
    watched = tensors_of(net) + tensors_of(extra)
    before = [t.clone() for t in watched]
    with pytest.raises(RuntimeError):
        call(ext, net, extra)
    torch.cuda.synchronize()
    for t, t0 in zip(watched, before):
        assert torch.equal(t, t0)


# ---------------------------------------------------------------------------
# 4. depth: the caps are the extension's, and a deeper net runs eager
# ---------------------------------------------------------------------------
def test_python_caps_equal_the_extensions(ext):
    from rl_replicas_amd.ops import fused_mlp

    max_layers, max_width, narrow_width, gauss_max_d = ext.fused_mlp_limits()
    assert (fused_mlp.MAX_LAYERS, fused_mlp.MAX_WIDTH) == (max_layers, max_width)
    assert (max_layers, max_width, narrow_width, gauss_max_d) == (5, 256, 64, 512)


def test_six_layer_net_falls_back_to_eager(ext):
    from rl_replicas_amd.networks import MLP
    from rl_replicas_amd.ops import fused_onpolicy as fop
    from rl_replicas_amd.ops.fused_mlp import try_fused_forward
    from rl_replicas_amd.policies import GaussianPolicy

    torch.manual_seed(0)
    mlp = MLP([8, 16, 16, 16, 16, 16, 2]).to("cuda")
    x = torch.randn(BATCH, 8, device="cuda")
    with torch.no_grad():
        assert try_fused_forward(mlp, x) is NotImplemented
        assert torch.equal(mlp(x), mlp.network(x))

    log_std = nn.Parameter(torch.zeros(2, device="cuda"))
    assert not fop.supported(GaussianPolicy(mlp, None, log_std), x)
    holder, _ = value_holder([8, 16, 16, 16, 16, 16, 1], torch.optim.Adam)
    assert fop.value_mode(holder, x) is None
    assert not fop.value_supported(holder, x)
