"""The shape-specialised twin PPO update kernel (gpu-marked):
mlp_bwd_fused_twin_shaped_f32 against the generic twin kernel that
RL_REPLICAS_AMD_TWIN_SHAPED=0 selects, and the wave-per-row
value_loss_finalize_rows against a sequential CPU sum.  The shaped kernel
feeds every MFMA accumulator the same operands in the same order and
keeps every other expression, so all comparisons are torch.equal.

Net pairs hit the runtime edges of the [in, 64, 32, out] shape: the bench
pair; in = 5 (below one column tile, no multiple of 4) with out = 3; in =
27 (two ragged layer-0 column tiles) with out = 8.  Batch 33 is two row
blocks with a 1-row tail (zero-filled rows), 160 an odd block count."""
import pytest
import torch

from test_gpu_ppo_twin_iter import (GATE_CASES, _Side, _run_two_epochs,
                                    assert_all_equal)

pytestmark = pytest.mark.gpu

SWITCH = "RL_REPLICAS_AMD_TWIN_SHAPED"
NET_PAIRS = {
    "bench": ([17, 64, 32, 6], [17, 64, 32, 1]),
    "narrow_in": ([5, 64, 32, 3], [5, 64, 32, 1]),
    "ragged_in": ([27, 64, 32, 8], [27, 64, 32, 1]),
}
INELIGIBLE = ([5, 24, 3], [5, 16, 8, 1])
BATCHES = [33, 160]


@pytest.fixture(scope="module")
def ext():
    from rl_replicas_amd import ops

    assert ops.hip_available()
    return ops._load_extension()


def _full_state(side):
    return side.policy_state() + side.value_state()


def _run_both(ext, monkeypatch, pdims, vdims, batch, case):
    """Three iterations on two identical sides, `a` with the switch unset
    and `b` with it at 0; compares all state after every iteration."""
    gate_open = case != "closed_on_entry"
    a = _Side(ext, pdims, vdims, batch, gate_open)
    b = _Side(ext, pdims, vdims, batch, gate_open)
    value0 = [t.clone() for t in a.vw + a.vb]
    for i, (first_iter, thr) in enumerate(GATE_CASES[case]):
        monkeypatch.delenv(SWITCH, raising=False)
        a.twin(i, first_iter, thr)
        monkeypatch.setenv(SWITCH, "0")
        b.twin(i, first_iter, thr)
        torch.cuda.synchronize()
        assert_all_equal(_full_state(a), _full_state(b), f"iteration {i}")
    # the kernels did run: the value half moves whatever the gate says
    assert not any(torch.equal(p, q) for p, q in zip(a.vw + a.vb, value0))
    return a


@pytest.mark.parametrize("case", list(GATE_CASES))
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("pair", list(NET_PAIRS))
def test_shaped_equals_generic_twin(ext, monkeypatch, pair, batch, case):
    pdims, vdims = NET_PAIRS[pair]
    monkeypatch.delenv(SWITCH, raising=False)
    assert ext.ppo_twin_uses_shaped(pdims, vdims, batch)
    monkeypatch.setenv(SWITCH, "0")
    assert not ext.ppo_twin_uses_shaped(pdims, vdims, batch)
    a = _run_both(ext, monkeypatch, pdims, vdims, batch, case)
    if case == "first_iter":
        assert float(a.gate) == 1.0 and float(a.iters_done) == 2.0
    elif case == "closes_in_call":
        assert float(a.gate) == 0.0 and float(a.iters_done) == 1.0


def test_ineligible_pair_takes_generic_kernel(ext, monkeypatch):
    """Nets outside [in, 64, 32, out] never reach the shaped kernel, with
    the switch unset as with it at 0, and the iteration still agrees."""
    pdims, vdims = INELIGIBLE
    monkeypatch.delenv(SWITCH, raising=False)
    assert not ext.ppo_twin_uses_shaped(pdims, vdims, 33)
    # one hidden width off, an output too wide, a value head that is no scalar
    assert not ext.ppo_twin_uses_shaped([17, 64, 16, 6], [17, 64, 32, 1], 33)
    assert not ext.ppo_twin_uses_shaped([17, 64, 32, 17], [17, 64, 32, 1], 33)
    assert not ext.ppo_twin_uses_shaped([17, 64, 32, 6], [17, 64, 32, 2], 33)
    assert not ext.ppo_twin_uses_shaped([65, 64, 32, 6], [65, 64, 32, 1], 33)
    _run_both(ext, monkeypatch, pdims, vdims, 33, "first_iter")


def test_epoch_graph_shaped_equals_generic(ext, monkeypatch):
    """Two epochs of the captured twin graph (_GraphedPPOTwin) from
    identical fresh models, with the shaped kernel and without it."""
    monkeypatch.setenv("RL_REPLICAS_AMD_PPO_TWIN", "1")
    monkeypatch.delenv(SWITCH, raising=False)
    s1, m1, it1, twin1 = _run_two_epochs(7, 7, 1e9)
    monkeypatch.setenv(SWITCH, "0")
    s0, m0, it0, twin0 = _run_two_epochs(7, 7, 1e9)
    assert twin1 and twin0
    assert it1 == it0 == [7, 7]
    assert m1 == m0
    assert_all_equal(s1, s0, "epoch graph")


@pytest.mark.parametrize("fb", [125, 7])
def test_value_loss_finalize_rows_sequential_sum(ext, fb):
    """Each row's sum is the float32 left-to-right sum from 0.f.  Row
    stride 130 > fb: the tail of a row (NaN here) is never added."""
    rows, stride = 3, 130
    g = torch.Generator().manual_seed(7)
    p = torch.randn(rows, stride, generator=g)
    p[:, fb:] = float("nan")
    want = torch.zeros(rows)
    for r in range(rows):
        s = torch.zeros(())
        for c in range(fb):
            s = s + p[r, c]
        want[r] = s
    got = ext.value_loss_finalize(p.cuda(), fb).cpu()
    assert torch.equal(got, want)
