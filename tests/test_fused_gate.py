"""The one persistent-kernel gate of ops/fused_rollout.py and the samplers'
lockstep arithmetic, on the CPU: the gate takes the binding's limits and its
LDS function as arguments, so no extension is needed."""
import pytest
import torch

from rl_replicas_amd.ops.fused_rollout import _fused_gate
from rl_replicas_amd.samplers.device_sampler import lockstep_cuts, segment_bounds

MAX_LDS = 65536
LIMITS = (3, 64, 16, MAX_LDS)  # max_layers, max_width, max_cuts, max_lds
LIMITS_NO_CUT_CAP = (3, 64, MAX_LDS)
ENV = "RL_REPLICAS_AMD_ROLLOUT_FUSED"


def _lds(dims):
    return 4 * sum(a * b for a, b in zip(dims, dims[1:]))


def _net(dims, dtype=torch.float32, fp64_layer=None):
    ws = [torch.zeros(o, i, dtype=dtype) for i, o in zip(dims, dims[1:])]
    if fp64_layer is not None:
        ws[fp64_layer] = ws[fp64_layer].double()
    return ws


GOOD = [3, 64, 32, 1]
CUTS17 = tuple(range(17))
F32 = torch.zeros(1)
F64 = torch.zeros(1, dtype=torch.float64)

# id: (want, dims, gate kwargs, env value or None for unset)
GATE_CASES = {
    "accepted": (True, GOOD, {}, None),
    "four_layers": (False, [3, 8, 8, 8, 1], {}, None),
    "width_65": (False, [3, 65, 1], {}, None),
    "width_64": (True, [3, 64, 1], {}, None),
    "wrong_input_width": (False, [4, 64, 32, 1], {}, None),
    "wrong_output_width_required": (False, [3, 64, 32, 2], {}, None),
    "any_output_width_when_none_required": (True, [3, 64, 32, 2], {"out_dim": None}, None),
    "17_cuts_cap_given": (False, GOOD, {"cuts": CUTS17}, None),
    "16_cuts_cap_given": (True, GOOD, {"cuts": CUTS17[:16]}, None),
    "17_cuts_no_cap_given": (True, GOOD, {"cuts": CUTS17, "limits": LIMITS_NO_CUT_CAP}, None),
    "no_cut_list": (True, GOOD, {"cuts": None}, None),
    "fp64_weight": (False, GOOD, {"fp64_layer": 1}, None),
    "fp64_extra_tensor": (False, GOOD, {"extra_fp32": [F32, F64]}, None),
    "fp32_extra_tensor": (True, GOOD, {"extra_fp32": [F32]}, None),
    "lds_one_byte_over": (False, GOOD, {"lds_bytes": lambda dims: MAX_LDS + 1}, None),
    "lds_exactly_at_the_limit": (True, GOOD, {"lds_bytes": lambda dims: MAX_LDS}, None),
    "env_0": (False, GOOD, {}, "0"),
    "env_1": (True, GOOD, {}, "1"),
    "env_unset_default_false": (False, GOOD, {"default": False}, None),
    "env_1_default_false": (True, GOOD, {"default": False}, "1"),
    "env_0_default_false": (False, GOOD, {"default": False}, "0"),
}


@pytest.mark.parametrize("case", list(GATE_CASES))
def test_fused_gate(monkeypatch, case):
    want, dims, kw, env = GATE_CASES[case]
    kw = dict(kw)
    monkeypatch.delenv("RL_REPLICAS_AMD_COMPUTE_DTYPE", raising=False)
    if env is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, env)
    weights = _net(dims, fp64_layer=kw.pop("fp64_layer", None))
    got = _fused_gate(
        weights, kw.pop("extra_fp32", ()), kw.pop("limits", LIMITS),
        kw.pop("lds_bytes", _lds), 3, kw.pop("out_dim", 1), kw.pop("cuts", ()),
        **kw)
    assert got is want


def test_fused_gate_bf16_compute_and_no_net(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.setenv("RL_REPLICAS_AMD_COMPUTE_DTYPE", "bf16")
    assert not _fused_gate(_net(GOOD), (), LIMITS, _lds, 3, 1)
    monkeypatch.delenv("RL_REPLICAS_AMD_COMPUTE_DTYPE")
    # a body that reads no net (the uniform draw): only the switches and the cuts
    assert _fused_gate(None, (), LIMITS, _lds, 3, 1, CUTS17[:16])
    assert not _fused_gate(None, (), LIMITS, _lds, 3, 1, CUTS17)
    monkeypatch.setenv(ENV, "0")
    assert not _fused_gate(None, (), LIMITS, _lds, 3, 1, ())


# steps = 5; the cut is the step after which (start_elapsed + t + 1) is a
# multiple of the horizon.  Written out by hand:
#   horizon 3, elapsed 0: steps 0 1 2|3 4      -> cut after step 2
#   horizon 3, elapsed 1: steps 0 1|2 3 4|     -> cuts after steps 1 and 4
#   horizon 3, elapsed 2: steps 0|1 2 3|4      -> cuts after steps 0 and 3
LOCKSTEP_CASES = [
    # horizon, start_elapsed, cuts, (start, end, done) segments
    (3, 0, (2,), [(0, 3, True), (3, 5, False)]),
    (3, 1, (1, 4), [(0, 2, True), (2, 5, True)]),  # last step is a cut: no open tail
    (3, 2, (0, 3), [(0, 1, True), (1, 4, True), (4, 5, False)]),
    (None, 0, (), [(0, 5, False)]),
    (None, 2, (), [(0, 5, False)]),
]


@pytest.mark.parametrize("horizon,start_elapsed,cuts,bounds", LOCKSTEP_CASES)
def test_lockstep_cuts_and_segment_bounds(horizon, start_elapsed, cuts, bounds):
    got = lockstep_cuts(5, horizon, start_elapsed)
    assert isinstance(got, tuple) and got == cuts
    assert segment_bounds(5, got) == bounds
    # the segments tile the epoch, and only the last may be open
    assert [s for s, _, _ in bounds] == [0] + [e for _, e, _ in bounds[:-1]]
    assert bounds[-1][1] == 5 and all(d for _, _, d in bounds[:-1])
