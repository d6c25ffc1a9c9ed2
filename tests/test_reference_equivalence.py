"""Update-equivalence harness: our CPU path vs the reference implementation.

Real MuJoCo is unavailable offline, so the reference's published return
curves can't be reproduced directly (round-1 VERDICT.md, gap #2).  This
suite proves the ALGORITHM MATH instead: the actual reference modules
(gymnasium/tensorboard stubbed — see tests/_reference_loader.py) and our
stack are fed byte-identical Experience/minibatch data from identically
initialized networks, and the resulting losses, KL, GAE pipeline, CG
step and post-update parameters must agree to fp32 tolerance for all
five algorithms:

  VPG/PPO/TRPO  — full train(experience) epoch (reference vpg.py:127-192,
                  ppo.py:139-223, trpo.py:130-240)
  DDPG/TD3      — full train(buffer, n, mb) loop under matched RNG
                  streams (reference ddpg.py:195-253, td3.py:214-263)
  CG optimizer  — step() on identical closures (reference CGO:59-98)
  utils         — scan/GAE/bootstrap/normalize/polyak primitives

The reference side of every case is recorded once, by
tools/record_reference_golden.py running the case functions of
tests/_equivalence_cases.py on the reference modules, into
tests/golden/reference_equivalence.npz; the tests run the same case
functions on our stack and compare against that record, so the suite
needs no reference checkout.

Our HIP kernels are separately pinned to this CPU path by the GPU
numerics tests, so equivalence is transitive: kernels == our CPU path ==
reference.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _equivalence_cases as cases


@pytest.fixture(scope="module")
def ours():
    return cases.our_namespace()


def _sub(results, prefix):
    """{state-dict key: tensor} of the entries under '<prefix>/'."""
    prefix = prefix + "/"
    return {
        k[len(prefix):]: torch.from_numpy(np.asarray(v))
        for k, v in results.items()
        if k.startswith(prefix)
    }


def _assert_modules_close(ref, our, module, rtol=1e-4, atol=1e-6, label=""):
    ref_sd = _sub(ref, module)
    our_sd = _sub(our, module)
    assert ref_sd, f"{label}: no recorded reference state for {module}"
    assert ref_sd.keys() == our_sd.keys(), label
    for k in ref_sd:
        torch.testing.assert_close(
            our_sd[k], ref_sd[k], rtol=rtol, atol=atol, msg=f"{label}:{k}"
        )


def _assert_same_init(ref, our, module="init_policy"):
    """Both sides must have started from bit-identical weights."""
    ref_sd = _sub(ref, module)
    our_sd = _sub(our, module)
    assert ref_sd.keys() == our_sd.keys()
    for k in ref_sd:
        assert torch.equal(our_sd[k], ref_sd[k]), f"initial weights differ: {k}"


def _metric(results, tag):
    return float(results["metric/" + tag])


def _metric_tags(results):
    return {k[len("metric/"):] for k in results if k.startswith("metric/")}


# ---------------------------------------------------------------------------
# utils primitives
# ---------------------------------------------------------------------------
def test_utils_equivalence(ours):
    ref = cases.load_golden("utils")
    our = cases.run_utils(ours)

    np.testing.assert_allclose(
        our["discounted_cumulative_sums"],
        ref["discounted_cumulative_sums"],
        rtol=1e-6,
    )
    np.testing.assert_allclose(our["gae"], ref["gae"], rtol=1e-5, atol=1e-6)

    assert int(our["bootstrap/count"]) == int(ref["bootstrap/count"]) == 2
    for i in range(int(ref["bootstrap/count"])):
        np.testing.assert_allclose(ref[f"bootstrap/{i}"], our[f"bootstrap/{i}"])

    torch.testing.assert_close(
        torch.from_numpy(our["normalize_tensor"]),
        torch.from_numpy(ref["normalize_tensor"]),
    )

    for i in range(2):
        torch.testing.assert_close(
            torch.from_numpy(our[f"polyak_average/{i}"]),
            torch.from_numpy(ref[f"polyak_average/{i}"]),
        )


# ---------------------------------------------------------------------------
# on-policy: full train(experience) equivalence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo_name", ["VPG", "PPO", "TRPO"])
def test_onpolicy_train_equivalence(ours, algo_name):
    ref = cases.load_golden(f"onpolicy_{algo_name}")
    our = cases.run_onpolicy(ours, algo_name)
    _assert_same_init(ref, our)

    if algo_name == "TRPO":
        # Both stacks must take the SAME accepted trust-region step
        # (direction + length).  Element tolerances don't fit here: 10 CG
        # iterations on the damped (1e-5) Fisher amplify fp noise to
        # ~0.3% of the step vector, so compare the steps as vectors.
        def step(results):
            init = _sub(results, "init_policy")
            return torch.cat(
                [(v - init[k]).flatten() for k, v in _sub(results, "policy").items()]
            )

        step_ref = step(ref)
        step_our = step(our)
        assert step_ref.numel() == step_our.numel() > 0
        cos = torch.dot(step_ref, step_our) / (step_ref.norm() * step_our.norm())
        assert float(cos) > 0.999, f"CG step direction diverged: cos={float(cos)}"
        ratio = float(step_our.norm() / step_ref.norm())
        assert abs(ratio - 1.0) < 0.02, f"accepted step length diverged: {ratio}"
    else:
        _assert_modules_close(ref, our, "policy", label=f"{algo_name}.policy")
        torch.testing.assert_close(
            torch.from_numpy(our["log_std"]),
            torch.from_numpy(ref["log_std"]),
            rtol=1e-4,
            atol=1e-6,
        )
    _assert_modules_close(ref, our, "value", label=f"{algo_name}.value")
    if _sub(ref, "old_policy") and algo_name != "TRPO":
        # (TRPO's old_policy is synced to the post-step policy, so it
        # carries the same CG fp noise compared above as a step vector)
        _assert_modules_close(ref, our, "old_policy", label=f"{algo_name}.old_policy")

    for tag in ("policy/loss", "value_function/average_loss", "policy/avarage_entropy"):
        if tag in _metric_tags(ref) and tag in _metric_tags(our):
            assert _metric(our, tag) == pytest.approx(
                _metric(ref, tag), rel=1e-3, abs=1e-6
            ), tag


def test_ppo_kl_and_early_stop_metric_equivalence(ours):
    """PPO's approx-KL drives early stop (reference ppo.py:173-181): the
    recorded kl_divergence after the epoch must match."""
    ref = cases.load_golden("ppo_kl")
    our = cases.run_onpolicy(ours, "PPO", rollout_seed=7)
    _assert_same_init(ref, our)
    ref_kl = _metric(ref, "policy/kl_divergence")
    our_kl = _metric(our, "policy/kl_divergence")
    assert our_kl == pytest.approx(ref_kl, rel=1e-3, abs=1e-7)


# ---------------------------------------------------------------------------
# CG optimizer: identical closures -> identical accepted step
# ---------------------------------------------------------------------------
def test_cg_optimizer_step_equivalence(ours):
    ref = cases.load_golden("cg_optimizer")
    our = cases.run_cg_optimizer(ours)
    assert list(_sub(ref, "net")) == list(_sub(our, "net"))
    _assert_modules_close(ref, our, "net", rtol=1e-5, atol=1e-7, label="cg")


# ---------------------------------------------------------------------------
# off-policy: full train(buffer, n, mb) equivalence under matched RNG
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo_name", ["DDPG", "TD3"])
def test_offpolicy_train_equivalence(ours, algo_name):
    ref = cases.load_golden(f"offpolicy_{algo_name}")
    our = cases.run_offpolicy(ours, algo_name)

    _assert_modules_close(ref, our, "policy", label=f"{algo_name}.policy")
    _assert_modules_close(ref, our, "target_policy", label=f"{algo_name}.target_policy")
    for name in cases.OFFPOLICY_MODULES[algo_name]:
        _assert_modules_close(ref, our, name, label=f"{algo_name}.{name}")

    shared = _metric_tags(ref) & _metric_tags(our)
    assert shared, "no common metric tags recorded"
    for tag in shared:
        assert _metric(our, tag) == pytest.approx(_metric(ref, tag), rel=1e-3, abs=1e-5), tag


def test_ppo_categorical_train_equivalence(ours):
    """PPO with a CategoricalPolicy (the reference's discrete-action
    config, reference categorical_policy.py:8-32) — full train()
    equivalence on identical integer-action rollouts."""
    ref = cases.load_golden("ppo_categorical")
    our = cases.run_ppo_categorical(ours)

    _assert_modules_close(ref, our, "policy", label="PPO-cat.policy")
    _assert_modules_close(ref, our, "value", label="PPO-cat.value")
    assert _metric(our, "policy/kl_divergence") == pytest.approx(
        _metric(ref, "policy/kl_divergence"), rel=1e-3, abs=1e-7
    )
