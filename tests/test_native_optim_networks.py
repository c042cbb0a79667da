"""
``mzx.optim.Adam`` / ``mzx.optim.SGD`` on networks, on the serial test double of the ABI (tests/native_optim_net_cases.py):
two steps on a fully connected network against the restatement bit for bit and against torch within torch's own error, a
residual network's statistics and a stem's bypassed tensors left alone, optimizer state round trips, a reference-format
state loaded into a native optimizer, the constructor refusals.
"""
import pytest

import hostcheck
import native_optim_net_cases as cases


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


KINDS = ["adam", "sgd"]


@pytest.mark.parametrize("kind", KINDS)
def test_two_steps_are_the_restatement_and_within_torchs_own_error(be, kind):
    cases.check_two_steps(be, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_residual_statistics_hold_the_commit_and_have_no_state(be, kind):
    cases.check_residual(be, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", cases.STEM_CASES, ids=lambda c: c["name"])
def test_bypassed_tensors_behind_a_stem_keep_their_bits(be, case, kind):
    cases.check_stem(be, case, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_state_round_trip(be, kind):
    cases.check_round_trip(be, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_a_reference_format_state_of_a_torch_optimizer_loads(be, kind):
    cases.check_reference_state_loads(be, kind)


def test_constructor_refusals(be):
    cases.check_constructor_refusals(be)
