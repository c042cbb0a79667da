"""
mzx.trainer.train_steps (mzx_train_chain) on the serial test double of the ABI, against the loop of its definition, bit
for bit (tests/train_chain_cases.py).
"""
import pytest

import hostcheck
import train_chain_cases as cases


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


@pytest.mark.parametrize("name,per,n", cases.ROWS, ids=[f"{name}-{'per' if per else 'uniform'}-n{n}" for name, per, n in cases.ROWS])
def test_a_chain_leaves_what_the_loop_leaves(be, name, per, n):
    cases.check_row(be, name, per, n)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_chain_from_a_fresh_optimizer(be, kind):
    """No warm-up step: the chain creates the optimizer state and ``.grad`` (SGD: the first-step launch, then momentum)."""
    cases.check_row(be, "fc_b5_k4", True, 5, kind=kind, warm=False)


def test_sgd_with_momentum_on_a_residual_network(be):
    cases.check_row(be, "resnet_b_b3_k3", True, 5, kind="sgd")


def test_the_store_makes_windows_overlap_and_pass_game_ends(be):
    cases.check_windows_overlap_and_pass_game_ends(be)


@pytest.mark.parametrize("what", cases.REFUSALS)
def test_refusals_name_what_is_missing_and_queue_nothing(be, what):
    cases.check_refusal(be, what)
