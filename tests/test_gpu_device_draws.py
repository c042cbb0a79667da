"""
Self-play draws on the MI355X (libmzx.so): the check functions of tests/device_draws_cases.py on the device library.
Tape, action choice and determinism are bit-exact (no libm); the noise is held to the restatement within 1e-12 relative
-- the device log / exp / pow are within 3 / 3 / 16 ulp, amplified by at most 1 / alpha = 10 in the shape < 1 branch:
about 64 ulp = 1.4e-14, plus the sum and the division; the gate leaves a factor of about 70 -- with no row excused: the
cases module asserts that no accept / reject comparison of the grid is closer than 1e-9 to its boundary.
Every case is a few launches on tiny buffers.
"""
import pytest

import device_draws_cases as cases
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def test_library_words_on_the_device(backend):
    cases.check_library_words(backend)


@pytest.mark.parametrize("ai", range(len(cases.ACTIONS)), ids=[f"A{a}" for a in cases.ACTIONS])
def test_tape_bit_for_bit_and_noise_within_the_gate_on_the_device(backend, ai):
    cases.check_margins(ai)
    cases.check_grid(backend, ai, exact_noise=False)


def test_longer_tape_begins_with_the_shorter_on_the_device(backend):
    cases.check_tape_prefix(backend)


@pytest.mark.parametrize("ai", range(len(cases.ACTIONS)), ids=[f"A{a}" for a in cases.ACTIONS])
def test_action_choice_bit_for_bit_on_the_device(backend, ai):
    cases.check_select(backend, ai)


def test_action_choice_boundaries_on_the_device(backend):
    cases.check_select_boundaries(backend)


def test_dirichlet_moments_on_the_device(backend):
    cases.check_distribution(backend)


def test_determinism_and_independence_on_the_device(backend):
    cases.check_determinism(backend)


def test_refusals_on_the_device(backend):
    cases.check_refusals(backend)


@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_fused_move_is_draws_search_select_on_the_device(backend, kind):
    cases.check_composition(backend, kind)


def test_native_rounds_equal_the_python_loop_with_device_draws_on_the_device(backend):
    cases.check_selfplay_rounds(backend)


def test_tape_overflow_takes_the_retry_path_on_the_device(backend):
    cases.check_selfplay_rounds(backend, zero_weights=True)


def test_the_actor_seed_keys_the_draws_on_the_device(backend):
    cases.check_actor_seed(backend)


def test_move_and_selfplay_refusals_on_the_device(backend):
    cases.check_move_refusals(backend)
