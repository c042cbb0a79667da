"""
Self-play draws on the device, on the serial build (tests/hostcheck): the check functions of tests/device_draws_cases.py
-- the numpy / math restatement of csrc/mzx_draws.h, bit for bit (the serial build calls the libm Python's math calls).
"""
import pytest

import device_draws_cases as cases
import hostcheck


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


def test_philox_known_answers_through_the_draws_layout(backend):
    cases.check_known_answers()
    cases.check_library_words(backend)


@pytest.mark.parametrize("ai", range(len(cases.ACTIONS)), ids=[f"A{a}" for a in cases.ACTIONS])
def test_comparison_margins_of_the_grid(ai):
    cases.check_margins(ai)


@pytest.mark.parametrize("ai", range(len(cases.ACTIONS)), ids=[f"A{a}" for a in cases.ACTIONS])
def test_tape_and_noise_bit_for_bit(backend, ai):
    cases.check_grid(backend, ai, exact_noise=True)


def test_longer_tape_begins_with_the_shorter(backend):
    cases.check_tape_prefix(backend)


@pytest.mark.parametrize("ai", range(len(cases.ACTIONS)), ids=[f"A{a}" for a in cases.ACTIONS])
def test_action_choice_bit_for_bit(backend, ai):
    cases.check_select(backend, ai)


def test_action_choice_boundaries(backend):
    cases.check_select_boundaries(backend)


def test_dirichlet_moments(backend):
    cases.check_distribution(backend)


def test_determinism_and_independence(backend):
    cases.check_determinism(backend)


def test_refusals(backend):
    cases.check_refusals(backend)


@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_fused_move_is_draws_search_select(backend, kind):
    cases.check_composition(backend, kind)


def test_continued_searches_without_rngs(backend):
    cases.check_engine_continued(backend)


def test_native_rounds_equal_the_python_loop_with_device_draws(backend):
    cases.check_selfplay_rounds(backend)


def test_tape_overflow_takes_the_retry_path_and_still_matches(backend):
    cases.check_selfplay_rounds(backend, zero_weights=True)


def test_the_actor_seed_keys_the_draws(backend):
    cases.check_actor_seed(backend)


def test_lockstep_play_games_with_device_draws(backend):
    cases.check_selfplay_lockstep(backend)


def test_move_and_selfplay_refusals(backend):
    cases.check_move_refusals(backend)
