"""
mzx.trainer.Trainer on the serial test double of the ABI (tests/trainer_worker_cases.py): the worker loop in chunks
against a twin per-step loop, the reference's sequence of set_info calls, the ratio wait and terminate, the routes.
"""
import pytest

import hostcheck
import trainer_worker_cases as cases


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


def test_the_loop_in_chunks_publishes_what_a_per_step_loop_holds(be):
    cases.check_loop(be)


def test_chunks_of_one_make_the_reference_sequence_of_set_info_calls(be):
    cases.check_reference_sequence(be)


def test_the_ratio_wait_polls_until_terminate_and_trains_no_further(be, monkeypatch):
    cases.check_ratio_wait(be, monkeypatch)


def test_terminate_before_the_first_chunk_trains_nothing(be, monkeypatch):
    cases.check_terminate_first(be, monkeypatch)


def test_the_loop_waits_for_the_first_played_game(be, monkeypatch):
    cases.check_waits_for_a_game(be, monkeypatch)


def test_a_torch_model_takes_the_per_step_route(be):
    cases.check_torch_model_route(be)


def test_a_buffer_without_the_device_sampler_takes_the_host_route(be):
    cases.check_host_buffer_route(be)


def test_bound_forms_and_a_resumed_checkpoint(be):
    cases.check_bound_forms_and_checkpoint(be)
