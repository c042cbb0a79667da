"""
Resident rounds (config.device_games; csrc/mzx_resident.h) on the serial build of the ABI: the vote, commit and gather
wave bodies executed with one lane and the host's chunk loop around them, against the native round loop on device draws
(tests/resident_rounds_cases.py has the checks and what "same" means).
"""
import pytest

import hostcheck
import resident_rounds_cases as cases


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


def test_resident_tictactoe(backend):
    cases.check_tictactoe(backend)


def test_resident_connect4(backend):
    cases.check_connect4(backend)


def test_resident_gomoku(backend):
    cases.check_gomoku(backend)


def test_resident_synthetic(backend):
    cases.check_synthetic(backend)


def test_resident_halt_and_repair(backend):
    cases.check_halt_and_repair(backend)


def test_resident_min_games(backend):
    cases.check_min_games(backend)


def test_resident_three_groups(backend):
    cases.check_three_groups(backend)


def test_resident_draw_counter(backend):
    cases.check_draw_counter(backend)


def test_resident_refusals(backend):
    cases.check_refusals(backend)


def test_resident_continuous_self_play(backend):
    cases.check_continuous_self_play(backend)
