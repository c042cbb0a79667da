"""
Resident rounds (config.device_games; csrc/mzx_resident.h) through the product library on the GPU.  The comparator is the
host loop with device draws on the same device, bit for bit: both feed identical inputs to identical search kernels, so no
tolerance is needed (tests/resident_rounds_cases.py).
"""
import pytest

import resident_rounds_cases as cases
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def test_resident_tictactoe(backend):
    cases.check_tictactoe(backend)


def test_resident_connect4(backend):
    cases.check_connect4(backend)


def test_resident_connect4_partial_last_workgroup(backend):
    cases.check_connect4(backend, B=65, calls=[(1.0, dict(max_rounds=30, min_games=cases.FOREVER))])


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
