"""
The device-resident game twin (mzx_game_device_*, csrc/mzx_games_device.h) through the product library on the GPU: one
wavefront per game, against the host game object of the same library, bit for bit (tests/device_games_cases.py).
"""
import pytest

import device_games_cases as cases
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.mark.parametrize("name", sorted(cases.KINDS))
def test_device_game_equals_the_host_game(backend, name):
    cases.check_twin_equals_host(backend, name)


def test_out_of_range_actions_and_reset_indices_touch_nothing(backend):
    cases.check_out_of_range_inputs_touch_nothing(backend)


def test_device_game_refusals(backend):
    cases.check_refusals(backend)
