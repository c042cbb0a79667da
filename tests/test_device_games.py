"""
The device-resident game twin (mzx_game_device_*, csrc/mzx_games_device.h) on the serial build of the ABI: the wave
bodies executed with one lane, the same statements the product kernels run (tests/device_games_cases.py has the checks
and what they compare against).
"""
import pytest

import device_games_cases as cases
import hostcheck


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


@pytest.mark.parametrize("name", sorted(cases.KINDS))
def test_device_game_equals_the_host_game(backend, name):
    cases.check_twin_equals_host(backend, name)


def test_out_of_range_actions_and_reset_indices_touch_nothing(backend):
    cases.check_out_of_range_inputs_touch_nothing(backend)


def test_device_game_refusals(backend):
    cases.check_refusals(backend)
