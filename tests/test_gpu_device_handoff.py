"""
Reading games back from the device replay store on the MI355X (libmzx.so): the check functions of
tests/device_handoff_cases.py on the device library.  Every case is one launch over at most a few hundred pool rows.
"""
import pytest

import device_handoff_cases as cases
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.mark.parametrize("optional", [(True, True), (False, False), (True, False), (False, True)],
                         ids=["mask+priorities", "bare", "mask", "priorities"])
@pytest.mark.parametrize("geometry", ["odd-frame", "long-frame", "connect4", "wide"])
def test_download_games_bit_for_bit_on_the_device(backend, geometry, optional):
    cases.check_download(backend, geometry, *optional)


def test_download_games_refusals_on_the_device(backend):
    cases.check_download_refusals(backend)


def test_download_reads_the_pool_as_it_lies_on_the_device(backend):
    cases.check_download_after_reanalyse(backend)


def test_export_frame_copy_paths_on_the_device(backend):
    cases.check_frame_paths(backend)


def test_export_passes_over_a_game_outside_the_pool_on_the_device(backend):
    cases.check_passed_over(backend)


def test_export_abi_refusals_on_the_device(backend):
    cases.check_abi_refusals(backend)


# ---- the device hand-off (config.device_handoff) against the twin that goes through the host

@pytest.mark.parametrize("per", [True, False])
def test_handoff_tictactoe_on_the_device(backend, per):
    cases.check_handoff_tictactoe(backend, per)


def test_handoff_synthetic_max_moves_on_the_device(backend):
    cases.check_handoff_synthetic(backend)


def test_handoff_connect4_partial_workgroup_on_the_device(backend):
    cases.check_handoff_connect4(backend)


@pytest.mark.parametrize("situation", ["positions", "slots"])
def test_handoff_eviction_inside_the_hand_off_on_the_device(backend, situation):
    cases.check_handoff_eviction(backend, situation)


def test_handoff_halt_and_repair_on_the_device(backend):
    cases.check_handoff_halt_and_repair(backend)


def test_it_was_on_the_device_on_the_mi355x(backend):
    cases.check_it_was_on_the_device(backend)


def test_handoff_overlap_on_the_device(backend):
    cases.check_overlap(backend)


def test_handoff_refusals_on_the_device(backend):
    cases.check_refusals(backend)


def test_handoff_max_log_bytes_on_the_device(backend):
    cases.check_max_log_bytes(backend)
