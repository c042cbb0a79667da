"""
Reading games back from the device replay store on the serial build of the functors (tests/hostcheck): the check functions
of tests/device_handoff_cases.py, which tests/test_gpu_device_handoff.py runs on the device library.  The reference of
every check is a numpy restatement over plain host copies of the pool's columns.
"""
import pytest

import device_handoff_cases as cases
import hostcheck


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


@pytest.mark.parametrize("optional", [(True, True), (False, False), (True, False), (False, True)],
                         ids=["mask+priorities", "bare", "mask", "priorities"])
@pytest.mark.parametrize("geometry", ["odd-frame", "long-frame", "connect4", "wide"])
def test_download_games_bit_for_bit(backend, geometry, optional):
    cases.check_download(backend, geometry, *optional)


def test_download_games_refusals(backend):
    cases.check_download_refusals(backend)


def test_download_reads_the_pool_as_it_lies(backend):
    cases.check_download_after_reanalyse(backend)


def test_export_frame_copy_paths(backend):
    cases.check_frame_paths(backend)


def test_export_passes_over_a_game_outside_the_pool(backend):
    cases.check_passed_over(backend)


def test_export_abi_refusals(backend):
    cases.check_abi_refusals(backend)


# ---- the device hand-off (config.device_handoff) against the twin that goes through the host

@pytest.mark.parametrize("per", [True, False])
def test_handoff_tictactoe(backend, per):
    cases.check_handoff_tictactoe(backend, per)


def test_handoff_synthetic_max_moves(backend):
    cases.check_handoff_synthetic(backend)


def test_handoff_connect4_partial_workgroup(backend):
    cases.check_handoff_connect4(backend)


@pytest.mark.parametrize("situation", ["positions", "slots"])
def test_handoff_eviction_inside_the_hand_off(backend, situation):
    cases.check_handoff_eviction(backend, situation)


def test_handoff_halt_and_repair(backend):
    cases.check_handoff_halt_and_repair(backend)


def test_it_was_on_the_device(backend):
    cases.check_it_was_on_the_device(backend)


def test_handoff_overlap(backend):
    cases.check_overlap(backend)


def test_handoff_refusals(backend):
    cases.check_refusals(backend)


def test_handoff_max_log_bytes(backend):
    cases.check_max_log_bytes(backend)
