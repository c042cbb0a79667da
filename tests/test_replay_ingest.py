"""
Bulk ingest of a shard's finished games into the device replay store on the serial build of the functors
(tests/hostcheck): the check functions of tests/replay_ingest_cases.py, which tests/test_gpu_replay_ingest.py runs on the
device library.  The reference of every check is the per-game path (``add_many`` / ``save_game``) as it stands.
"""
import pytest

import hostcheck
import replay_ingest_cases as cases


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


@pytest.mark.parametrize("geometry", list(cases.GEOMETRIES))
def test_columns_bit_for_bit_with_staged_priorities(backend, geometry):
    cases.check_columns(backend, geometry, per=True, staged=True)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.7])
@pytest.mark.parametrize("geometry", ["cartpole", "odd-frame"])
def test_priorities_computed_by_the_kernel(backend, geometry, alpha):
    cases.check_columns(backend, geometry, per=True, staged=False, alpha=alpha)


@pytest.mark.parametrize("geometry", ["cartpole", "connect4"])
def test_columns_without_per(backend, geometry):
    cases.check_columns(backend, geometry, per=False, staged=False)


def test_store_without_sampler_and_without_mask_column(backend):
    cases.check_columns(backend, "odd-frame", per=True, staged=True, max_games=None, legal_masks=False)


def test_hand_off_that_wraps_the_pool(backend):
    cases.check_wrap(backend)


def test_store_full_leaves_the_store_unchanged(backend):
    cases.check_store_full(backend)


def test_forced_chunks(backend):
    cases.check_chunks(backend)


def test_mixed_hand_off(backend):
    cases.check_mixed(backend)


@pytest.mark.parametrize("per", [True, False])
def test_downstream_results(backend, per):
    cases.check_downstream(backend, per)


@pytest.mark.parametrize("situation", ["plain", "size-eviction", "position-eviction", "slot-eviction", "mixed", "oversized",
                                       "no-store", "plain-list"])
def test_save_games_against_the_loop(backend, situation):
    cases.check_save_games(backend, situation)


@pytest.mark.parametrize("order", [(0, 2, 1), (0, 1, 2)], ids=["3-3-5", "3-5-3"])
@pytest.mark.parametrize("rows", [10, 11, 12])
def test_save_games_when_the_hand_off_evicts_its_own_games(backend, rows, order):
    cases.check_handoff_eviction(backend, rows, order)


def test_frame_copy_paths(backend):
    cases.check_frame_paths(backend)


def test_abi_refusals(backend):
    cases.check_abi_refusals(backend)


def test_end_to_end(backend):
    cases.check_end_to_end(backend)
