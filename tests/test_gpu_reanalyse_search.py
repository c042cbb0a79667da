"""
Reanalyse with fresh searches over the device-resident replay store on the MI355X (libmzx.so): the check functions of
tests/test_reanalyse_search.py on the device library, plus a connect4 buffer of played games swept in chunks of 256 roots
on whatever route the search takes at that tree count.  Every comparison is bit for bit.
"""
import ctypes

import numpy
import pytest

from mzx import _lib, games
from test_reanalyse_search import (INPUT_CASES, check_downstream, check_inputs, check_refusals, check_selection_and_errors,
                                   check_sweep, check_worker, check_write, engine_for, played_store, search_config, sweep_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.mark.parametrize("kind,A,masks", INPUT_CASES)
def test_search_inputs_on_the_device(backend, kind, A, masks):
    check_inputs(backend, kind, A, masks)


@pytest.mark.parametrize("A", [9, 70])
def test_search_write_on_the_device(backend, A):
    check_write(backend, A)


def test_refusals_on_the_device(backend):
    check_refusals(backend)


@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_sweep_equals_direct_searches_on_the_device(backend, kind):
    cfg, buffer, store, engine, chunk = sweep_case(backend, kind)
    check_sweep(backend, cfg, buffer, store, engine, chunk)


def test_selection_and_errors_on_the_device(backend):
    check_selection_and_errors(backend)


@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_batches_and_sync_on_the_device(backend, kind):
    check_downstream(backend, kind)


def test_worker_on_the_device(backend):
    check_worker(backend)


def test_connect4_games_in_chunks_of_256(backend):
    """24 played connect4 games of 7 .. 42 positions (one of none), their masks from the games, 25 simulations, chunks of
    256 roots: the pool equals the direct searches of every chunk, two runs agree, nothing is skipped."""
    cfg = search_config("connect4", td_steps=42, PER=False, stacked_observations=0)
    rs = numpy.random.RandomState(31)
    limits = [int(v) for v in rs.randint(7, 43, size=24)]
    limits[5] = 0
    buffer, store = played_store(backend, cfg, games.Connect4, limits, 300)
    lengths = [T for _, T in store.games.values()]
    assert lengths[5] == 0 and all(7 <= T <= 42 for T in lengths if T) and sum(lengths) > 256
    engine = engine_for(backend, cfg, 256, 25, weights_seed=5)
    route = (ctypes.c_int32 * 8)()
    backend.lib.check(backend.lib.mzx_search_route(engine.handle(256), ctypes.byref(route)))
    print(f"connect4 reanalyse search: {sum(lengths)} positions, route of 256 trees x 25 simulations: {list(route)}")
    report = check_sweep(backend, cfg, buffer, store, engine, 256)
    print(f"connect4 reanalyse search: {report}, kernel {engine.kernel_name(256)}")
