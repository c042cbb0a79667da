"""
The reanalyse sweep of the device-resident replay store on the MI355X (libmzx.so): the check functions of
tests/test_reanalyse_sweep.py on the device library, plus a connect4-sized buffer whose chunks are large enough for the
network engine to leave the small-batch route.  Bitwise where both sides ran the same batch; the decoded-scalar gate of
tests/test_gpu_parity.py (3e-4) where the batches differ.
"""
import numpy
import pytest

from mzx import _lib, configs, models, replay, synthetic
from test_device_replay import CHECKPOINT
from test_reanalyse_sweep import (GATE, KINDS, SamplingStock, bits, check_downstream, check_mixed_chunks, check_positions,
                                  check_same_batch, check_worker, check_worker_without_the_flag, check_write_back, history)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def test_positions_on_the_device(backend):
    check_positions(backend)


def test_write_back_on_the_device(backend):
    check_write_back(backend)


@pytest.mark.parametrize("kind", KINDS)
def test_one_game_per_chunk_on_the_device(backend, kind):
    check_same_batch(backend, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_chunks_straddling_games_on_the_device(backend, kind):
    check_mixed_chunks(backend, kind, exact=False)      # (prints the largest difference; asserts the gate)


@pytest.mark.parametrize("kind,chunk", [("fc", 7), ("resnet", 50)])
def test_targets_and_batches_on_the_device(backend, kind, chunk):
    check_downstream(backend, kind, chunk)


@pytest.mark.parametrize("kind", KINDS)
def test_worker_on_the_device(backend, kind):
    check_worker(backend, kind)


def test_loop_without_the_flag_on_the_device(backend):
    check_worker_without_the_flag(backend)


def test_connect4_buffer_in_large_chunks(backend):
    """96 connect4 games of 7 .. 42 positions (one of none): the default chunk takes them in ONE network batch, 1000
    positions take three; both agree with the per-game path within the gate, each is deterministic, and the pool ends
    as update_game_history leaves it for the sweep's own arrays."""
    cfg = configs.connect4(td_steps=42, num_unroll_steps=5, PER=False, batch_size=64, replay_buffer_size=10 ** 6)
    rs = numpy.random.RandomState(12)
    lengths = [int(T) for T in rs.randint(7, 43, size=96)]
    lengths[17] = 0
    games = [history(cfg, T, 900 + i) for i, T in enumerate(lengths)]
    store = replay.DeviceGameStore(cfg, backend, sum(lengths) + len(lengths))
    buffer = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=SamplingStock, device_store=store)
    for g in games:
        buffer.save_game(g)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 5)
    worker = replay.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, cfg, _backend=backend, device_store=store)
    want = {g: worker.reanalyse_game(gh, g).reshape(-1) for g, gh in buffer.buffer.items()}
    assert store.reanalyse_chunk_positions() > sum(lengths) > 2000
    worst = 0.0
    for chunk in (None, 1000):
        got = store.reanalyse(worker.model, chunk_positions=chunk)
        again = store.reanalyse(worker.model, chunk_positions=chunk)
        for g, T in enumerate(lengths):
            assert got[g].shape == (T,) and numpy.array_equal(bits(got[g]), bits(again[g]))
            if T:
                worst = max(worst, float(numpy.abs(got[g] - want[g]).max()))
            assert numpy.allclose(got[g], want[g], atol=GATE, rtol=GATE), (chunk, g)
        root_values, values = store.root_values.cpu().numpy(), store.values.cpu().numpy()
        for g, gh in buffer.buffer.items():
            base, T = store.games[g]
            gh.reanalysed_predicted_root_values = got[g]
            assert numpy.array_equal(bits(root_values[base:base + T]), bits(got[g].astype(numpy.float64)))
            assert numpy.array_equal(bits(values[base:base + T]), bits(replay.n_step_values(gh, cfg)))
    print(f"connect4 sweep vs per-game path: largest difference {worst:.3e} (gate {GATE:g})")
