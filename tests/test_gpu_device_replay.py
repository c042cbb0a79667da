"""
The device-resident replay store on the MI355X (libmzx.so): mzx_replay_values / mzx_replay_batch against the reference's
fixture batches and against the host get_batch path, bit for bit.  No reference tree is needed: the stock buffer is the
stand-in of tests/test_device_replay.py.
"""
import os
import types

import numpy
import pytest
import torch

from conftest import GOLDEN
from mzx import _lib, replay, self_play
from test_device_replay import CHECKPOINT, StandInStock, check_fixture_case, float_obs, host
from test_replay_batch import as_arrays, assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.mark.parametrize("c", range(4))
def test_fixture_batches_on_the_device(backend, c):
    check_fixture_case(backend, numpy.load(os.path.join(GOLDEN, "replay_batch.npz")), c)


def shaped_config(shape, stacked, A, per, batch_size):
    return types.SimpleNamespace(PER=per, PER_alpha=0.5, seed=7, replay_buffer_size=10 ** 6, batch_size=batch_size,
                                 num_unroll_steps=5, td_steps=6, discount=0.997, stacked_observations=stacked,
                                 observation_shape=shape, action_space=list(range(A)), players=[0, 1])


def shaped_games(shape, A, lengths, seed, dtype):
    rs = numpy.random.RandomState(seed)
    games = []
    for T in lengths:
        gh = self_play.GameHistory()
        gh.action_history = [0] + [int(a) for a in rs.randint(0, A, size=T)]
        gh.reward_history = [0] + [float(r) for r in rs.standard_normal(T)]
        gh.to_play_history = [i % 2 for i in range(T + 1)]
        gh.root_values = [float(v) for v in rs.standard_normal(T)]
        visits = rs.randint(0, 20, size=(T, A)) + 1
        gh.child_visits = [[int(v) / int(row.sum()) for v in row] for row in visits]
        frames = rs.rand(T + 1, *shape) * 255
        gh.observation_history = [f.astype(dtype) for f in frames]
        games.append(gh)
    return games


def check_against_the_host_path(backend, cfg, games, rows, rounds):
    plain = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock)
    store = replay.DeviceGameStore(cfg, backend, rows)
    device = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock, device_store=store)
    for g in games:
        plain.save_game(g)
        device.save_game(g)
    assert list(store.games) == list(device.buffer)
    for r in range(rounds):
        numpy.random.seed(300 + r)
        want = plain.get_batch()
        numpy.random.seed(300 + r)
        got = device.get_batch()
        assert got[0] == want[0] and got[1][0].device == store.frames.device and got[1][0].dtype == torch.float32
        assert_same(host(got), float_obs(as_arrays(want)), r)
    # positions at both ends of every resident game: the first moves (planes before the game are zeros), the last searched
    # position and the one past it (every unroll step absorbing but the first)
    A, k, U = len(cfg.action_space), cfg.stacked_observations, cfg.num_unroll_steps
    ids, pos = [], []
    for game_id, gh in device.buffer.items():
        T = len(gh.root_values)
        for p in sorted({0, 1, min(k, T), T - 1, T}):
            ids.append(game_id)
            pos.append(p)
    tape = numpy.random.RandomState(1).randint(0, A, size=(len(ids), U + 1))
    obs, targets = store.batch(ids, pos, tape)
    values, rewards, policies, actions, scales = (t.cpu() for t in targets)
    want_obs = numpy.array([device.buffer[g].get_stacked_observations(p, k, A) for g, p in zip(ids, pos)])
    assert torch.equal(obs.cpu(), torch.tensor(want_obs).float())
    for n, (g, p) in enumerate(zip(ids, pos)):
        gh = device.buffer[g]
        T = len(gh.root_values)
        nstep = replay.n_step_values(gh, cfg)
        for u in range(U + 1):
            i = p + u
            assert values[n, u].item() == (nstep[i] if i < T else 0.0)
            assert rewards[n, u].item() == (gh.reward_history[i] if i <= T else 0.0)
            assert policies[n, u].tolist() == (gh.child_visits[i] if i < T else [1 / A] * A)
            assert actions[n, u].item() == (gh.action_history[i] if i <= T else tape[n, u])
            assert scales[n, u].item() == min(U, T + 1 - p)


def test_atari_shaped_batches_equal_the_host_path(backend):
    """games/atari.py's geometry: 3 x 96 x 96 frames, 32 stacked observations -> 131 planes, the 16-byte path."""
    cfg = shaped_config((3, 96, 96), 32, 4, True, 12)
    games = shaped_games(cfg.observation_shape, 4, [37, 5, 14], 2, numpy.float32)
    check_against_the_host_path(backend, cfg, games, 80, 2)


def test_gomoku_shaped_batches_equal_the_host_path(backend):
    """11 x 11 planes: H * W is not a multiple of 4, the scalar path; integer boards, 121 actions, no PER."""
    cfg = shaped_config((3, 11, 11), 3, 121, False, 32)
    games = shaped_games(cfg.observation_shape, 121, [9, 30, 2, 17], 4, numpy.int32)
    check_against_the_host_path(backend, cfg, games, 70, 2)


def test_pool_reuse_after_eviction_on_the_device(backend):
    """Rows released by evicted games are overwritten by later ones while batches keep being drawn."""
    cfg = shaped_config((2, 8, 8), 4, 6, False, 16)
    games = shaped_games(cfg.observation_shape, 6, [12, 9, 15, 7, 11, 14, 5, 13], 6, numpy.float32)
    store = replay.DeviceGameStore(cfg, backend, 40)
    device = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock, device_store=store)
    for i, g in enumerate(games):
        device.save_game(g)
        assert list(store.games) == list(device.buffer)
        plain = replay.ReplayBuffer(dict(CHECKPOINT), dict(device.buffer), cfg, stock=StandInStock)
        numpy.random.seed(i)
        want = plain.get_batch()
        numpy.random.seed(i)
        assert_same(host(device.get_batch()), float_obs(as_arrays(want)), i)
    assert min(device.buffer) > 0
