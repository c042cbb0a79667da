"""
mzx.replay.DeviceGameStore + ReplayBuffer(..., device_store=...): finished games resident in a ragged device pool, the
trainer's batch assembled there by mzx_replay_values / mzx_replay_batch (csrc/mzx_replay.h, csrc/mzx_obs.h).  Here on the
serial build of the same functors (tests/hostcheck); tests/test_gpu_device_replay.py runs the device library.

Every float comparison is by bit pattern (the helpers of tests/test_replay_batch.py): the device path copies frames,
stored binary64 columns and host-drawn actions, and recomputes compute_target_value in the reference's operation order.
"""
import copy
import json
import os

import numpy
import pytest
import torch

import hostcheck
from conftest import GOLDEN
from mzx import replay, self_play
from oracle import ref_shim
from test_replay_batch import CASES, as_arrays, assert_same, config_for, make_games

OBS_SHAPE = (2, 3, 3)       # make_games' default
CHECKPOINT = {"num_played_games": 0, "num_played_steps": 0}


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


def config(per, players, stacked, **overrides):
    cfg = config_for(per, players, stacked)
    cfg.observation_shape = OBS_SHAPE
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def host(batch):
    """A get_batch() result with device tensors -> the dictionary of numpy arrays tests/test_replay_batch.py compares."""
    index_batch, tensors = batch
    return as_arrays((index_batch, tuple(None if t is None else (t.cpu().numpy() if torch.is_tensor(t) else t) for t in tensors)))


def float_obs(arrays):
    """The observation as the trainer sees it: torch.tensor(numpy.array(obs)).float() (trainer.py:146-148)."""
    out = dict(arrays)
    out["obs"] = torch.tensor(numpy.array(arrays["obs"])).float().numpy()
    return out


class StandInStock:
    """
    The storage half of a replay buffer, written for these tests (no reference needed): games under growing ids, eviction
    of the oldest beyond ``replay_buffer_size`` games, the counters, and ``sample_n_games`` -- uniform, or by game priority
    with PER.  ``mzx.replay.ReplayBuffer(..., stock=StandInStock)`` drives it like the reference's class.
    """

    def __init__(self, initial_checkpoint, initial_buffer, config):
        self.config = config
        self.buffer = dict(initial_buffer)
        self.num_played_games = initial_checkpoint["num_played_games"]
        self.num_played_steps = initial_checkpoint["num_played_steps"]
        self.total_samples = sum(len(g.root_values) for g in self.buffer.values())

    def save_game(self, game_history, shared_storage=None):
        self.buffer[self.num_played_games] = game_history
        self.num_played_games += 1
        self.num_played_steps += len(game_history.root_values)
        self.total_samples += len(game_history.root_values)
        if len(self.buffer) > self.config.replay_buffer_size:
            oldest = self.num_played_games - len(self.buffer)
            self.total_samples -= len(self.buffer[oldest].root_values)
            del self.buffer[oldest]

    def update_game_history(self, game_id, game_history):
        if next(iter(self.buffer)) <= game_id:
            self.buffer[game_id] = game_history

    def sample_n_games(self, n_games, force_uniform=False):
        ids = list(self.buffer)
        probs = None
        if self.config.PER and not force_uniform:
            probs = numpy.array([self.buffer[g].game_priority for g in ids], dtype="float32")
            probs /= probs.sum()
        chosen = numpy.random.choice(ids, n_games, p=probs)
        lookup = dict(zip(ids, probs)) if probs is not None else {}
        return [(g, self.buffer[g], lookup.get(g)) for g in chosen]


# ---------------------------------------------------------------------------------------------------- the fixture

@pytest.mark.parametrize("c", range(4))
def test_fixture_batches_from_the_store(backend, c):
    """tests/golden/replay_batch.npz (whole batches the reference produced) from a store holding the fixture's games."""
    z = numpy.load(os.path.join(GOLDEN, "replay_batch.npz"))
    check_fixture_case(backend, z, c)


def check_fixture_case(backend, z, c):
    case = json.loads(str(z["meta"]))["cases"][c]
    cfg = config(case["per"], case["players"], case["stacked"])
    games = make_games(case["games_seed"], case["n_games"], case["players"])
    store = replay.DeviceGameStore(cfg, backend, sum(len(g.root_values) + 1 for g in games))
    store.add_many(list(enumerate(games)))
    U = cfg.num_unroll_steps
    for r in range(case["rounds"]):
        want = {k: z[f"c{c}_r{r}_{k}"] for k in ("index", "obs", "actions", "values", "rewards", "policies", "scales")}
        ids, pos = want["index"][:, 0], want["index"][:, 1]
        length = numpy.array([len(games[g].root_values) for g in ids])
        absorbing = pos[:, None] + numpy.arange(U + 1)[None, :] > length[:, None]
        tape = numpy.where(absorbing, want["actions"], -1)        # only the absorbing steps' draws come from the host
        obs, (values, rewards, policies, actions, scales) = store.batch(list(ids), pos, tape)
        got = dict(index=want["index"], obs=obs.cpu().numpy(), actions=actions.cpu().numpy(), values=values.cpu().numpy(),
                   rewards=rewards.cpu().numpy(), policies=policies.cpu().numpy(), scales=scales.cpu().numpy())
        assert got["obs"].dtype == numpy.float32 and got["values"].dtype == numpy.float64
        assert got["actions"].dtype == numpy.int64 and got["scales"].dtype == numpy.int64
        assert_same(got, float_obs(want), (c, r))


# ---------------------------------------------------------------------------------------------------- the allocator

def game_of(T, seed, A=4, players=1):
    """One game of exactly T positions with make_games' contents."""
    rs = numpy.random.RandomState(seed)
    gh = self_play.GameHistory()
    gh.action_history = [0] + [int(a) for a in rs.randint(0, A, size=T)]
    gh.reward_history = [0] + [float(r) for r in rs.standard_normal(T)]
    gh.to_play_history = [int(i % players) for i in range(T + 1)]
    gh.root_values = [float(v) for v in rs.standard_normal(T)]
    visits = rs.randint(0, 20, size=(T, A)) + 1
    gh.child_visits = [[int(v) / int(row.sum()) for v in row] for row in visits]
    gh.observation_history = [rs.rand(*OBS_SHAPE).astype(numpy.float32) for _ in range(T + 1)]
    return gh


def gather_all(store, game_id, T):
    """Every position of a game (the position past the last search included) as bit patterns."""
    ids, pos = [game_id] * (T + 1), numpy.arange(T + 1)
    tape = numpy.arange((T + 1) * (store.config.num_unroll_steps + 1)).reshape(T + 1, -1) % store.A
    obs, targets = store.batch(ids, pos, tape)
    return [t.cpu().numpy().copy().view(numpy.uint8) for t in (obs,) + targets]


def assert_like_fresh_store(backend, store, game_id, game):
    T = len(game.root_values)
    fresh = replay.DeviceGameStore(store.config, backend, T + 1)
    fresh.add(0, game)
    for a, b in zip(gather_all(store, game_id, T), gather_all(fresh, 0, T)):
        assert numpy.array_equal(a, b), game_id


def test_allocator_wraps_and_releases_oldest_first(backend):
    cfg = config(False, 2, 2)
    store = replay.DeviceGameStore(cfg, backend, 30)
    games = {i: game_of(T, 40 + i, players=2) for i, T in enumerate([9, 9, 7, 5, 11, 3])}
    for i in (0, 1, 2):
        store.add(i, games[i])
    assert store.games == {0: (0, 9), 1: (10, 9), 2: (20, 7)} and len(store) == 3 and 1 in store
    with pytest.raises(replay.StoreFull):         # 2 rows up to the end of the pool, none at the start
        store.add(3, games[3])
    assert store.games == {0: (0, 9), 1: (10, 9), 2: (20, 7)}          # a failed add changes nothing
    store.drop(0)
    store.add(3, games[3])                        # 6 rows: the tail room (2) is too short -> wraps to row 0
    assert store.games[3] == (0, 5)
    with pytest.raises(replay.StoreFull):         # rows 6..9 are free, game 1 (the oldest) still holds 10..19
        store.add(4, games[4])
    store.drop(1)
    store.add(4, games[4])                        # rows 6..17
    assert store.games[4] == (6, 11) and list(store.games) == [2, 3, 4]
    with pytest.raises(replay.StoreFull):
        store.add(5, games[5])                    # 4 rows: only 18..19 free before game 2
    store.drop(2)                                 # the oldest is now game 3 at row 0: everything behind the head is free
    store.add(5, games[5])
    assert store.games[5] == (18, 3)
    for i in (3, 4, 5):
        assert_like_fresh_store(backend, store, i, games[i])
    with pytest.raises(replay.StoreFull):
        replay.DeviceGameStore(cfg, backend, 30).add(0, game_of(30, 1))      # 31 rows never fit
    with pytest.raises(ValueError):
        store.add(5, games[5])                    # already resident


def test_drop_of_a_younger_game_frees_its_rows_once_the_older_ones_left(backend):
    cfg = config(False, 1, 0)
    store = replay.DeviceGameStore(cfg, backend, 20)
    games = [game_of(4, 60 + i) for i in range(5)]
    for i in range(4):
        store.add(i, games[i])                    # rows 0..19
    store.drop(1)
    assert 1 not in store and list(store.games) == [0, 2, 3]
    with pytest.raises(KeyError):
        store.batch([1], [0])
    with pytest.raises(replay.StoreFull):
        store.add(4, games[4])                    # game 0 still pins the tail
    store.drop(0)                                 # tail moves to game 2: rows 0..9 are free
    store.add(4, games[4])
    assert store.games[4] == (0, 4)
    for i in (2, 3, 4):
        assert_like_fresh_store(backend, store, i, games[i])
    with pytest.raises(ValueError):
        store.batch([2], [5])                     # position outside the game


def test_update_changes_exactly_that_games_values(backend):
    cfg = config(True, 2, 1)
    store = replay.DeviceGameStore(cfg, backend, 200)
    games = make_games(31, 6, 2)
    store.add_many(list(enumerate(games)))
    before = {i: gather_all(store, i, len(g.root_values)) for i, g in enumerate(games)}
    values_before = store.values.cpu().numpy().copy()
    target = max(range(6), key=lambda i: len(games[i].root_values))
    T = len(games[target].root_values)
    assert T > cfg.td_steps                       # (some position bootstraps from a root value)
    games[target].reanalysed_predicted_root_values = numpy.random.RandomState(9).standard_normal(T)
    store.update(target, games[target])
    base = store.games[target][0]
    changed = numpy.flatnonzero(store.values.cpu().numpy() != values_before)
    assert changed.size and changed.min() >= base and changed.max() < base + T
    want = replay.n_step_values(games[target], cfg)
    assert numpy.array_equal(store.values.cpu().numpy()[base:base + T].view(numpy.uint64), want.view(numpy.uint64))
    for i, g in enumerate(games):
        if i != target:
            for a, b in zip(gather_all(store, i, len(g.root_values)), before[i]):
                assert numpy.array_equal(a, b)
    assert_like_fresh_store(backend, store, target, games[target])


def test_values_equal_the_host_n_step_values(backend):
    """mzx_replay_values for ragged games (reanalysed ones among them) == n_step_values, binary64 bit patterns."""
    for players in (1, 2):
        cfg = config(True, players, 0)
        games = make_games(70 + players, 12, players)
        store = replay.DeviceGameStore(cfg, backend, 600)
        store.add_many(list(enumerate(games)))
        values = store.values.cpu().numpy()
        for i, g in enumerate(games):
            base, T = store.games[i]
            assert numpy.array_equal(values[base:base + T].view(numpy.uint64), replay.n_step_values(g, cfg).view(numpy.uint64))


def test_random_add_and_evict_gathers_like_a_fresh_store(backend):
    cfg = config(False, 2, 2)
    rs = numpy.random.RandomState(3)
    store = replay.DeviceGameStore(cfg, backend, 90)
    resident, next_id, wrapped = {}, 0, 0
    for step in range(60):
        game = game_of(int(rs.randint(1, 28)), 1000 + step, players=2)
        while True:
            try:
                store.add(next_id, game)
                break
            except replay.StoreFull:
                oldest = next(iter(store.games))
                assert oldest == min(resident)            # eviction order: the oldest game goes first
                store.drop(oldest)
                del resident[oldest]
        wrapped += store.games[next_id][0] == 0 and step > 0
        resident[next_id] = game
        next_id += 1
        spans = sorted((b, b + T + 1) for b, T in store.games.values())
        assert spans[0][0] >= 0 and spans[-1][1] <= store.rows
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))            # no two games share a row
        if step % 7 == 6:
            for game_id, g in resident.items():
                assert_like_fresh_store(backend, store, game_id, g)
    assert wrapped >= 3 and set(store.games) == set(resident)
    for game_id, g in resident.items():
        assert_like_fresh_store(backend, store, game_id, g)


# ---------------------------------------------------------------------------------------------------- the buffer

def buffers(backend, cfg, games, rows, stock=StandInStock, initial=None):
    plain = replay.ReplayBuffer(dict(CHECKPOINT), initial or {}, cfg, stock=stock)
    store = replay.DeviceGameStore(cfg, backend, rows)
    device = replay.ReplayBuffer(dict(CHECKPOINT), initial or {}, cfg, stock=stock, device_store=store)
    for g in games:
        plain.save_game(copy.deepcopy(g))
        device.save_game(copy.deepcopy(g))
    return plain, device, store


@pytest.mark.parametrize("per,players,stacked", CASES)
def test_device_batches_equal_the_host_path(backend, per, players, stacked):
    cfg = config(per, players, stacked)
    plain, device, store = buffers(backend, cfg, make_games(50 + players, 9, players), 400)
    assert device.device_store is store and plain.device_store is None
    for r in range(3):
        numpy.random.seed(200 + r)
        want = plain.get_batch()
        numpy.random.seed(200 + r)
        got = device.get_batch()
        assert isinstance(got[0], list) and got[0] == want[0]
        assert all(torch.is_tensor(t) for t in got[1] if t is not None) and (got[1][5] is None) == (not per)
        assert_same(host(got), float_obs(as_arrays(want)), (per, players, stacked, r))
        if r == 0:      # a reanalysed game: the store's values follow update_game_history
            gid = sorted(plain.buffer)[3]
            fresh = numpy.random.RandomState(5).standard_normal(len(plain.buffer[gid].root_values))
            for rb in (plain, device):
                g2 = copy.deepcopy(rb.buffer[gid])
                g2.reanalysed_predicted_root_values = fresh
                rb.update_game_history(gid, g2)


def test_store_follows_the_stock_eviction_and_an_initial_buffer(backend):
    cfg = config(False, 1, 1, replay_buffer_size=4)
    games = make_games(21, 9, 1)
    initial = {i: g for i, g in enumerate(games[:3])}
    checkpoint = {"num_played_games": 3, "num_played_steps": sum(len(g.root_values) for g in games[:3])}
    store = replay.DeviceGameStore(cfg, backend, 400)
    rb = replay.ReplayBuffer(checkpoint, initial, cfg, stock=StandInStock, device_store=store)
    assert list(store.games) == [0, 1, 2]
    for g in games[3:]:
        rb.save_game(g)
        assert list(store.games) == list(rb.buffer) and len(rb.buffer) <= 4
    assert list(rb.buffer) == [5, 6, 7, 8]
    plain = replay.ReplayBuffer(dict(CHECKPOINT), {i: rb.buffer[i] for i in rb.buffer}, cfg, stock=StandInStock)
    plain.num_played_games = rb.num_played_games
    numpy.random.seed(8)
    want = plain.get_batch()
    numpy.random.seed(8)
    assert_same(host(rb.get_batch()), float_obs(as_arrays(want)), "after eviction")


def test_capacity_bound_in_positions_evicts_from_both(backend):
    """The one deliberate difference: a pool too small for replay_buffer_size games makes the OLDEST games leave the store
    and the stock buffer, total_samples adjusted as the stock eviction does (replay_buffer.py:59-61)."""
    cfg = config(False, 2, 2)           # replay_buffer_size = 10 ** 6: the stock bound never bites
    games = [game_of(T, 80 + i, players=2) for i, T in enumerate([20, 12, 25, 9, 30, 14, 6, 22])]
    rows = 70
    store = replay.DeviceGameStore(cfg, backend, rows)
    rb = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock, device_store=store)
    evicted_early = 0
    for i, g in enumerate(games):
        rb.save_game(g)
        ids = list(rb.buffer)
        assert ids == list(store.games) == list(range(ids[0], i + 1))            # oldest first, both in step
        assert rb.total_samples == sum(len(rb.buffer[j].root_values) for j in ids)
        assert sum(len(rb.buffer[j].root_values) + 1 for j in ids) <= rows
        assert rb.num_played_games == i + 1 and rb.num_played_steps == sum(len(x.root_values) for x in games[:i + 1])
        evicted_early += ids[0] > 0
        numpy.random.seed(i)
        got = rb.get_batch()
        plain = replay.ReplayBuffer(dict(CHECKPOINT), dict(rb.buffer), cfg, stock=StandInStock)
        numpy.random.seed(i)
        assert_same(host(got), float_obs(as_arrays(plain.get_batch())), i)
    assert evicted_early >= 4
    with pytest.raises(replay.StoreFull):
        rb.save_game(game_of(rows, 99, players=2))        # rows + 1 rows: can never be resident
    assert rb.num_played_games == len(games)              # refused before the stock buffer saw it


def test_trainer_tensors_of_a_host_batch_and_a_store_batch_agree(backend):
    for per in (True, False):
        cfg = config(per, 2, 2)
        plain, device, _ = buffers(backend, cfg, make_games(13, 9, 2), 400)
        numpy.random.seed(4)
        want = replay.trainer_tensors(plain.get_batch()[1], "cpu")
        numpy.random.seed(4)
        got = replay.trainer_tensors(device.get_batch()[1], "cpu")
        n, U, A = cfg.batch_size, cfg.num_unroll_steps, len(cfg.action_space)
        shapes = [(n, 2 * 3 + 2, 3, 3), (n, U + 1, 1), (n, U + 1), (n, U + 1), (n, U + 1, A), (n,), (n, U + 1)]
        dtypes = [torch.float32, torch.int64] + [torch.float32] * 5
        assert len(got) == len(want) == 7
        for i, (a, b) in enumerate(zip(got, want)):
            if i == 5 and not per:
                assert a is None and b is None
                continue
            assert a.dtype == b.dtype == dtypes[i] and tuple(a.shape) == tuple(b.shape) == shapes[i], i
            assert torch.equal(a, b), i


def test_abi_argument_checks(backend):
    import ctypes
    from mzx import _lib
    lib = backend.lib
    cfg = config(False, 1, 0)
    store = replay.DeviceGameStore(cfg, backend, 16)
    store.add(0, game_of(5, 1))
    io = _lib.ReplayBatchIO()
    io.num_samples = 1
    assert lib.mzx_replay_batch(None, ctypes.byref(io), None) != 0 and b"null" in lib.mzx_last_error()
    assert lib.mzx_replay_batch(ctypes.byref(store.pool), ctypes.byref(io), None) != 0 and b"sample arrays" in lib.mzx_last_error()
    bad = _lib.ReplayPool.from_buffer_copy(store.pool)
    bad.action_space_size = 0
    assert lib.mzx_replay_batch(ctypes.byref(bad), ctypes.byref(io), None) != 0 and b"action_space_size" in lib.mzx_last_error()
    idx = torch.zeros(4, dtype=torch.int64)
    out = torch.zeros(64, dtype=torch.float32)
    io.d_base, io.d_len, io.d_pos, io.d_observation = idx.data_ptr(), idx.data_ptr(), idx.data_ptr(), out.data_ptr()
    bad = _lib.ReplayPool.from_buffer_copy(store.pool)
    bad.height = 0
    assert lib.mzx_replay_batch(ctypes.byref(bad), ctypes.byref(io), None) != 0 and b"observation shape" in lib.mzx_last_error()
    assert lib.mzx_replay_values(ctypes.byref(store.pool), None, None, 1, 5, None, None) != 0 and b"missing" in lib.mzx_last_error()
    assert lib.mzx_replay_values(ctypes.byref(store.pool), None, None, -1, 5, None, None) != 0
    assert lib.mzx_replay_values(ctypes.byref(store.pool), None, None, 0, 5, None, None) == 0


# ---------------------------------------------------------------------------------------------------- the reference

def evict_like(theirs, ours):
    """The store's capacity bound applied to the reference buffer: its own eviction statements (replay_buffer.py:59-61)."""
    while len(theirs.buffer) > len(ours.buffer):
        del_id = theirs.num_played_games - len(theirs.buffer)
        theirs.total_samples -= len(theirs.buffer[del_id].root_values)
        del theirs.buffer[del_id]
    assert list(theirs.buffer) == list(ours.buffer)


@pytest.mark.reference
@pytest.mark.parametrize("rows", [400, 120])
@pytest.mark.parametrize("per,players,stacked", CASES)
def test_store_batches_identical_to_the_reference(backend, per, players, stacked, rows):
    """Side by side with the unmodified reference buffer, with the feedback of test_batches_identical_to_the_reference;
    rows = 120 holds fewer positions than the nine games have: the store evicts before the stock bound would."""
    ref_shim.load()
    import replay_buffer as ref_rb
    cfg = config(per, players, stacked)
    games = make_games(11 + players, 9, players)
    theirs = ref_rb.ReplayBuffer(dict(CHECKPOINT), {}, cfg)
    store = replay.DeviceGameStore(cfg, backend, rows)
    ours = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, device_store=store)
    for gh in games:
        theirs.save_game(copy.deepcopy(gh))
        ours.save_game(copy.deepcopy(gh))
        evict_like(theirs, ours)
    assert (len(ours.buffer) < len(games)) == (rows == 120)
    assert ours.total_samples == theirs.total_samples and ours.num_played_steps == theirs.num_played_steps
    for rounds in range(4):
        numpy.random.seed(100 + rounds)
        want = float_obs(as_arrays(theirs.get_batch()))
        numpy.random.seed(100 + rounds)
        got = host(ours.get_batch())
        assert_same(got, want, (per, players, stacked, rounds))
        if per:
            pr = numpy.abs(numpy.random.RandomState(rounds).standard_normal((cfg.batch_size, cfg.num_unroll_steps + 1))).astype("float32")
            theirs.update_priorities(pr, want["index"].tolist())
            ours.update_priorities(pr, got["index"].tolist())
        if rounds == 1:
            gid, gh, _ = theirs.sample_game(force_uniform=True)
            fresh = numpy.random.RandomState(5).standard_normal(len(gh.root_values)).astype(numpy.float32).astype(numpy.float64)
            for rb in (theirs, ours):
                g2 = copy.deepcopy(rb.buffer[gid])
                g2.reanalysed_predicted_root_values = fresh
                rb.update_game_history(gid, g2)
        if rounds == 2:       # more games arrive: eviction while batches are being drawn
            for gh in make_games(90, 3, players):
                theirs.save_game(copy.deepcopy(gh))
                ours.save_game(copy.deepcopy(gh))
                evict_like(theirs, ours)


@pytest.mark.reference
def test_reanalyse_from_the_store_equals_the_upload_path(backend):
    from mzx import configs, models, synthetic
    _, ref_self_play = ref_shim.load()
    cfg = configs.tictactoe(stacked_observations=2, td_steps=4, discount=0.997, num_unroll_steps=5)    # (the replay fields)
    rs = numpy.random.RandomState(17)
    A = len(cfg.action_space)
    histories = []
    for T in (7, 9, 4):
        gh = ref_self_play.GameHistory()                    # the reference's own object
        gh.observation_history = [rs.randint(-1, 2, size=cfg.observation_shape).astype("int32") for _ in range(T + 1)]
        gh.action_history = [0] + [int(a) for a in rs.randint(0, A, size=T)]
        gh.reward_history = [0] + [float(r) for r in rs.standard_normal(T)]
        gh.to_play_history = [i % 2 for i in range(T + 1)]
        gh.root_values = [float(v) for v in rs.standard_normal(T)]
        gh.child_visits = [[1 / A] * A for _ in range(T)]
        histories.append(gh)
    store = replay.DeviceGameStore(cfg, backend, 40)
    store.add_many([(5 + i, gh) for i, gh in enumerate(histories)])
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 3)
    checkpoint = {"weights": weights, "num_reanalysed_games": 0}
    plain = replay.Reanalyse(checkpoint, cfg, _backend=backend)
    resident = replay.Reanalyse(checkpoint, cfg, _backend=backend, device_store=store)
    from mzx import observations
    for i, gh in enumerate(histories):
        T = len(gh.root_values)
        want_obs = observations.stack_history(backend, cfg, gh.observation_history, gh.action_history, count=T)
        assert torch.equal(store.stacked(5 + i), want_obs)
        want, got = plain.reanalyse_game(gh), resident.reanalyse_game(gh, 5 + i)
        assert got.dtype == want.dtype == numpy.float32 and got.shape == want.shape == (T,)
        assert numpy.array_equal(got.view(numpy.uint32), want.view(numpy.uint32))
        assert numpy.array_equal(resident.reanalyse_game(gh, 99).view(numpy.uint32), want.view(numpy.uint32))   # not resident: upload
