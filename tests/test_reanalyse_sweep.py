"""
The reanalyse sweep of the device-resident replay store: mzx_replay_positions / mzx_replay_reanalyse_write
(csrc/mzx_replay.h), DeviceGameStore.reanalyse and Reanalyse.reanalyse_store (mzx/replay.py).  Here on the serial build of
the same functors (tests/hostcheck); tests/test_gpu_reanalyse_sweep.py runs the check functions of this file on the device
library.

The comparisons are against paths the suite already pins to the reference: Reanalyse.reanalyse_game +
update_game_history (tests/test_observations.py, tests/test_device_replay.py), n_step_values and the host get_batch
(tests/test_replay_batch.py).  Floats are compared by bit pattern wherever both sides ran the same network batch; where the
batch differs (chunks that straddle games against one game per batch) the network engine may take another route, and with
it another summation order, so the gate is the decoded-scalar tolerance of tests/test_gpu_parity.py: 3e-4 absolute +
relative (the inverse value transform cancels ~3 digits of logits that agree to 1e-6).

Every case uses the same buffer: ragged games, one of T == 0, one that already carries reanalysed values, in a pool so
small that the allocation has wrapped; chunks of 7 and 50 positions divide no game length and not the total either.
"""
import copy

import numpy
import pytest
import torch

import hostcheck
from mzx import configs, models, replay, self_play, synthetic
from test_device_replay import CHECKPOINT, StandInStock, float_obs, host
from test_replay_batch import as_arrays, assert_same

GATE = 3e-4                                   # tests/test_gpu_parity.py:86-90
LENGTHS = [25, 9, 0, 13, 5, 11, 20, 1]        # the first game leaves when the seventh needs its rows
ROWS = 80
CHUNKS = (7, 50)
KINDS = ("fc", "resnet")


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


class SamplingStock(StandInStock):
    """The stand-in stock buffer; games without a position are never drawn (sample_position has nothing to draw from)."""

    def sample_n_games(self, n_games, force_uniform=False):
        ids = [g for g in self.buffer if len(self.buffer[g].root_values)]
        probs = None
        if self.config.PER and not force_uniform:
            probs = numpy.array([self.buffer[g].game_priority for g in ids], dtype="float32")
            probs /= probs.sum()
        chosen = numpy.random.choice(ids, n_games, p=probs)
        lookup = dict(zip(ids, probs)) if probs is not None else {}
        return [(g, self.buffer[g], lookup.get(g)) for g in chosen]


def sweep_config(kind, **overrides):
    replay_fields = dict(td_steps=4, num_unroll_steps=5, PER=True, PER_alpha=0.5, batch_size=16, replay_buffer_size=10 ** 6,
                         stacked_observations=2)
    replay_fields.update(overrides)
    if kind == "fc":
        return configs.cartpole(**replay_fields)
    return configs.tictactoe(discount=0.997, **replay_fields)


def history(cfg, T, seed):
    rs = numpy.random.RandomState(seed)
    A, players = len(cfg.action_space), len(cfg.players)
    gh = self_play.GameHistory()
    if cfg.network == "resnet":
        gh.observation_history = [rs.randint(-1, 2, size=cfg.observation_shape).astype("int32") for _ in range(T + 1)]
    else:
        gh.observation_history = [rs.standard_normal(cfg.observation_shape).astype("float32") for _ in range(T + 1)]
    gh.action_history = [0] + [int(a) for a in rs.randint(0, A, size=T)]
    gh.reward_history = [0] + [float(r) for r in rs.standard_normal(T)]
    gh.to_play_history = [i % players for i in range(T + 1)]
    gh.root_values = [float(v) for v in rs.standard_normal(T)]
    visits = rs.randint(0, 20, size=(T, A)) + 1
    gh.child_visits = [[int(v) / int(row.sum()) for v in row] for row in visits]
    return gh


def build(backend, kind, **overrides):
    """(config, buffer with a device store, the store, a Reanalyse worker reading from the store) holding the games above."""
    cfg = sweep_config(kind, **overrides)
    games = [history(cfg, T, 500 + i) for i, T in enumerate(LENGTHS)]
    games[3].reanalysed_predicted_root_values = numpy.random.RandomState(3).standard_normal(LENGTHS[3]).astype(numpy.float32)
    store = replay.DeviceGameStore(cfg, backend, ROWS)
    buffer = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=SamplingStock, device_store=store)
    for g in games:
        buffer.save_game(g)
    assert list(store.games) == list(buffer.buffer) == list(range(1, len(LENGTHS)))      # game 0 made room ...
    assert store.games[6][0] < store.games[1][0]                                          # ... and the allocation wrapped
    lengths = [T for _, T in store.games.values()]
    assert 0 in lengths and all(T % c for T in lengths if T for c in CHUNKS) and all(sum(lengths) % c for c in CHUNKS)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 3)
    worker = replay.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, cfg, _backend=backend, device_store=store)
    return cfg, buffer, store, worker


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({4: numpy.uint32, 8: numpy.uint64}[a.dtype.itemsize])


def per_game_path(backend, kind, **overrides):
    """The same buffer refreshed by the existing loop body: reanalyse_game + update_game_history, game by game."""
    cfg, buffer, store, worker = build(backend, kind, **overrides)
    values = {}
    for game_id, gh in list(buffer.buffer.items()):
        values[game_id] = gh.reanalysed_predicted_root_values = worker.reanalyse_game(gh, game_id).reshape(-1)
        buffer.update_game_history(game_id, gh)
    return cfg, buffer, store, values


# ---------------------------------------------------------------------------------------------------- 1. enumeration

def positions(backend, base, length, lo, count):
    lib = backend.lib
    first = numpy.concatenate([[0], numpy.cumsum(length)[:-1]]).astype(numpy.int64)
    up = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(backend.device)
    d = [up(base.astype(numpy.int64)), up(length.astype(numpy.int32)), up(first)]
    out = [backend.empty((max(count, 1),), t) for t in (torch.int64, torch.int32, torch.int32)]
    rc = lib.mzx_replay_positions(*(backend.ptr(t) for t in d), len(base), int(length.sum()), lo, count,
                                  *(backend.ptr(t) for t in out), backend.stream())
    return rc, [t.cpu().numpy()[:max(count, 0)] for t in out]


def check_positions(backend):
    rs = numpy.random.RandomState(1)
    for trial in range(12):
        G = int(rs.randint(1, 40))
        length = rs.randint(0, 30, size=G)
        length[rs.randint(0, G)] = 0
        if trial % 3 == 0:
            length[0] = 0
        if trial % 4 == 0:
            length[-1] = 0
        if length.sum() == 0:
            length[G // 2] = 17
        base = rs.permutation(G).astype(numpy.int64) * 64 + 5
        total = int(length.sum())
        want = (numpy.repeat(base, length), numpy.repeat(length, length),
                numpy.concatenate([numpy.arange(T) for T in length]))
        assert want[0].size == total
        mid = int(rs.randint(0, total))
        for lo, count in ((0, min(7, total)), (mid, min(50, total - mid)), (max(0, total - 9), min(9, total)), (0, total),
                          (total, 0)):
            rc, got = positions(backend, base, length, lo, count)
            assert rc == 0, backend.lib.mzx_last_error()
            for g, w in zip(got, want):
                assert numpy.array_equal(g, w[lo:lo + count]), (trial, lo, count)
            assert (got[1] > 0).all()                  # games of T == 0 contribute no element
        for lo, count in ((0, total + 1), (total, 1), (total - 3, 4), (-1, 2), (0, -1)):
            rc, _ = positions(backend, base, length, lo, count)
            assert rc == -1 and b"mzx_replay_positions" in backend.lib.mzx_last_error(), (lo, count)       # MZX_ERR_INVALID
    lib = backend.lib
    assert lib.mzx_replay_positions(None, None, None, 3, 10, 0, 4, None, None, None, None) == -1 and b"missing" in lib.mzx_last_error()
    assert lib.mzx_replay_positions(None, None, None, -1, 10, 0, 4, None, None, None, None) == -1
    assert lib.mzx_replay_positions(None, None, None, 3, 10, 0, 0, None, None, None, None) == 0


def test_positions_equal_repeat_and_arange(backend):
    check_positions(backend)


# ---------------------------------------------------------------------------------------------------- 2. write-back

def check_write_back(backend):
    cfg, buffer, store, worker = build(backend, "fc", support_size=7)
    lib, S = backend.lib, 7
    selection = [2, 4, 7, 3]                                   # (a T == 0 game among them; not in allocation order)
    entries = [store.games[g] for g in selection]
    base = numpy.array([b for b, _ in entries])
    length = numpy.array([T for _, T in entries])
    n = int(length.sum())
    rc, (s_base, s_len, s_pos) = positions(backend, base, length, 0, n)
    assert rc == 0
    logits = torch.from_numpy((numpy.random.RandomState(8).standard_normal((n, 2 * S + 1)) * 3).astype(numpy.float32)).to(backend.device)
    want = models.support_to_scalar(logits, S, _backend=backend).cpu().numpy().reshape(n)
    before = store.root_values.cpu().numpy().copy()
    others = {name: getattr(store, name).cpu().numpy().copy() for name in ("frames", "actions", "rewards", "to_play", "child_visits", "values")}
    d_base, d_pos = (torch.from_numpy(a).to(backend.device) for a in (s_base, s_pos))
    out = backend.zeros((n,), torch.float32)
    lib.check(lib.mzx_replay_reanalyse_write(backend.ptr(logits), n, S, backend.ptr(d_base), backend.ptr(d_pos), backend.ptr(out),
                                             backend.ptr(store.root_values), backend.stream()))
    got = out.cpu().numpy()
    assert numpy.array_equal(bits(got), bits(want))                                 # mzx_support_to_scalar's bits
    after = store.root_values.cpu().numpy()
    rows = s_base + s_pos
    assert numpy.unique(rows).size == n
    assert numpy.array_equal(bits(after[rows]), bits(got.astype(numpy.float64)))   # float64(float32), bit for bit
    untouched = numpy.ones(store.rows, bool)
    untouched[rows] = False
    assert numpy.array_equal(bits(after[untouched]), bits(before[untouched]))      # other games, every padding row
    for b, T in store.games.values():
        assert untouched[b + T]
    for name, column in others.items():
        assert numpy.array_equal(getattr(store, name).cpu().numpy(), column), name
    # argument checks
    assert lib.mzx_replay_reanalyse_write(None, 4, S, None, None, None, None, None) == -1 and b"missing" in lib.mzx_last_error()
    assert lib.mzx_replay_reanalyse_write(backend.ptr(logits), -1, S, backend.ptr(d_base), backend.ptr(d_pos), backend.ptr(out),
                                          backend.ptr(store.root_values), None) == -1
    assert lib.mzx_replay_reanalyse_write(backend.ptr(logits), 4, -1, backend.ptr(d_base), backend.ptr(d_pos), backend.ptr(out),
                                          backend.ptr(store.root_values), None) == -1 and b"negative" in lib.mzx_last_error()
    assert lib.mzx_replay_reanalyse_write(None, 0, S, None, None, None, None, None) == 0


def test_write_back_bit_for_bit(backend):
    check_write_back(backend)


# ---------------------------------------------------------------------------------------------------- 3. same batch

def check_same_batch(backend, kind):
    cfg, buffer, store, worker = build(backend, kind)
    _, buffer2, store2, _ = build(backend, kind)
    assert store.games == store2.games
    for game_id, gh in buffer.buffer.items():
        T = len(gh.root_values)
        want = worker.reanalyse_game(gh, game_id).reshape(-1)
        got = store.reanalyse(worker.model, [game_id], chunk_positions=T)
        assert list(got) == [game_id] and got[game_id].dtype == numpy.float32 and got[game_id].shape == (T,)
        assert numpy.array_equal(bits(got[game_id]), bits(want)), (kind, game_id)
        gh2 = buffer2.buffer[game_id]
        gh2.reanalysed_predicted_root_values = want
        buffer2.update_game_history(game_id, gh2)
    for name in ("root_values", "values"):
        assert numpy.array_equal(bits(getattr(store, name).cpu().numpy()), bits(getattr(store2, name).cpu().numpy())), (kind, name)


@pytest.mark.parametrize("kind", KINDS)
def test_one_game_per_chunk_equals_reanalyse_game(backend, kind):
    check_same_batch(backend, kind)


# ---------------------------------------------------------------------------------------------------- 4. mixed chunks

def check_mixed_chunks(backend, kind, exact):
    """Returns the largest |sweep - per-game| seen.  ``exact``: the two paths must agree bit for bit (the serial build,
    whose network arithmetic does not depend on the batch)."""
    cfg, buffer, store, worker = build(backend, kind)
    _, _, store2, want = per_game_path(backend, kind)
    worst = 0.0
    for chunk in CHUNKS + (None,):
        first = store.reanalyse(worker.model, chunk_positions=chunk)
        columns = [store.root_values.cpu().numpy().copy(), store.values.cpu().numpy().copy()]
        again = store.reanalyse(worker.model, chunk_positions=chunk)
        assert list(first) == list(again) == list(store.games)
        for game_id, (_, T) in store.games.items():
            a, b = first[game_id], again[game_id]
            assert a.dtype == numpy.float32 and a.shape == (T,)
            assert numpy.array_equal(bits(a), bits(b)), (kind, chunk, game_id)            # deterministic
            diff = float(numpy.abs(a - want[game_id]).max()) if T else 0.0
            worst = max(worst, diff)
            assert numpy.allclose(a, want[game_id], atol=GATE, rtol=GATE), (kind, chunk, game_id, diff)
            if exact:
                assert numpy.array_equal(bits(a), bits(want[game_id])), (kind, chunk, game_id, diff)
        assert numpy.array_equal(bits(columns[0]), bits(store.root_values.cpu().numpy()))
        assert numpy.array_equal(bits(columns[1]), bits(store.values.cpu().numpy()))
        if exact:
            assert numpy.array_equal(bits(columns[0]), bits(store2.root_values.cpu().numpy()))
            assert numpy.array_equal(bits(columns[1]), bits(store2.values.cpu().numpy()))
    print(f"reanalyse sweep vs per-game path ({kind}): largest difference {worst:.3e} (gate {GATE:g})")
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_chunks_straddling_games(backend, kind):
    """On the serial build the sweep and the per-game path agree BIT FOR BIT (observed: largest difference 0 for both
    networks -- its network operators compute a sample independently of the batch it sits in), so that is asserted."""
    assert check_mixed_chunks(backend, kind, exact=True) == 0.0


# ---------------------------------------------------------------------------------------------------- 5. downstream targets

def check_downstream(backend, kind, chunk):
    cfg, buffer, store, worker = build(backend, kind)
    before = {name: getattr(store, name).cpu().numpy().copy() for name in ("frames", "actions", "rewards", "to_play", "child_visits")}
    swept = store.reanalyse(worker.model, chunk_positions=chunk)
    for name, column in before.items():
        assert numpy.array_equal(getattr(store, name).cpu().numpy(), column), name          # no other column is touched
    values = store.values.cpu().numpy()
    plain_games = {}
    for game_id, gh in buffer.buffer.items():
        g2 = copy.deepcopy(gh)
        g2.reanalysed_predicted_root_values = swept[game_id]
        plain_games[game_id] = g2
        base, T = store.games[game_id]
        assert numpy.array_equal(bits(values[base:base + T]), bits(replay.n_step_values(g2, cfg))), (kind, game_id)
    checkpoint = {"num_played_games": buffer.num_played_games, "num_played_steps": buffer.num_played_steps}
    plain = replay.ReplayBuffer(checkpoint, plain_games, cfg, stock=SamplingStock)
    assert plain.total_samples == buffer.total_samples
    for r in range(3):
        numpy.random.seed(40 + r)
        want = plain.get_batch()
        numpy.random.seed(40 + r)
        got = buffer.get_batch()
        assert got[0] == want[0]
        assert_same(host(got), float_obs(as_arrays(want)), (kind, r))


@pytest.mark.parametrize("kind,chunk", [("fc", 7), ("resnet", 50)])
def test_targets_and_batches_after_a_sweep(backend, kind, chunk):
    check_downstream(backend, kind, chunk)


def test_selection_and_errors(backend):
    cfg, buffer, store, worker = build(backend, "fc")
    assert store.reanalyse(worker.model, []) == {}
    with pytest.raises(KeyError):
        store.reanalyse(worker.model, [1, 99])
    with pytest.raises(ValueError):
        store.reanalyse(worker.model, chunk_positions=0)
    empty = store.reanalyse(worker.model, [2])                # the game of T == 0
    assert list(empty) == [2] and empty[2].shape == (0,) and empty[2].dtype == numpy.float32
    before = store.root_values.cpu().numpy().copy()
    some = store.reanalyse(worker.model, [6, 4, 6], chunk_positions=7)
    assert list(some) == [6, 4]
    after = store.root_values.cpu().numpy()
    rows = numpy.zeros(store.rows, bool)
    for g in (6, 4):
        b, T = store.games[g]
        rows[b:b + T] = True
        assert numpy.array_equal(bits(after[b:b + T]), bits(some[g].astype(numpy.float64)))
    assert numpy.array_equal(bits(after[~rows]), bits(before[~rows]))
    # the default chunk: the byte budget, within one gather launch
    sample_bytes = 4 * int(numpy.prod(store.sample_shape))
    assert store.reanalyse_chunk_positions() == min(replay.REANALYSE_CHUNK_BYTES // sample_bytes, store.reanalyse_chunk_limit())
    big = replay.DeviceGameStore(configs.atari(td_steps=10), backend, 4)
    assert big.sample_shape == (131, 96, 96) and big.reanalyse_chunk_positions() == replay.REANALYSE_CHUNK_BYTES // (4 * 131 * 96 * 96)
    assert big.reanalyse_chunk_limit() * 131 * 36 < replay.REPLAY_GATHER_GROUPS


# ---------------------------------------------------------------------------------------------------- 6. the worker

class Storage:
    """shared_storage of one loop iteration (tests/test_observations.py check_reanalyse)."""

    def __init__(self, weights, training_steps):
        self.passes, self.steps = 0, training_steps
        self.info = {"num_played_games": 1, "terminate": False, "weights": weights}

    def get_info(self, key):
        if key == "training_step":
            self.passes += 1
            return 0 if self.passes == 1 else self.steps
        return self.info[key]

    def set_info(self, key, value=None):
        self.info[key] = value


class RecordingBuffer:
    """A buffer that is not an in-process mzx.replay.ReplayBuffer (a stand-in for an actor handle): records its calls."""

    def __init__(self, game_history):
        self.calls, self.game_history = [], game_history

    def sample_game(self, force_uniform=False):
        self.calls.append(("sample_game", force_uniform))
        return 7, self.game_history, 1.0

    def update_game_history(self, game_id, game_history):
        self.calls.append(("update_game_history", game_id, game_history))


def check_worker(backend, kind):
    cfg, buffer, store, worker = build(backend, kind, reanalyse_sweep=True)
    weights = synthetic.fill_state_dict(worker.model.state_dict(), 21)          # the loop must pull these
    _, _, _, want = per_game_path(backend, kind)
    reference = replay.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, cfg, _backend=backend)
    for game_id in (4, 5):                   # cached host arrays (what make_target keeps per game): must be dropped
        buffer._game_arrays(game_id, buffer.buffer[game_id])
    cached = set(buffer._arrays)
    assert cached == {4, 5}
    worker.num_reanalysed_games = 3
    storage = Storage(weights, cfg.training_steps)
    worker.reanalyse(buffer, storage)
    n = len(store.games)
    assert worker.num_reanalysed_games == 3 + n and storage.info["num_reanalysed_games"] == 3 + n
    assert not cached & set(buffer._arrays)
    for game_id, gh in buffer.buffer.items():
        got = gh.reanalysed_predicted_root_values
        T = len(gh.root_values)
        assert isinstance(got, numpy.ndarray) and got.dtype == numpy.float32 and got.shape == (T,)
        single = reference.reanalyse_game(gh).reshape(-1)                     # the upload path under the pulled weights
        assert numpy.allclose(got, single, atol=GATE, rtol=GATE), (kind, game_id)
        if T:
            assert not numpy.array_equal(got, want[game_id])                  # (not the initial weights' values)
    # an evicted game still listed in the store is passed over, not resurrected
    gone = next(iter(buffer.buffer))
    del buffer._stock.buffer[gone]
    assert gone in store
    assert worker.reanalyse_store(buffer) == n - 1 and gone not in buffer.buffer
    assert worker.num_reanalysed_games == 3 + 2 * n - 1
    assert worker.reanalyse_store(buffer, [gone, 5]) == 1
    with pytest.raises(KeyError):
        worker.reanalyse_store(buffer, [99])
    # device pointers do not cross processes; a buffer without a store has nothing to sweep
    with pytest.raises(ValueError):
        worker.reanalyse_store(RecordingBuffer(None))
    with pytest.raises(ValueError):
        worker.reanalyse_store(replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=SamplingStock))


@pytest.mark.parametrize("kind", KINDS)
def test_worker_sweeps_the_store(backend, kind):
    check_worker(backend, kind)


def check_worker_without_the_flag(backend):
    for flag, gate in ((None, True), (False, True), (True, True), (True, False)):
        overrides = {} if flag is None else {"reanalyse_sweep": flag}
        cfg, buffer, store, worker = build(backend, "fc", use_last_model_value=gate, **overrides)
        gh = history(cfg, 6, 77)
        weights = worker.model.get_weights()
        # anything but an in-process buffer with a store takes the existing calls, whatever the flag says
        recording = RecordingBuffer(gh)
        worker.reanalyse(recording, Storage(weights, cfg.training_steps))
        assert recording.calls == [("sample_game", True), ("update_game_history", 7, gh)]
        assert worker.num_reanalysed_games == 1
        assert (gh.reanalysed_predicted_root_values is not None) == gate
        if flag and gate:
            continue
        # a buffer with a store, but no flag (or the gate closed): one drawn game through update_game_history
        calls = []
        stock = buffer._stock
        update = stock.update_game_history

        def sample_game(force_uniform=False):
            calls.append(("sample_game", force_uniform))
            return 5, stock.buffer[5], None

        def update_game_history(game_id, game_history):
            calls.append(("update_game_history", game_id))
            return update(game_id, game_history)

        stock.sample_game, stock.update_game_history = sample_game, update_game_history
        touched = {g: h.reanalysed_predicted_root_values for g, h in buffer.buffer.items()}
        worker.reanalyse(buffer, Storage(weights, cfg.training_steps))
        assert calls == [("sample_game", True), ("update_game_history", 5)] and worker.num_reanalysed_games == 2
        for g, h in buffer.buffer.items():
            if g != 5 or not gate:
                assert h.reanalysed_predicted_root_values is touched[g]


def test_loop_without_the_flag_is_the_existing_one(backend):
    check_worker_without_the_flag(backend)
