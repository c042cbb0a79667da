"""
Bulk ingest of a shard's finished games into the device replay store (mzx_replay_ingest, csrc/mzx_replay.h;
DeviceGameStore.add_records, ReplayBuffer.save_games): the check functions.  tests/test_replay_ingest.py runs them on the
serial build (tests/hostcheck), tests/test_gpu_replay_ingest.py on the device library.

The reference of every comparison is the per-game path as it stands: a second store fed the same games, materialised, one
``add_many`` per game.  Records are built from seeded numpy arrays, twice from the same seed -- one copy stays a set of
fresh views for the bulk path, the other is pickled into plain materialised histories (pickling a view materialises it, so
the two must not share objects).  Everything is compared as raw bytes.
"""
import copy
import ctypes
import pickle

import numpy
import pytest
import torch

from mzx import _lib, configs, games, models, replay, self_play, synthetic, trainer
from mzx.history import ShardGameHistory, ShardGames, _ShardRecord
from test_device_replay import CHECKPOINT
from test_reanalyse_sweep import history
from replay_sampler_cases import FeedbackStock
import trainer_loss_cases

TD_STEPS = 4
# (k games, T): only the padding row; one position; a few; past one lane stride of the values kernel and past td_steps;
# shorter than td_steps (no bootstrap term)
LENGTHS = [(2, 0), (3, 1), (3, 5), (1, 65), (2, 3)]
# name -> (observation shape, actions, players, legal masks, int8 observations and int64 rewards)
GEOMETRIES = {
    "cartpole": ((1, 1, 4), 2, 1, False, False),
    "odd-frame": ((3, 3, 3), 7, 2, True, True),          # 27 floats: the dword path of the frame copy; illegal actions
    "connect4": ((3, 6, 7), 33, 2, True, False),         # two mask words, the last one bit wide
    "wide": ((1, 1, 4), 70, 1, False, False),            # more actions than lanes
    "long-frame": ((1, 8, 40), 2, 1, False, False),      # 320 floats: 80 groups of 16 bytes, more than one per lane
}
COLUMNS = ("frames", "actions", "rewards", "to_play", "root_values", "child_visits", "values")
SLOT_COLUMNS = ("slot_game", "slot_base", "slot_len", "slot_priority", "slot_sum")


def ingest_config(geometry="cartpole", per=True, alpha=0.5, **overrides):
    shape, A, players, _, _ = GEOMETRIES[geometry]
    fields = dict(td_steps=TD_STEPS, num_unroll_steps=5, PER=per, PER_alpha=alpha, batch_size=16, replay_buffer_size=10 ** 6,
                  stacked_observations=2, seed=7)
    fields.update(overrides)
    cfg = configs.cartpole(**fields)
    cfg.observation_shape, cfg.action_space, cfg.players = shape, list(range(A)), list(range(players))
    return cfg


def make_record(cfg, rs, k, T, masked=False, integer=False):
    """A ``_ShardRecord`` of k games of T positions as ``native_rounds.collect`` builds one.  ``masked``: illegal actions (a
    nonzero count only on legal ones) and, every few rows, a root without a visit (no legal action, total == 0)."""
    shape, A, P = tuple(cfg.observation_shape), len(cfg.action_space), len(cfg.players)
    if integer:
        obs = rs.randint(-1, 2, size=(k, T + 1) + shape).astype(numpy.int8)
        rews = rs.randint(-2, 3, size=(k, T + 1)).astype(numpy.int64)
    else:
        obs = rs.standard_normal((k, T + 1) + shape).astype(numpy.float32)
        rews = rs.standard_normal((k, T + 1))
    rews[:, 0] = 0
    acts = numpy.concatenate([numpy.zeros((k, 1), numpy.int64), rs.randint(0, A, size=(k, T)).astype(numpy.int64)], 1)
    tps = ((numpy.arange(T + 1)[None, :] + numpy.arange(k)[:, None]) % P).astype(numpy.int64)      # two players taking turns
    vis = (rs.randint(0, 20, size=(k, T, A)) + 1).astype(numpy.int32)
    legal = None
    if masked:
        legal = rs.random_sample((k, T, A)) < 0.6
        legal[:, :, 0] = True
        if k > 1:
            legal[0] = True                       # one game whose rows are all legal: the record's own rows serve it
        legal.reshape(-1, A)[2::5] = False        # roots without a visit
        vis = vis * legal
    vals = rs.standard_normal((k, T))
    totals = vis.sum(2).astype(numpy.int64)
    ratios = vis / numpy.maximum(totals, 1)[:, :, None]
    plain = totals > 0
    if legal is not None:
        plain = plain & legal.all(2)
    return _ShardRecord(A, obs, acts, rews, tps, vis, vals, totals, ratios, plain.all(1), legal)


def make_handoff(cfg, backend, geometry, seed, priorities, lengths=LENGTHS):
    """``ShardGames`` of fresh views over records of the given lengths, in finishing order: records interleaved, one record
    handed over in reverse and one short of a game (the gather path), the others whole and in order (the arrays as they
    lie).  ``priorities``: the records carry theirs (``device_priorities``, what ``collect(priorities_for=...)`` does)."""
    _, _, _, masked, integer = GEOMETRIES[geometry]
    rs = numpy.random.RandomState(seed)
    records, keyed = [], []
    for r, (k, T) in enumerate(lengths):
        record = make_record(cfg, rs, k, T, masked, integer)
        if priorities and cfg.PER and T:
            record.priorities, record.game_priority = replay.device_priorities(
                backend, numpy.where(record.totals > 0, record.vals, 0.0), record.tps, record.rews, cfg)
        views = ShardGameHistory.make_many(record, k, T)
        members = views[::-1] if r == 1 else (views[:-1] if r == 2 else views)
        records.append((record, T, views))
        keyed += [(j, r, h) for j, h in enumerate(members)]
    out = ShardGames([h for _, _, h in sorted(keyed, key=lambda e: e[:2])])
    out.records = records
    return out


def twins_of(cfg, backend, geometry, seed, lengths=LENGTHS):
    """The same hand-off as plain materialised histories that carry their priorities: what the per-game path takes."""
    return pickle.loads(pickle.dumps(list(make_handoff(cfg, backend, geometry, seed, True, lengths))))


def new_store(cfg, backend, rows=400, max_games=64, legal_masks=True):
    return replay.DeviceGameStore(cfg, backend, rows, max_games=max_games, legal_masks=legal_masks)


def host(t):
    return t.detach().cpu().numpy()


def snapshot(store):
    """Every column and dictionary of a store, as host copies."""
    if store.sampler is not None:
        store._flush_slots()
    names = COLUMNS + (("legal_mask",) if store.legal_mask is not None else ())
    if store.sampler is not None:
        names += ("priorities", "owner") + SLOT_COLUMNS
    out = {name: host(getattr(store, name)).copy() for name in names}
    out["games"] = list(store.games.items())
    out["head"], out["with_positions"] = store._head, store._with_positions
    if store.sampler is not None:
        out["slot_owner"] = dict(store._slot_owner)
    return out


def assert_unchanged(store, before):
    after = snapshot(store)
    assert after.keys() == before.keys()
    for name, want in before.items():
        got = after[name]
        assert (got.tobytes() == want.tobytes()) if isinstance(want, numpy.ndarray) else got == want, name


def assert_same_pool(ours, theirs, same_rows=True, emptied=False):
    """The two stores hold the same games in the same order with the same bytes in every column, on the occupied rows
    including each game's padding row; with ``same_rows`` at the same bases, and the slot table alike.  ``emptied``: games
    that only the per-game path uploaded have left again -- their slots are empty in both tables (game -1, base 0, length
    0), and the maximum / sum such a slot keeps, which nothing reads, is not compared."""
    assert list(ours.games) == list(theirs.games)
    assert [T for _, T in ours.games.values()] == [T for _, T in theirs.games.values()]
    assert ours._with_positions == theirs._with_positions
    if same_rows:
        assert list(ours.games.items()) == list(theirs.games.items()) and ours._head == theirs._head
    a, b = snapshot(ours), snapshot(theirs)
    names = [n for n in a if isinstance(a[n], numpy.ndarray) and n not in SLOT_COLUMNS and n != "owner"]
    for g, (base, T) in ours.games.items():
        other = theirs.games[g][0]
        for name in names:
            # (no path writes the padding row of the derived ``values``: it is compared where the rows are the same rows with
            # the same past -- not where only the per-game path had an evicted game on them)
            n = T if name == "values" and (emptied or not same_rows) else T + 1
            assert a[name][base:base + n].tobytes() == b[name][other:other + n].tobytes(), (name, g, T)
    if ours.sampler is not None:
        assert ours._slot_owner == theirs._slot_owner
        assert a["slot_game"].tobytes() == b["slot_game"].tobytes() and a["owner"].tobytes() == b["owner"].tobytes()
        live = a["slot_game"] >= 0         # (a slot that was emptied keeps its last base / length / priority / sum: never followed)
        for name in SLOT_COLUMNS:
            if same_rows and not (emptied and name in ("slot_priority", "slot_sum")):
                assert a[name].tobytes() == b[name].tobytes(), name
            elif same_rows or name != "slot_base":
                assert a[name][live].tobytes() == b[name][live].tobytes(), name


def per_game(store, ids, twins):
    for g, gh in zip(ids, twins):
        store.add_many([(g, gh)])


# ------------------------------------------------------------------------------------------------ columns, priorities

def check_columns(backend, geometry, per, staged, alpha=0.5, max_games=64, legal_masks=True):
    cfg = ingest_config(geometry, per, alpha)
    out = make_handoff(cfg, backend, geometry, 11, staged)
    twins = twins_of(cfg, backend, geometry, 11)
    ids = [3 + 2 * i for i in range(len(out))]                   # ids with gaps: empty slots in between
    ours, theirs = (new_store(cfg, backend, max_games=max_games, legal_masks=legal_masks) for _ in range(2))
    ours.add_records(list(zip(ids, out)), out.records)
    assert ours.ingest_calls == 1                                # one upload + one library call for the whole hand-off
    assert all(len(h.__dict__) <= 4 and "_view" in h.__dict__ for h in out)      # nothing materialised on the way
    per_game(theirs, ids, twins)
    assert_same_pool(ours, theirs)
    if per and max_games and not staged:
        # the kernel's priorities are device_priorities of the same record, bit for bit; the host views stay without
        assert all(h.priorities is None for h in out)
        column = host(ours.priorities)
        for record, T, views in out.records:
            if T:
                want, top = replay.device_priorities(backend, numpy.where(record.totals > 0, record.vals, 0.0), record.tps,
                                                     record.rews, cfg)
                for h in out:
                    if h.__dict__["_view"][0] is record:
                        row = h.__dict__["_view"][1]
                        g = ids[[id(x) for x in out].index(id(h))]
                        base = ours.games[g][0]
                        assert column[base:base + T].tobytes() == want[row].tobytes()
                        assert ours.priorities_of(g)[1].tobytes() == numpy.float32(top[row]).tobytes()


# ------------------------------------------------------------------------------------------------ allocation

def check_wrap(backend):
    """A hand-off that wraps the circular pool: its games form two runs of rows."""
    cfg = ingest_config("odd-frame")
    out, twins = make_handoff(cfg, backend, "odd-frame", 5, True), twins_of(cfg, backend, "odd-frame", 5)
    # residents on rows 0 .. 112; the two oldest leave: free rows 113 .. 124 (room for the first three games of the
    # hand-off, not for the game of 65 positions) and 0 .. 101
    stores = [new_store(cfg, backend, rows=125) for _ in range(2)]
    first = [history(cfg, T, 40 + i) for i, T in enumerate((70, 30, 10))]
    for gh in first:
        replay.fill_initial_priorities(gh, cfg)
    for store in stores:
        store.add_many([(i, copy.deepcopy(gh)) for i, gh in enumerate(first)])
        store.drop(0)
        store.drop(1)
    ids = list(range(3, 3 + len(out)))
    stores[0].add_records(list(zip(ids, out)), out.records)
    per_game(stores[1], ids, twins)
    bases = [stores[0].games[g][0] for g in ids]
    assert any(b < a for a, b in zip(bases, bases[1:]))          # the allocation wrapped inside the hand-off
    assert_same_pool(stores[0], stores[1])


def check_store_full(backend):
    cfg = ingest_config("cartpole")
    out = make_handoff(cfg, backend, "cartpole", 6, True)
    store = new_store(cfg, backend, rows=60, max_games=64)       # the hand-off needs ~100 rows
    store.add_many([(0, history_with_priorities(cfg, 4, 1))])
    before = snapshot(store)
    with pytest.raises(replay.StoreFull):
        store.add_records(list(zip(range(1, 1 + len(out)), out)), out.records)
    assert_unchanged(store, before)
    assert store.ingest_calls == 0
    # a slot held by a resident game
    store = new_store(cfg, backend, rows=400, max_games=8)
    store.add_many([(3, history_with_priorities(cfg, 4, 1))])
    before = snapshot(store)
    with pytest.raises(replay.StoreFull):
        store.add_records([(8 + i, h) for i, h in enumerate(out[:5])], out.records)        # game 11 takes slot 3
    assert_unchanged(store, before)
    with pytest.raises(ValueError):
        store.add_records([(3, out[0])], out.records)             # already resident
    assert_unchanged(store, before)


def history_with_priorities(cfg, T, seed):
    gh = history(cfg, T, seed)
    replay.fill_initial_priorities(gh, cfg)
    return gh


def check_chunks(backend, geometry="odd-frame"):
    """A forced chunk size small enough for at least three upload + ingest pairs: the same pool."""
    cfg = ingest_config(geometry)
    ids = None
    stores = []
    for chunk_bytes in (None, 3000, 1):
        out = make_handoff(cfg, backend, geometry, 12, True)
        ids = list(range(len(out)))
        store = new_store(cfg, backend)
        store.add_records(list(zip(ids, out)), out.records, chunk_bytes=chunk_bytes)
        stores.append(store)
    assert stores[0].ingest_calls == 1 and stores[1].ingest_calls >= 3 and stores[2].ingest_calls == len(ids)
    assert_same_pool(stores[1], stores[0])
    assert_same_pool(stores[2], stores[0])


# ------------------------------------------------------------------------------------------------ mixed hand-off

def check_mixed(backend):
    """Views with a materialised or an assigned field and a plain GameHistory among fresh views: runs of either kind in
    hand-off order, order and bases as add_many of the whole list gives."""
    cfg = ingest_config("odd-frame")
    handoff, twins = make_handoff(cfg, backend, "odd-frame", 13, True), twins_of(cfg, backend, "odd-frame", 13)
    out, records = list(handoff), handoff.records
    out[1].root_values, out[2].child_visits                       # materialised
    out[6].reward_history = list(out[6].reward_history)          # assigned
    plain = history_with_priorities(cfg, 7, 99)
    out.insert(4, plain)
    twins.insert(4, copy.deepcopy(plain))
    ids = list(range(len(out)))
    ours, theirs = new_store(cfg, backend), new_store(cfg, backend)
    ours.add_records(list(zip(ids, out)), records)
    theirs.add_many(list(zip(ids, twins)))
    assert ours.ingest_calls == 4                                # the runs of fresh views between the other games
    assert_same_pool(ours, theirs)


# ------------------------------------------------------------------------------------------------ downstream

def check_downstream(backend, per=True):
    geometry = "odd-frame"
    cfg = ingest_config(geometry, per)
    out, twins = make_handoff(cfg, backend, geometry, 14, True), twins_of(cfg, backend, geometry, 14)
    ids = list(range(len(out)))
    ours, theirs = new_store(cfg, backend), new_store(cfg, backend)
    ours.add_records(list(zip(ids, out)), out.records)
    per_game(theirs, ids, twins)
    total, U, n = sum(T for _, T in ours.games.values()), cfg.num_unroll_steps, 24
    drawn = [store.sample(n, cfg.seed, 3, total, per, U) for store in (ours, theirs)]
    for a, b in zip(*drawn):
        assert (a is None and b is None) or host(a).tobytes() == host(b).tobytes()
    batches = [store.gather(*d[:4], U) for store, d in zip((ours, theirs), drawn)]
    assert host(batches[0][0]).tobytes() == host(batches[1][0]).tobytes()
    for a, b in zip(batches[0][1], batches[1][1]):
        assert host(a).tobytes() == host(b).tobytes()
    if per:
        fresh = numpy.random.RandomState(2).random_sample((n, U + 1)).astype(numpy.float32)
        for store, d in zip((ours, theirs), drawn):
            store.update_priorities(fresh, d[4], d[2])
        for g in ids:
            (pa, ta), (pb, tb) = ours.priorities_of(g), theirs.priorities_of(g)
            assert pa.tobytes() == pb.tobytes() and ta.tobytes() == tb.tobytes()
    # the search inputs of a game with illegal actions
    g = max(ids, key=lambda g: ours.games[g][1])
    results = []
    for store in (ours, theirs):
        base, T = store.games[g]
        sb, sp = store._up(numpy.full(T, base, numpy.int64)), store._up(numpy.arange(T, dtype=numpy.int32))
        to_play, flags = backend.empty((T,), torch.int32), backend.empty((T,), torch.int32)
        legal, tape = backend.empty((T, store.A), torch.int32), backend.empty((T, 8), torch.int32)
        backend.lib.check(backend.lib.mzx_replay_search_inputs(
            ctypes.byref(store.pool), backend.ptr(store.legal_mask), backend.ptr(sb), backend.ptr(sp), T, 8, 5, 0, 0,
            backend.ptr(to_play), backend.ptr(legal), backend.ptr(tape), backend.ptr(flags), backend.stream()))
        results.append([host(t).copy() for t in (to_play, legal, tape, flags)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*results))
    assert (results[0][1] == -1).any() and (results[0][3] == 1).any()      # illegal actions, and a root without any


# ------------------------------------------------------------------------------------------------ save_games

def buffers(cfg, backend, rows, max_games=64, store=True):
    out = []
    for _ in range(2):
        s = new_store(cfg, backend, rows=rows, max_games=max_games) if store else None
        out.append(replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=FeedbackStock, device_store=s))
    return out


def assert_same_buffers(ours, theirs, emptied=False):
    assert list(ours.buffer) == list(theirs.buffer)
    for name in ("num_played_games", "num_played_steps", "total_samples"):
        assert getattr(ours, name) == getattr(theirs, name), name
    for g in ours.buffer:
        a, b = ours.buffer[g], theirs.buffer[g]
        assert len(a.root_values) == len(b.root_values)
        if ours.config.PER and len(a.root_values):
            assert numpy.asarray(a.priorities).tobytes() == numpy.asarray(b.priorities).tobytes()
    if ours.device_store is not None:
        assert_same_pool(ours.device_store, theirs.device_store, emptied=emptied)


class Counters:
    def __init__(self):
        self.calls = []

    def set_info(self, key, value):
        self.calls.append((key, value))


def check_save_games(backend, situation):
    """``save_games`` against a loop of ``save_game``, each on its own buffer and store: the same stock buffer, counters,
    residency, bases and pool contents."""
    geometry = "odd-frame"
    lengths, max_games = LENGTHS, 64
    if situation == "size-eviction":        # replay_buffer_size evicts games of the hand-off inside the hand-off
        cfg, rows = ingest_config(geometry, replay_buffer_size=5), 400
    elif situation in ("position-eviction", "mixed"):     # the pool is too small for the residents plus the hand-off
        cfg, rows = ingest_config(geometry), 120      # 38 rows of residents + 94 of the hand-off: the oldest resident leaves
    elif situation == "slot-eviction":      # four slots: every game has to wait for the game four ids before it to leave
        cfg, rows, max_games = ingest_config(geometry), 400, 4
    elif situation == "oversized":          # a single game larger than the pool
        cfg, rows, lengths = ingest_config(geometry), 40, [(1, 65)]
    else:
        cfg, rows = ingest_config(geometry), 400
    store = situation != "no-store"
    ours, theirs = buffers(cfg, backend, rows, max_games=max_games, store=store)
    residents = [history_with_priorities(cfg, T, 70 + i) for i, T in enumerate((12, 9, 14))]
    if situation != "oversized":
        for gh in residents:
            ours.save_game(copy.deepcopy(gh))
            theirs.save_game(copy.deepcopy(gh))
    out, twins = make_handoff(cfg, backend, geometry, 15, True, lengths), twins_of(cfg, backend, geometry, 15, lengths)
    if situation == "plain-list":
        out = list(out)
    if situation == "mixed":                # two games that are no fresh views any more: the per-game path in their turn
        out[2].root_values, out[7].child_visits
    if situation == "oversized":
        state = snapshot(ours.device_store)
        for buffer, games_ in ((ours, out), (theirs, twins)):
            with pytest.raises(replay.StoreFull):
                buffer.save_games(games_) if buffer is ours else buffer.save_game(games_[0])
            assert not buffer.buffer and buffer.num_played_games == 0 and buffer.total_samples == 0
        assert_unchanged(ours.device_store, state)
        return
    storage = Counters()
    ours.save_games(out, storage)
    for gh in twins:
        theirs.save_game(gh)
    if store and situation != "plain-list":       # the two counters, published once
        assert storage.calls == [("num_played_games", theirs.num_played_games), ("num_played_steps", theirs.num_played_steps)]
        # one upload + ingest for the hand-off; in the mixed one, one per run of fresh views (before, between, behind)
        assert ours.device_store.ingest_calls == (3 if situation == "mixed" else 1)
    if situation == "size-eviction":
        assert len(ours.buffer) == 5 and min(ours.buffer) > 3
    if situation == "position-eviction":
        assert list(ours.buffer) == list(range(1, 3 + len(out)))      # the oldest resident left, the hand-off stayed
    if situation == "slot-eviction":
        assert list(ours.buffer) == list(range(len(out) - 1, 3 + len(out)))
    assert_same_buffers(ours, theirs, emptied=situation in ("size-eviction", "slot-eviction"))


def check_handoff_eviction(backend, rows, order):
    """The position bound evicts games of the hand-off itself: an empty pool of 10 to 12 rows takes games of 3, 3 and 5
    positions (4 + 4 + 6 rows).  The loop places every game at the running head: in the order 3, 3, 5 the third game finds
    no room behind the first two, both leave and it lands on row 0; in the order 3, 5, 3 the third game evicts the first
    and takes its rows.  ``save_games`` ends in the same state -- and uploads only the games that stayed."""
    geometry = "odd-frame"
    cfg, lengths = ingest_config(geometry), [(2, 3), (1, 5)]
    ours, theirs = buffers(cfg, backend, rows)
    handoff, twins = make_handoff(cfg, backend, geometry, 16, True, lengths), twins_of(cfg, backend, geometry, 16, lengths)
    assert [len(h.root_values) for h in twins] == [3, 5, 3]
    out = ShardGames([handoff[i] for i in order])
    out.records = handoff.records
    twins = [twins[i] for i in order]
    ours.save_games(out)
    for gh in twins:
        theirs.save_game(gh)
    if order == (0, 2, 1):                # 3, 3, 5
        assert list(theirs.buffer) == [2] and theirs.total_samples == 5 and theirs.device_store.games == {2: (0, 5)}
    else:                                 # 3, 5, 3
        assert list(theirs.buffer) == [1, 2] and theirs.total_samples == 8 and theirs.device_store.games == {1: (4, 5), 2: (0, 3)}
    assert ours.device_store.ingest_calls == 1
    assert_same_buffers(ours, theirs, emptied=True)


# ------------------------------------------------------------------------------------------------ the frame copy

def check_frame_paths(backend):
    """The two paths of the frame copy on one geometry whose rows are whole 16-byte groups (320 floats: 80 groups, more
    than one per lane): staged observations on a 16-byte boundary take the vector path, the same observations 4 bytes
    further the dword path.  Both must land the same frames, and nothing outside the game's rows."""
    lib = backend.lib
    cfg = ingest_config("long-frame")
    F, A, T = 320, 2, 3
    frames = numpy.random.RandomState(21).standard_normal((T + 1, F)).astype(numpy.float32)
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(backend.device)
    staged = dict(d_len=dev(numpy.array([T], numpy.int32)), d_base=dev(numpy.array([2], numpy.int64)),
                  d_game_id=dev(numpy.array([1], numpy.int64)), d_src1=dev(numpy.zeros(1, numpy.int64)),
                  d_src0=dev(numpy.zeros(1, numpy.int64)), d_actions=dev(numpy.ones(T + 1, numpy.int64)),
                  d_rewards=dev(numpy.ones(T + 1, numpy.float64)), d_to_play=dev(numpy.zeros(T + 1, numpy.int64)),
                  d_visits=dev(numpy.ones((T, A), numpy.int32)), d_root_values=dev(numpy.ones(T, numpy.float64)))
    for offset in (4, 5):                 # floats into the block: 16 bytes (the vector path), 20 bytes (the dword path)
        block = dev(numpy.concatenate([numpy.zeros(offset, numpy.float32), frames.reshape(-1)]))
        assert block.data_ptr() % 16 == 0
        store = new_store(cfg, backend, rows=8, max_games=4, legal_masks=False)
        store.frames.fill_(77)
        assert store.frames.data_ptr() % 16 == 0
        x = _lib.ReplayIngestIO()
        for k, v in staged.items():
            setattr(x, k, v.data_ptr())
        x.d_observations, x.d_discount_pow = block.data_ptr() + 4 * offset, store._discount_pow.data_ptr()
        x.per_alpha, x.total_rows, x.num_games, x.td_steps, x.per, x.action_space_size = 0.5, T + 1, 1, TD_STEPS, 1, A
        x.channels, x.height, x.width = store.shape
        assert lib.mzx_replay_ingest(ctypes.byref(store.pool), ctypes.byref(store.sampler), None, 0, ctypes.byref(x),
                                     backend.stream()) == 0
        got = host(store.frames).reshape(8, F)
        assert got[2:2 + T + 1].tobytes() == frames.tobytes(), offset
        assert (got[:2] == 77).all() and (got[2 + T + 1:] == 77).all()


# ------------------------------------------------------------------------------------------------ the ABI

def check_abi_refusals(backend):
    """Every refusal of include/mzx.h: MZX_ERR_INVALID with a message and a canary-filled pool untouched; G == 0 succeeds
    and launches nothing; the accepted call writes."""
    lib = backend.lib
    cfg = ingest_config("odd-frame")
    store = new_store(cfg, backend, rows=16, max_games=4)
    for name in COLUMNS + ("legal_mask", "priorities"):
        getattr(store, name).fill_(77)
    F, A, T = 27, store.A, 2
    dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(backend.device)
    staged = dict(d_len=dev(numpy.array([T], numpy.int32)), d_base=dev(numpy.array([1], numpy.int64)),
                  d_game_id=dev(numpy.array([2], numpy.int64)), d_src1=dev(numpy.zeros(1, numpy.int64)),
                  d_src0=dev(numpy.zeros(1, numpy.int64)), d_observations=dev(numpy.ones((T + 1, F), numpy.float32)),
                  d_actions=dev(numpy.ones(T + 1, numpy.int64)), d_rewards=dev(numpy.ones(T + 1, numpy.float64)),
                  d_to_play=dev(numpy.ones(T + 1, numpy.int64)), d_visits=dev(numpy.ones((T, A), numpy.int32)),
                  d_root_values=dev(numpy.ones(T, numpy.float64)), d_discount_pow=store._discount_pow)

    def io(**fields):
        x = _lib.ReplayIngestIO()
        for k, v in staged.items():
            setattr(x, k, v.data_ptr())
        x.per_alpha, x.total_rows, x.num_games, x.td_steps, x.per, x.action_space_size = 0.5, T + 1, 1, TD_STEPS, 1, A
        x.channels, x.height, x.width = store.shape
        for k, v in fields.items():
            setattr(x, k, v)
        return x

    def call(pool=store.pool, sampler=store.sampler, mask=store.legal_mask, mask_rows=store.rows, **fields):
        return lib.mzx_replay_ingest(None if pool is None else ctypes.byref(pool), None if sampler is None else ctypes.byref(sampler),
                                     backend.ptr(mask), mask_rows, ctypes.byref(io(**fields)), backend.stream())

    before = snapshot(store)

    def refused(rc, word):
        assert rc == -1 and word in lib.mzx_last_error().decode(), (rc, lib.mzx_last_error())
        assert_unchanged(store, before)

    refused(call(pool=None), "null")
    refused(lib.mzx_replay_ingest(ctypes.byref(store.pool), None, None, 0, None, backend.stream()), "null")
    for name in staged:
        refused(call(**{name: None}), "missing")
    refused(call(num_games=-1), "negative")
    refused(call(action_space_size=A + 1), "actions")
    refused(call(width=store.shape[2] + 1), "frames")
    refused(call(channels=store.shape[0] + 1), "frames")
    short = _lib.ReplaySampler.from_buffer_copy(store.sampler)
    short.rows = store.rows - 1
    refused(call(sampler=short), "sampler")
    refused(call(mask_rows=store.rows - 1), "mask")
    bare = _lib.ReplayPool.from_buffer_copy(store.pool)
    bare.d_child_visits = None
    refused(call(pool=bare), "pool column")
    assert call(num_games=0, total_rows=0) == 0
    assert_unchanged(store, before)
    assert call() == 0
    assert host(store.actions)[1:4].tolist() == [1, 1, 1] and host(store.actions)[0] == 77 and host(store.actions)[4] == 77
    assert host(store.slot_game)[2] == 2 and host(store.slot_len)[2] == T
    # without a sampler and without a mask column: the optional pointers NULL
    assert call(sampler=None, mask=None, mask_rows=0, d_base=dev(numpy.array([6], numpy.int64)).data_ptr()) == 0
    assert host(store.actions)[6:9].tolist() == [1, 1, 1] and host(store.priorities)[6] == 77


# ------------------------------------------------------------------------------------------------ end to end

def check_end_to_end(backend):
    """A natively played tic-tac-toe shard of 8 games: play_rounds' output through save_games, the same games, materialised,
    through the per-game loop -- the same pool, and one train_step on each buffer returns the same four losses."""
    games.NativeBatchedGame.backend = backend

    def play():
        cfg = configs.tictactoe(num_simulations=5, td_steps=4, num_unroll_steps=3, batch_size=16, PER=True, PER_alpha=0.5, seed=7)
        cfg.reanalyse_search = True               # the shard records its legal masks
        cfg.value_loss_weight, cfg.replay_buffer_size = 0.25, 10 ** 6
        weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 3)
        shard = self_play.SelfPlay({"weights": weights}, games.TicTacToeNative, cfg, 9, num_games=8, _backend=backend)
        out = shard.play_rounds(1.0, None, min_games=8)
        shard.close_game()
        return cfg, out

    cfg, out = play()
    _, again = play()
    assert isinstance(out, ShardGames) and out.records and len(out) >= 8
    assert any(record.legal_mask is not None for record, _, _ in out.records)
    twins = pickle.loads(pickle.dumps(list(again)))
    rows = sum(len(h.root_values) + 1 for h in twins) + 8
    built = []
    for _ in range(2):
        store = replay.DeviceGameStore(cfg, backend, rows, max_games=64, legal_masks=True)
        built.append(replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=FeedbackStock, device_store=store, device_sampler=True))
    ours, theirs = built
    ours.save_games(out)
    for gh in twins:
        theirs.save_game(gh)
    assert ours.device_store.ingest_calls == 1
    assert_same_buffers(ours, theirs)
    torch.manual_seed(5)
    width = int(numpy.prod(ours.device_store.sample_shape))
    model = trainer_loss_cases.TinyModel(width, 8, cfg.support_size, len(cfg.action_space)).to(backend.device)
    twin = trainer_loss_cases.TinyModel(width, 8, cfg.support_size, len(cfg.action_space)).to(backend.device)
    twin.load_state_dict(model.state_dict())
    opt, opt_twin = torch.optim.SGD(model.parameters(), lr=0.05), torch.optim.SGD(twin.parameters(), lr=0.05)
    a = trainer.train_step(model, opt, ours, cfg, backend=backend)
    b = trainer.train_step(twin, opt_twin, theirs, cfg, backend=backend)
    assert a.shape == (4,) and host(a).tobytes() == host(b).tobytes()
    assert_same_pool(ours.device_store, theirs.device_store)         # the priority feedback landed alike
