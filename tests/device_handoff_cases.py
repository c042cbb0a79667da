"""
The device hand-off of resident self-play games into the device replay store (config.device_handoff; csrc/mzx_resident.h
ResidentPackBody, mzx_actor_take_device / mzx_actor_release_device, ReplayBuffer.save_games) and reading games back from
the store (mzx_replay_export, csrc/mzx_replay.h; DeviceGameStore.download_games): the check functions.
tests/test_device_handoff.py runs them on the serial build (tests/hostcheck), tests/test_gpu_device_handoff.py on the
device library.  First the export alone, then (second half) the hand-off against a twin shard that goes through the host.

The export is the inverse of the bulk ingest, so the games come from ``replay_ingest_cases.make_handoff`` (its LENGTHS: a
game of no position, of one, and of 65 -- more packed rows than a wavefront has lanes) and go in through ``add_records``.
The reference is a numpy restatement of the packed layout built from ``snapshot(store)``: plain ``.cpu()`` reads of the
pool's columns, independent of the kernel.  Everything is compared as raw bytes.
"""
import copy
import ctypes

import numpy
import pytest
import torch

import resident_rounds_cases as rr
from mzx import _lib, configs, games, models, replay, self_play, shared_storage
from mzx.history import ShardGames, _PieceRecord
from replay_ingest_cases import GEOMETRIES, assert_same_pool, host, ingest_config, make_handoff, new_store, snapshot
from replay_sampler_cases import FeedbackStock
from test_device_replay import CHECKPOINT
from test_selfplay_refill import _same

WHOLE = ("observations", "actions", "rewards", "to_play")                  # T + 1 entries per game
SEARCHED = ("child_visits", "root_values", "legal_mask", "priorities")    # T entries per game
CANARY = 77


def filled_store(backend, geometry, per=True, max_games=64, legal_masks=True, rows=400):
    """A store holding the hand-off of ``replay_ingest_cases`` under ids with gaps, and its snapshot."""
    cfg = ingest_config(geometry, per)
    out = make_handoff(cfg, backend, geometry, 31, True)
    store = new_store(cfg, backend, rows=rows, max_games=max_games, legal_masks=legal_masks)
    ids = [3 + 2 * i for i in range(len(out))]
    store.add_records(list(zip(ids, out)), out.records)
    return store, ids, snapshot(store)


def restated(store, snap, ids, legal_mask, priorities):
    """The packed arrays of the games ``ids`` as include/mzx.h states them, from the host copies of the pool's columns."""
    A = store.A
    cols = {name: [] for name in WHOLE + SEARCHED}
    for g in ids:
        base, T = store.games[g]
        rows = slice(base, base + T + 1)
        cols["observations"].append(snap["frames"][rows])
        cols["actions"].append(snap["actions"][rows].astype(numpy.int64))
        cols["rewards"].append(snap["rewards"][rows])
        cols["to_play"].append(snap["to_play"][rows].astype(numpy.int64))
        cols["child_visits"].append(snap["child_visits"][base:base + T])
        cols["root_values"].append(snap["root_values"][base:base + T])
        if legal_mask:
            words = snap["legal_mask"][base:base + T].view(numpy.uint32)
            a = numpy.arange(A)
            cols["legal_mask"].append(((words[:, a >> 5] >> (a & 31).astype(numpy.uint32)) & 1).astype(numpy.uint8))
        if priorities:
            cols["priorities"].append(snap["priorities"][base:base + T])
    return {name: numpy.concatenate(parts) for name, parts in cols.items() if parts}


def export_order(ids):
    """Not the pool's order, and not every game: reversed, one game left out."""
    return [g for g in reversed(ids) if g != ids[2]]


# ------------------------------------------------------------------------------------------------ download_games

def check_download(backend, geometry, legal_mask, priorities):
    store, ids, snap = filled_store(backend, geometry, max_games=64 if priorities else None, legal_masks=legal_mask)
    chosen = export_order(ids)
    got = store.download_games(chosen)
    assert store.export_calls == 1
    want = restated(store, snap, chosen, legal_mask, priorities)
    lens = numpy.array([store.games[g][1] for g in chosen], dtype=numpy.int64)
    assert 0 in lens and 65 in lens and 1 in lens
    assert got["lengths"].dtype == numpy.int32 and got["lengths"].tolist() == lens.tolist()
    assert got["first1"].tolist() == (numpy.cumsum(lens + 1) - lens - 1).tolist()
    assert got["first0"].tolist() == (numpy.cumsum(lens) - lens).tolist()
    assert sorted(got) == sorted(list(want) + ["lengths", "first1", "first0"])
    for name, array in want.items():
        assert got[name].dtype == array.dtype and got[name].shape == array.shape, name
        assert got[name].tobytes() == array.tobytes(), name
    if legal_mask and GEOMETRIES[geometry][3]:
        assert 0 < got["legal_mask"].mean() < 1                 # illegal actions came back as zeros
    assert snapshot(store).keys() == snap.keys()
    for name, array in snap.items():                            # nothing of the store was written
        after = snapshot(store)[name]
        assert (after.tobytes() == array.tobytes()) if isinstance(array, numpy.ndarray) else after == array, name
    # only the games without a position: the arrays of T entries are empty
    short = [g for g in ids if store.games[g][1] == 0]
    empty = store.download_games(short)
    assert empty["child_visits"].shape == (0, store.A) and empty["root_values"].shape == (0,)
    assert empty["observations"].tobytes() == restated(store, snap, short, legal_mask, priorities)["observations"].tobytes()
    assert store.download_games([])["observations"].shape == (0,) + store.shape


def check_download_refusals(backend):
    store, ids, snap = filled_store(backend, "cartpole", max_games=None, legal_masks=False)
    with pytest.raises(LookupError, match="1000"):
        store.download_games([ids[0], 1000])
    store.drop(ids[0])
    with pytest.raises(LookupError, match=str(ids[0])):
        store.download_games([ids[0]])
    with pytest.raises(ValueError):
        store.download_games(ids[1:], legal_mask=True)
    with pytest.raises(ValueError):
        store.download_games(ids[1:], priorities=True)
    assert store.export_calls == 0
    assert "legal_mask" not in store.download_games(ids[1:]) and store.export_calls == 1


def check_download_after_reanalyse(backend):
    """The exported root values are the pool's column as it lies: a value written in place comes back."""
    store, ids, snap = filled_store(backend, "odd-frame")
    g = max(ids, key=lambda g: store.games[g][1])
    base, T = store.games[g]
    store.root_values[base + 2] = 0.125
    got = store.download_games([g])
    assert got["root_values"][2] == 0.125 and got["root_values"].shape == (T,)


# ------------------------------------------------------------------------------------------------ the ABI

class Packed:
    """Canary-filled packed arrays for direct calls of the entry, on the backend's device."""

    def __init__(self, backend, store, lens, frame_offset=0):
        self.backend, self.store = backend, store
        F, A = int(numpy.prod(store.shape)), store.A
        lens = numpy.asarray(lens, dtype=numpy.int64)
        self.G, self.R0 = len(lens), int(lens.sum())
        self.R1 = self.R0 + self.G
        dev = lambda a: torch.from_numpy(numpy.ascontiguousarray(a)).to(backend.device)
        self.d_len = dev(lens.astype(numpy.int32))
        self.d_dst1, self.d_dst0 = dev(numpy.cumsum(lens + 1) - lens - 1), dev(numpy.cumsum(lens) - lens)
        full = lambda shape, dtype: torch.full(shape, CANARY, dtype=dtype, device=backend.device)
        self.frame_offset = frame_offset
        self.block = full((frame_offset + self.R1 * F + 8,), torch.float32)      # (canaries on both sides of the frames)
        self.out = dict(d_actions=full((self.R1,), torch.int64), d_rewards=full((self.R1,), torch.float64),
                        d_to_play=full((self.R1,), torch.int64), d_child_visits=full((max(self.R0, 1), A), torch.float64),
                        d_root_values=full((max(self.R0, 1),), torch.float64),
                        d_legal_mask=full((max(self.R0, 1), A), torch.uint8), d_priorities=full((max(self.R0, 1),), torch.float32))

    def io(self, bases, legal_mask=True, priorities=True, **fields):
        x = _lib.ReplayExportIO()
        x.d_base, x.d_len, x.d_dst1, x.d_dst0 = (t.data_ptr() for t in (bases, self.d_len, self.d_dst1, self.d_dst0))
        x.d_observations = self.block.data_ptr() + 4 * self.frame_offset
        for name, t in self.out.items():
            setattr(x, name, t.data_ptr())
        if not legal_mask:
            x.d_legal_mask = None
        if not priorities:
            x.d_priorities = None
        x.total_rows, x.num_games = self.R1, self.G
        for k, v in fields.items():
            setattr(x, k, v)
        return x

    def frames(self):
        F = int(numpy.prod(self.store.shape))
        return host(self.block)[self.frame_offset:self.frame_offset + self.R1 * F].reshape(self.R1, F)

    def untouched(self):
        F = int(numpy.prod(self.store.shape))
        block = host(self.block)
        return ((block[:self.frame_offset] == CANARY).all() and (block[self.frame_offset + self.R1 * F:] == CANARY).all()
                and (self.frames() == CANARY).all() and all((host(t) == CANARY).all() for t in self.out.values()))


def call(backend, store, x, pool=None, sampler="own", mask="own", mask_rows=None):
    pool = store.pool if pool is None else pool
    sampler = store.sampler if sampler == "own" else sampler
    mask = store.legal_mask if mask == "own" else mask
    return backend.lib.mzx_replay_export(ctypes.byref(pool), None if sampler is None else ctypes.byref(sampler), backend.ptr(mask),
                                         (store.rows if mask is not None else 0) if mask_rows is None else mask_rows,
                                         None if x is None else ctypes.byref(x), backend.stream())


def check_frame_paths(backend):
    """Both paths of the frame copy on a geometry whose frames are whole 16-byte groups (320 floats: more than one group per
    lane): packed observations on a 16-byte boundary take the vector path, the same 4 bytes further the dword path.  Both
    land the same frames and nothing outside them."""
    store, ids, snap = filled_store(backend, "long-frame", legal_masks=False)
    assert store.frames.data_ptr() % 16 == 0
    chosen = export_order(ids)
    want = restated(store, snap, chosen, False, True)
    lens = [store.games[g][1] for g in chosen]
    d_base = store._up(numpy.array([store.games[g][0] for g in chosen], dtype=numpy.int64))
    for offset in (4, 5):
        packed = Packed(backend, store, lens, frame_offset=offset)
        assert packed.block.data_ptr() % 16 == 0
        assert call(backend, store, packed.io(d_base, legal_mask=False), mask=None) == 0
        block = host(packed.block)
        assert packed.frames().tobytes() == want["observations"].tobytes(), offset
        assert (block[:offset] == CANARY).all() and (block[offset + packed.frames().size:] == CANARY).all()
        assert host(packed.out["d_priorities"])[:packed.R0].tobytes() == want["priorities"].tobytes()
        assert (host(packed.out["d_legal_mask"]) == CANARY).all()


def check_passed_over(backend):
    """A game whose rows would leave the pool is passed over -- its packed rows keep what they held -- and the games around
    it are exported."""
    store, ids, snap = filled_store(backend, "odd-frame")
    chosen = [g for g in ids if store.games[g][1] in (3, 5)][:3]
    lens = [store.games[g][1] for g in chosen]
    for bad in (store.rows - lens[1], -1):                     # base + T == rows; a negative base
        bases = [store.games[g][0] for g in chosen]
        bases[1] = bad
        packed = Packed(backend, store, lens)
        assert call(backend, store, packed.io(store._up(numpy.array(bases, dtype=numpy.int64)))) == 0
        want = restated(store, snap, chosen, True, True)
        lo1, hi1 = lens[0] + 1, lens[0] + lens[1] + 2
        lo0, hi0 = lens[0], lens[0] + lens[1]
        got = dict(observations=packed.frames(), **{name[2:]: host(t) for name, t in packed.out.items()})
        for name in WHOLE + SEARCHED:
            lo, hi = (lo1, hi1) if name in WHOLE else (lo0, hi0)
            array = got[name].reshape((got[name].shape[0], -1))
            ref = want[name].reshape((want[name].shape[0], -1))
            assert (array[lo:hi] == CANARY).all(), name
            assert array[:lo].tobytes() == ref[:lo].tobytes() and array[hi:len(ref)].tobytes() == ref[hi:].tobytes(), name


def check_abi_refusals(backend):
    """Every refusal of include/mzx.h: MZX_ERR_INVALID with a message, nothing written; num_games == 0 succeeds and launches
    nothing; the accepted call writes, with and without the optional outputs."""
    lib = backend.lib
    store, ids, snap = filled_store(backend, "odd-frame")
    chosen = ids[:4]
    lens = [store.games[g][1] for g in chosen]
    d_base = store._up(numpy.array([store.games[g][0] for g in chosen], dtype=numpy.int64))
    packed = Packed(backend, store, lens)

    def refused(rc, word):
        assert rc == -1 and word in lib.mzx_last_error().decode(), (rc, lib.mzx_last_error())
        assert packed.untouched()

    refused(lib.mzx_replay_export(None, None, None, 0, ctypes.byref(packed.io(d_base)), backend.stream()), "null")
    refused(call(backend, store, None), "null")
    for name in ("d_base", "d_len", "d_dst1", "d_dst0", "d_observations", "d_actions", "d_rewards", "d_to_play", "d_child_visits",
                 "d_root_values"):
        refused(call(backend, store, packed.io(d_base, **{name: None})), "missing")
    refused(call(backend, store, packed.io(d_base, num_games=-1)), "negative")
    refused(call(backend, store, packed.io(d_base, total_rows=packed.G - 1)), "total_rows")
    refused(call(backend, store, packed.io(d_base), mask=None), "mask")
    refused(call(backend, store, packed.io(d_base), mask_rows=store.rows - 1), "mask")
    refused(call(backend, store, packed.io(d_base), sampler=None), "priorities")
    short = _lib.ReplaySampler.from_buffer_copy(store.sampler)
    short.rows = store.rows - 1
    refused(call(backend, store, packed.io(d_base), sampler=short), "priorities")
    bare = _lib.ReplayPool.from_buffer_copy(store.pool)
    bare.d_child_visits = None
    refused(call(backend, store, packed.io(d_base), pool=bare), "pool column")
    flat = _lib.ReplayPool.from_buffer_copy(store.pool)
    flat.action_space_size = 0
    refused(call(backend, store, packed.io(d_base), pool=flat), "positive")
    assert call(backend, store, packed.io(d_base, num_games=0, total_rows=0)) == 0
    assert packed.untouched()
    # accepted without the optional outputs, the sampler and the mask column: those two arrays keep their canaries
    want = restated(store, snap, chosen, True, True)
    assert call(backend, store, packed.io(d_base, legal_mask=False, priorities=False), sampler=None, mask=None) == 0
    assert packed.frames().tobytes() == want["observations"].tobytes()
    assert host(packed.out["d_child_visits"])[:packed.R0].tobytes() == want["child_visits"].tobytes()
    assert (host(packed.out["d_legal_mask"]) == CANARY).all() and (host(packed.out["d_priorities"]) == CANARY).all()
    assert call(backend, store, packed.io(d_base)) == 0
    for name in ("actions", "rewards", "to_play", "child_visits", "root_values", "legal_mask", "priorities"):
        n = packed.R1 if name in WHOLE else packed.R0
        assert host(packed.out["d_" + name])[:n].tobytes() == want[name].tobytes(), name


# =====================================================================================================================
# The device hand-off (config.device_handoff): resident rounds -> pieces on the device -> one ingest per piece.
#
# The comparator is never the new path alone: a twin shard with the same seed, weights and calls, ``device_games`` on and
# ``device_handoff`` off, whose games go through today's ``collect`` + ``save_games`` into a twin buffer.  Both feed
# identical inputs to identical kernels, so every comparison is bit for bit.  chunk = 3 (resident_rounds_cases.CHUNK).

FOREVER = rr.FOREVER


def replay_cfg(cfg, per=True, **extra):
    c = copy.copy(cfg)
    c.PER, c.PER_alpha, c.td_steps, c.num_unroll_steps, c.batch_size = per, 0.5, 4, 3, 8
    c.replay_buffer_size = 10 ** 6
    for k, v in extra.items():
        setattr(c, k, v)
    return c


def new_buffer(backend, cfg, rows, max_games=64, legal_masks=True):
    store = replay.DeviceGameStore(cfg, backend, rows, max_games=max_games, legal_masks=legal_masks)
    return replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=FeedbackStock, device_store=store, device_sampler=True)


class Run:
    """A resident shard and its buffer; ``handoff``: config.device_handoff.  Plays the calls, saving every call's games."""

    def __init__(self, backend, Game, cfg, weights, B, seed, handoff, rows=600, max_games=64, legal_masks=True, **extra):
        self.shard = rr.make_shard(backend, Game, cfg, weights, B, seed, True, device_handoff=handoff, **extra)
        self.buffer = new_buffer(backend, cfg, rows, max_games, legal_masks)
        self.store, self.B, self.handoff = self.buffer.device_store, B, handoff
        self.games, self.pieces, self.calls = [], 0, 0

    def play(self, calls, save=True):
        for temperature, kwargs in calls:
            out = self.shard.play_rounds(temperature, self.shard.config.temperature_threshold, **kwargs)
            assert len(out) == len(self.shard.finished_slots)
            if self.handoff:
                assert all(isinstance(record, _PieceRecord) and record.live for record, _, _ in out.records)
                self.pieces += len({id(record.piece) for record, _, _ in out.records})
            self.games += list(out)
            self.calls += 1
            if save:
                self.buffer.save_games(out)
        return self

    def close(self):
        self.shard.close_game()


def assert_same_run(ours, theirs, emptied=False, fields=True):
    """Pool, stock buffer, counters and residency alike; the games materialised from the store equal the twin's."""
    a, b = ours.buffer, theirs.buffer
    assert list(a.buffer) == list(b.buffer) and len(ours.games) == len(theirs.games) > 0
    for name in ("num_played_games", "num_played_steps", "total_samples"):
        assert getattr(a, name) == getattr(b, name), name
    assert ours.store.games == theirs.store.games
    assert_same_pool(ours.store, theirs.store, emptied=emptied)
    if fields:
        before = ours.store.export_calls
        for g in a.buffer:
            _same(a.buffer[g], b.buffer[g], g)
            for u, v in zip(a.buffer[g].observation_history, b.buffer[g].observation_history):
                assert numpy.asarray(u).dtype == numpy.asarray(v).dtype
        assert ours.store.export_calls == before + len(a.buffer)      # one export per game, whatever the fields touched


def both_runs(backend, Game, cfg, B, seed, calls, weights=None, **kwargs):
    weights = rr._weights(backend, cfg) if weights is None else weights
    ours = Run(backend, Game, cfg, weights, B, seed, True, **kwargs).play(calls)
    theirs = Run(backend, Game, cfg, weights, B, seed, False, **kwargs).play(calls)
    return ours, theirs


def assert_on_device(run):
    """It was on the device: the rounds were resident, one ingest per piece, bytes kept in pieces."""
    st = rr.assert_was_resident(run.shard, run.B)
    assert run.store.ingest_calls == run.pieces > 0
    assert st[7] > 0
    return st


def check_handoff_tictactoe(backend, per=True):
    """Case 1: tic-tac-toe, B = 5, two groups, calls mixing max_rounds and min_games; legal sets vary: the mask is staged."""
    cfg = replay_cfg(rr.tictactoe_cfg(), per)
    calls = rr.TICTACTOE_CALLS + [(1.0, dict(min_games=3))]
    ours, theirs = both_runs(backend, games.TicTacToeNative, cfg, 5, 7, calls)
    assert len(ours.shard._live["groups"]) == 2 and len(ours.games) >= 8
    assert len({g.__dict__["_view"][2] for g in ours.games}) > 1          # games of several lengths: several records per piece
    assert_on_device(ours)
    assert_same_run(ours, theirs)
    if per:
        assert (host(ours.store.priorities) > 0).any()
    ours.close(), theirs.close()


def check_handoff_synthetic(backend):
    """Case 2: the max_moves cut ends games, whole groups finish in one round -- in round 0 of a chunk too -- and with
    max_moves = 1 every game has one move."""
    for max_moves, rounds in ((5, (7, 6)), (1, (4, 3)), (3, (6, 4))):
        cfg = replay_cfg(configs.cartpole(num_simulations=7, max_moves=max_moves, action_space=list(range(3)),
                                          observation_shape=(2, 1, 3), players=list(range(2))))
        Native = games.make_native_synthetic_game(cfg.observation_shape, 3, 2)
        calls = [(1.0, dict(max_rounds=rounds[0], min_games=FOREVER)), (0.5, dict(max_rounds=rounds[1], min_games=FOREVER))]
        ours, theirs = both_runs(backend, Native, cfg, 12, 11, calls, weights=rr._weights(backend, cfg, 5), legal_masks=False)
        assert all(len(g.__dict__["_view"][0].rows_n) > 0 and g.__dict__["_view"][2] == max_moves for g in ours.games)
        # max_moves = 3 with chunk = 3: the games end in the last round of a chunk; max_moves = 1: in every round, round 0 too
        assert_on_device(ours)
        assert_same_run(ours, theirs)
        ours.close(), theirs.close()


def check_handoff_connect4(backend):
    """Case 3: Connect4, B = 65 -- a partial last workgroup of the pack --, max_rounds = 30; a store without a mask column."""
    cfg = replay_cfg(configs.connect4(num_simulations=4, blocks=1, channels=8))
    calls = [(1.0, dict(max_rounds=30, min_games=FOREVER))]
    ours, theirs = both_runs(backend, games.Connect4Native, cfg, 65, 3, calls, rows=2400, max_games=256, legal_masks=False)
    assert len(ours.games) >= 40
    assert_on_device(ours)
    assert_same_run(ours, theirs)
    ours.close(), theirs.close()


def check_handoff_eviction(backend, situation):
    """Case 4: eviction inside the hand-off -- the position bound (a pool too small for a call's games) or slot collisions
    (``max_games`` smaller than a call's games): the state of the twin, which uploads the same games through the host; a
    view whose game was evicted raises LookupError naming the game."""
    cfg = replay_cfg(rr.tictactoe_cfg())
    kwargs = dict(rows=40) if situation == "positions" else dict(rows=600, max_games=3)
    calls = [(1.0, dict(max_rounds=9, min_games=FOREVER)), (0.5, dict(max_rounds=9, min_games=FOREVER))]
    ours, theirs = both_runs(backend, games.TicTacToeNative, cfg, 5, 7, calls, **kwargs)
    assert len(ours.buffer.buffer) < len(ours.games), "nothing was evicted"
    assert ours.store.ingest_calls == ours.pieces
    assert_same_run(ours, theirs, emptied=True)
    gone = [h for h in ours.games if not any(h is kept for kept in ours.buffer.buffer.values())]
    assert gone
    with pytest.raises(LookupError, match="game"):
        gone[0].root_values
    ours.close(), theirs.close()


def check_handoff_halt_and_repair(backend):
    """Case 5: a tape short enough to halt every round (resident_rounds_cases.check_halt_and_repair): the same pool."""
    from mzx import search
    old = search.TAPE_WORDS
    search.TAPE_WORDS = 4
    try:
        cfg = replay_cfg(configs.cartpole(num_simulations=25, max_moves=4))
        Native = games.make_native_synthetic_game(cfg.observation_shape, len(cfg.action_space), 1)
        weights = {k: torch.zeros_like(v) if v.dtype.is_floating_point else v
                   for k, v in models.MuZeroNetwork(cfg, _backend=backend).state_dict().items()}
        calls = [(1.0, dict(max_rounds=5, min_games=FOREVER)), (0.5, dict(max_rounds=4, min_games=FOREVER))]
        ours, theirs = both_runs(backend, Native, cfg, 5, 7, calls, weights=weights, legal_masks=False)
        assert rr.assert_was_resident(ours.shard, 5)[2] > 0
        assert ours.store.ingest_calls == ours.pieces
        assert_same_run(ours, theirs)
        ours.close(), theirs.close()
    finally:
        search.TAPE_WORDS = old


def check_it_was_on_the_device(backend):
    """Case 6: the downloads of the rounds calls are bounded by control blocks and game states; bytes stay in pieces; one
    ingest per piece; mzx_actor_take is refused; a view touched before save_games downloads its piece once and still gives
    the twin's fields; the buffers are recycled."""
    lib = backend.lib
    cfg = replay_cfg(rr.tictactoe_cfg())
    weights = rr._weights(backend, cfg)
    B, calls = 5, rr.TICTACTOE_CALLS
    ours = Run(backend, games.TicTacToeNative, cfg, weights, B, 7, True)
    theirs = Run(backend, games.TicTacToeNative, cfg, weights, B, 7, False)
    ours.play(calls[:2]), theirs.play(calls[:2])
    groups = ours.shard._live["groups"]
    st, twin = ours.shard.stats["resident"], theirs.shard.stats["resident"]
    # per chunk and group: the control block (4 words) + the finished list (4 bytes per round of the chunk and slot) and
    # the game state.  The twin downloads exactly that PLUS the packed games: what it moved beyond ours is the game data.
    rounds, chunks = st[0], st[1]
    control = 4 * (4 * chunks + rounds // len(groups) * B)
    assert st[4] < twin[4] and st[2] == 0
    state = (st[4] - control) // chunks          # the game-state download of a chunk and group: the same every time
    assert st[4] == control + state * chunks and 0 < state <= 64 * B, (st, control, state)
    assert twin[4] - st[4] >= sum(8 * len(h.root_values) for h in theirs.games)      # (at least the root values alone)
    assert st[7] > 0 and st[6] == len(ours.games) == twin[6]
    assert ours.store.ingest_calls == ours.pieces and ours.pieces >= 2
    for g in groups:
        counts = (ctypes.c_int64 * 3)()
        assert lib.mzx_actor_finished(g.handle, -1, ctypes.byref(counts)) == -1
        assert b"hand-off" in lib.mzx_last_error()
        assert lib.mzx_actor_take(g.handle, -1, *([None] * 11)) == -1
        assert lib.mzx_actor_set_device_handoff(g.handle, 0) == 0 and lib.mzx_actor_set_device_handoff(g.handle, 1) == 0
    # recycling: a call of 9 rounds is three chunks, so a group never has more than three pieces out at once -- the buffers
    # (128 KiB each at these sizes) are reused call after call instead of one being allocated per piece
    for _ in range(3):
        ours.play(calls[2:]), theirs.play(calls[2:])
    ours.play(calls[2:], save=False), theirs.play(calls[2:], save=False)
    kept = ours.shard.stats["resident"][7]
    assert ours.pieces > 3 * len(groups) and kept % (2 << 16) == 0 and 0 < kept <= 3 * len(groups) * (2 << 16), (kept, ours.pieces)
    fresh, twin_fresh = ours.games[-1], theirs.games[-1]
    record = fresh.__dict__["_view"][0]
    piece = record.piece
    assert piece.live and piece.downloads == 0
    _same(fresh, twin_fresh, "touched before save_games")
    assert piece.downloads == 1 and not piece.live and piece.released
    for h, t in zip(ours.games, theirs.games):       # every other view of the piece reads the same download
        if h.__dict__["_view"][0].piece is piece:
            _same(h, t, "sibling")
    assert piece.downloads == 1
    # a hand-off that lacks a game of an untouched piece: the piece is fetched, the games go through the host
    out = ours.games[-len(ours.shard.finished_slots):]
    partial = [h for h in out if h is not fresh][:-1]
    handoff = ShardGames(partial)
    handoff.records = [(r, n, v) for r, n, v in _records_of(out)]
    before = ours.store.ingest_calls
    ours.buffer.save_games(handoff)
    assert all(not r.live for r, _, _ in handoff.records)
    for r, _, _ in handoff.records:                  # (pieces fetched for it are released: the actor holds none)
        assert r.piece.released
    assert ours.store.ingest_calls >= before
    ours.close(), theirs.close()


def _records_of(histories):
    seen, out = set(), []
    for h in histories:
        record, _, n = h.__dict__["_view"]
        if id(record) not in seen:
            seen.add(id(record))
            out.append((record, n, [x for x in histories if x.__dict__["_view"][0] is record]))
    return out


def check_overlap(backend):
    """Case 7: continuous_self_play with a local buffer (device store + sampler) against a local storage: the overlapped
    hand-off delivers the state the in-turn hand-off delivers; and against the twin without the flag."""
    games.NativeBatchedGame.backend = backend

    def once(overlap, handoff):
        cfg = replay_cfg(configs.tictactoe(num_simulations=5, training_steps=10, ratio=None, self_play_delay=0))
        cfg.self_play_overlap_handoff = overlap
        cfg.device_draws, cfg.device_games, cfg.device_games_chunk, cfg.device_handoff = True, True, rr.CHUNK, handoff
        weights = rr._weights(backend, cfg, 4)
        storage = shared_storage.LocalStorage(weights=weights, training_step=0, terminate=False, num_played_games=0,
                                              num_played_steps=0)
        buffer = new_buffer(backend, cfg, 2000)

        class Stopping:
            """The buffer, stopping the run after three hand-offs."""
            device_store, _sampler, save_game, calls = buffer.device_store, True, buffer.save_game, 0

            def save_games(self, histories, shared_storage=None):
                buffer.save_games(histories, shared_storage)
                Stopping.calls += 1
                if Stopping.calls >= 3:
                    storage.set_info("terminate", True)

        actor = self_play.SelfPlay({"weights": weights}, games.TicTacToeNative, cfg, 1, num_games=6, _backend=backend)
        actor.continuous_self_play(storage, Stopping())
        rr.assert_was_resident(actor, 6)
        return buffer, storage

    (a, sa), (b, _), (c, _) = once(True, True), once(False, True), once(True, False)
    n = min(len(a.buffer), len(b.buffer))
    assert n >= 6
    for x, y in ((a, b), (a, c)):
        for g in range(n):
            _same(x.buffer[g], y.buffer[g], g)
            bx, by = x.device_store.games[g], y.device_store.games[g]
            assert bx == by
            for name in ("frames", "actions", "rewards", "to_play", "root_values", "child_visits", "priorities", "legal_mask"):
                u, v = (host(getattr(s.device_store, name))[bx[0]:bx[0] + bx[1] + 1] for s in (x, y))
                assert u.tobytes() == v.tobytes(), (name, g)
    assert a.num_played_games == sa.get_info("num_played_games") == len(a.buffer)
    assert a.device_store.ingest_calls >= 3
    batch = a.get_batch()                            # the device sampler draws from what the hand-off stored
    assert batch[1][0].shape[0] == a.config.batch_size


def check_refusals(backend):
    """Case 9: the flag without device_games; continuous_self_play with a buffer that is remote, has no device store or no
    device sampler; mzx_actor_set_device_handoff on a group that is not resident or has games pending."""
    lib = backend.lib
    cfg = replay_cfg(rr.tictactoe_cfg())
    weights = rr._weights(backend, cfg)
    games.NativeBatchedGame.backend = backend
    c = copy.copy(cfg)
    c.device_draws, c.device_handoff = True, True
    shard = self_play.SelfPlay({"weights": weights}, games.TicTacToeNative, c, 7, num_games=4, _backend=backend)
    with pytest.raises(NotImplementedError, match="device_handoff"):
        shard.play_rounds(1.0, None, max_rounds=2, min_games=FOREVER)
    shard.close_game()

    c.device_games, c.device_games_chunk = True, rr.CHUNK
    storage = shared_storage.LocalStorage(weights=weights, training_step=0, terminate=True, num_played_games=0, num_played_steps=0)

    class Remote:
        class save_game:
            remote = staticmethod(lambda *a: None)

    no_store = replay.ReplayBuffer(dict(CHECKPOINT), {}, c, stock=FeedbackStock)
    store = replay.DeviceGameStore(c, backend, 100, max_games=16, legal_masks=True)
    no_sampler = replay.ReplayBuffer(dict(CHECKPOINT), {}, c, stock=FeedbackStock, device_store=store)
    for buffer in (Remote(), no_store, no_sampler):
        actor = self_play.SelfPlay({"weights": weights}, games.TicTacToeNative, c, 7, num_games=4, _backend=backend)
        with pytest.raises(NotImplementedError, match="device_handoff"):
            actor.continuous_self_play(storage, buffer)
        actor.close_game()
    # the ABI
    assert lib.mzx_actor_set_device_handoff(None, 1) == -1
    drawn = rr.make_shard(backend, games.TicTacToeNative, cfg, weights, 4, 7, False)
    handle = drawn._native_shard(1.0).groups[0].handle
    assert lib.mzx_actor_set_device_handoff(handle, 1) == -1 and b"resident" in lib.mzx_last_error()
    counts = (ctypes.c_int64 * 2)()
    assert lib.mzx_actor_finished_device(handle, -1, ctypes.byref(counts)) == -1
    assert lib.mzx_actor_release_device(handle, 1, None) == -1
    drawn.close_game()
    resident = rr.make_shard(backend, games.TicTacToeNative, cfg, weights, 4, 7, True)
    native = resident._native_shard(1.0)
    native.rounds(1.0, None, FOREVER, 9)             # finished games pending in the default queue
    for g in native.groups:
        assert lib.mzx_actor_set_device_handoff(g.handle, 1) == -1 and b"pending" in lib.mzx_last_error()
    native.collect()
    for g in native.groups:
        assert lib.mzx_actor_set_device_handoff(g.handle, 1) == 0
        g.handoff = True
    native.rounds(1.0, None, FOREVER, 9)             # ... and in the piece queue
    for g in native.groups:
        assert lib.mzx_actor_set_device_handoff(g.handle, 0) == -1 and b"pending" in lib.mzx_last_error()
        assert lib.mzx_actor_release_device(g.handle, 12345, None) == -1 and b"token" in lib.mzx_last_error()
    out, _ = native.collect()
    assert len(out) > 0 and all(r.live for r, _, _ in out.records)
    resident.close_game()                            # closing fetches what nobody ingested
    assert all(not r.live and r.piece.released for r, _, _ in out.records)
    assert len(out[0].root_values) == out[0].__dict__["_view"][2]


def check_max_log_bytes(backend):
    """Device log plus pieces are refused above max_log_bytes, with a message that states the sizes."""
    cfg = replay_cfg(rr.tictactoe_cfg())
    weights = rr._weights(backend, cfg)
    probe = rr.make_shard(backend, games.TicTacToeNative, cfg, weights, 4, 7, True)
    probe.play_rounds(1.0, None, max_rounds=3, min_games=FOREVER)
    log = probe.stats["resident"][5] // 2            # (two groups of the same size)
    probe.close_game()
    shard = rr.make_shard(backend, games.TicTacToeNative, cfg, weights, 4, 7, True, device_handoff=True,
                          device_games_max_bytes=log + 64)
    with pytest.raises(_lib.MzxError, match="max_log_bytes"):
        shard.play_rounds(1.0, None, max_rounds=9, min_games=FOREVER)
    shard.close_game()
