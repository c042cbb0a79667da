"""
``SelfPlay.play_rounds`` for a shard of NATIVELY stepped games: the whole round loop behind one library call.

Reference: the actor loop and ``play_game`` of /root/reference/self_play.py:31-52, :110-183 -- per move of one game:
MCTS.run, select_action, Game.step, GameHistory appends; the next game starts the moment one ends.  ``mzx.self_play``
plays B such actors as one shard; through a Python plugin game (batched protocol) a round costs ~75 interpreter
statements per slot group around two library calls, which holds BASELINE config C2 (a 0.2 ms search of 4096 trees) at a
third of its search rate.  When the game object steps inside the library (``mzx.games.NativeBatchedGame``:
``native_handle``) the rounds run in ``mzx_selfplay_rounds`` (include/mzx.h, csrc/mzx_actor.h) -- searches, action draws,
steps, history rows, finished games copied out, slots refilled, two slot groups taking turns on the GPU -- and this module
is what remains on the Python side: building the actors once, one call per ``play_rounds``, and wrapping the finished
games it hands back (game-major arrays) into the same ``ShardGameHistory`` views the Python loop produces.

Same games, field for field, in the same order as ``SelfPlay._rounds_batched`` on the same game object
(``config.native_rounds = False`` keeps that loop: the A/B and the parity reference, tests/test_native_rounds.py).
Stacked observations (the device frame store) and Python plugin games stay on the Python loop.
"""
import ctypes

import numpy

from . import _lib, draws
from .history import ShardGameHistory, ShardGames, _PieceRecord, _ShardRecord, gc_paused, shard_record_fields
from . import search as _search
from .search import BatchedMCTS
from .shard_play import SlotGroup


def resident_wanted(config):
    """``config.device_games``: the shard's games, move log and bookkeeping stay on the device (csrc/mzx_resident.h)."""
    return bool(getattr(config, "device_games", False))


def handoff_wanted(config):
    """``config.device_handoff``: a resident shard's finished games stay on the device until the replay store ingests them."""
    return bool(getattr(config, "device_handoff", False))


def check_handoff(actor):
    """``config.device_handoff`` sits on top of ``config.device_games``: anything else is an error, no silent fall-back."""
    if not resident_wanted(actor.config):
        raise NotImplementedError("config.device_handoff: config.device_games is off (only resident rounds keep their finished "
                                  "games on the device)")


def check_handoff_buffer(config, replay_buffer):
    """``continuous_self_play`` with ``config.device_handoff``: nothing on the host may need the histories to sample, so the
    buffer must be local, with a device store and the device sampler."""
    if not handoff_wanted(config):
        return
    why = None
    if hasattr(getattr(replay_buffer, "save_game", None), "remote"):
        why = "the replay buffer is remote (the games cannot leave the device's process)"
    elif getattr(replay_buffer, "device_store", None) is None:
        why = "the replay buffer has no device store"
    elif not getattr(replay_buffer, "_sampler", False):
        why = "the replay buffer has no device sampler (the host draws would read the histories)"
    if why is not None:
        raise NotImplementedError(f"config.device_handoff: {why}")


class _Piece:
    """A piece of a hand-off group (include/mzx.h ``mzx_actor_take_device``): the finished games of one chunk, packed on the
    device in a buffer the actor owns.  ``ptr``: the device addresses ``mzx_replay_ingest`` reads; ``length`` per game on
    the host.  ``fetch`` downloads it -- once, one copy per column, converted as ``collect`` converts -- and releases it."""

    def __init__(self, group, backend, info, length, A, shape):
        self.group, self.backend, self.A, self.shape = group, backend, A, tuple(shape)
        self.token, self.games, self.rows0, self.has_mask = int(info[0]), int(info[1]), int(info[2]), bool(info[3])
        names = ("len", "src1", "src0", "obs", "acts", "rews", "tps", "vis", "vals", "mask")
        self.ptr = {name: int(info[4 + j]) or None for j, name in enumerate(names)}
        self.bytes = int(info[14])
        self.length = length
        self.columns, self.released, self.downloads = None, False, 0

    @property
    def live(self):
        return self.columns is None and not self.released

    def release(self, stream=None):
        """The buffer may be reused once the work queued on ``stream`` (default: the backend's) so far has finished."""
        if not self.released:
            g = self.group
            g.lib.check(g.lib.mzx_actor_release_device(g.handle, self.token, self.backend.stream() if stream is None else stream))
            self.released = True
            g.pieces.remove(self)

    def fetch(self):
        if self.columns is None:
            if self.released:
                raise LookupError("the piece was handed over on the device and released: its games are read from the replay store")
            g, A, E = self.group, self.A, int(numpy.prod(self.shape))
            rows, G = self.rows0, self.games
            obs = numpy.empty((rows + G, E), numpy.float32)
            acts, tps = numpy.empty(rows + G, numpy.int64), numpy.empty(rows + G, numpy.int64)
            rews = numpy.empty(rows + G, numpy.float64)
            vis, vals = numpy.empty((rows, A), numpy.int32), numpy.empty(rows, numpy.float64)
            mask = numpy.empty((rows, A), numpy.uint8) if self.has_mask else None
            g.lib.check(g.lib.mzx_actor_download_device(g.handle, self.token, obs.ctypes.data, acts.ctypes.data, rews.ctypes.data,
                                                        tps.ctypes.data, vis.ctypes.data, vals.ctypes.data,
                                                        None if mask is None else mask.ctypes.data, self.backend.stream()))
            self.downloads += 1
            game = g.game
            if game.obs_dtype != numpy.float32:
                obs = obs.astype(game.obs_dtype)
            if game.reward_dtype is numpy.int64:
                rews = rews.astype(numpy.int64)
            if mask is not None and mask.all():       # (every action legal throughout: the record carries no mask)
                mask = None
            self.columns = (obs, acts, rews, tps, vis, vals, mask)
            self.release()
        return self.columns

    def record_fields(self, rows_n, n):
        obs, acts, rews, tps, vis, vals, mask = self.fetch()
        length = self.length
        off1, off0 = numpy.cumsum(length + 1) - (length + 1), numpy.cumsum(length) - length
        names = ("A", "obs", "acts", "rews", "tps", "vis", "vals", "totals", "ratios", "simple", "legal_mask")
        return dict(zip(names, shard_record_fields(self.A, self.shape, self.games, n, rows_n, off1, off0, obs, acts, rews, tps,
                                                   vis, vals, mask)))


def check_resident(actor):
    """With ``config.device_games`` set, every case the resident loop does not cover is an error: no silent fall-back."""
    cfg, game = actor.config, actor.batched_game
    why = None
    if not bool(getattr(actor, "device_draws", False)):
        why = "config.device_draws is off (the resident rounds draw on the device)"
    elif game is None:
        why = "the per-object game paths are not covered (a batched, natively stepped game is needed)"
    elif not getattr(game, "native_handle", None):
        why = "the game has no native_handle (Python plugin games step in the interpreter)"
    elif cfg.stacked_observations != 0:
        why = "stacked observations are not covered"
    elif not getattr(cfg, "native_rounds", True):
        why = "config.native_rounds = False keeps the Python round loop"
    elif not usable(actor):
        why = "the shard cannot play its rounds natively"
    if why is not None:
        raise NotImplementedError(f"config.device_games: {why}")


def usable(actor):
    """Whether ``actor``'s shard can play its rounds natively."""
    game = actor.batched_game
    return (game is not None and getattr(game, "native_handle", None) and actor.bank is not None
            and actor.config.stacked_observations == 0 and getattr(actor.config, "native_rounds", True)
            and actor.engine.fused_move and len(actor.config.action_space) <= 4096)


class _Group(SlotGroup):
    """A slot group whose rounds run inside the library: one ``mzx_actor`` over the group's game, engine and staging."""

    def __init__(self, actor, game, first, n, engine, temperature):
        cfg, lib = actor.config, actor.model.backend.lib
        super().__init__(first, n, engine, game, owns_game=game is not actor.batched_game)
        A = len(cfg.action_space)
        obs_floats = int(numpy.prod(cfg.observation_shape))
        assert tuple(game.shape) == tuple(cfg.observation_shape), \
            f"Observation should match the observation_shape defined in MuZeroConfig. Expected {tuple(cfg.observation_shape)} but got {tuple(game.shape)}."
        assert game.A == A, f"the game has {game.A} actions, the configuration {A}"
        device_draws = bool(getattr(actor, "device_draws", False))
        st = self.staging = engine._staging(n, _search.TAPE_WORDS, obs_floats, True, device_draws=device_draws)
        pin, pout = st["pin"], st["pout"]
        c_vp = ctypes.c_void_p
        if device_draws:        # noise and tape are device scratch: nothing of them is uploaded (csrc/mzx_draws.h)
            pin = dict(pin, noise=st["draw_noise"].data_ptr(), tape=st["draw_tape"].data_ptr())
        self.tape_words = _search.TAPE_WORDS      # (of this group's handle and staging; the retries grow from it)
        self.arena = engine.arena(n)
        conf = _lib.ActorConfig()
        conf.game, conf.search, conf.bank = game.native_handle, engine.handle(n, _search.TAPE_WORDS), actor.bank.handle
        conf.streams, conf.first_slot, conf.max_moves = self.streams.ctypes.data, first, int(cfg.max_moves)
        conf.temperature = float(temperature)
        conf.d_arena, conf.arena_bytes = self.arena.data_ptr(), self.arena.numel()
        mv = conf.move
        mv.num_games, mv.action_space_size, mv.tape_words, mv.num_threads = n, A, _search.TAPE_WORDS, actor.bank.threads
        mv.dirichlet_alpha, mv.add_exploration_noise = float(cfg.root_dirichlet_alpha), 1
        mv.h_in, mv.d_in, mv.in_bytes = st["h_in"].data_ptr(), st["d_in"].data_ptr(), st["h_in"].numel()
        mv.h_out, mv.d_out, mv.out_bytes = st["h_out"].data_ptr(), st["d_out"].data_ptr(), st["h_out"].numel()
        mv.io = _lib.SearchIO(c_vp(pin["obs"]), c_vp(pin["legal"]), c_vp(pin["to_play"]), c_vp(pin["noise"]), c_vp(pin["tape"]),
                              c_vp(pout["visits"]), c_vp(pout["root_value"]), c_vp(pout["predicted"]), c_vp(pout["info"]))
        self.handle = c_vp()
        lib.check(lib.mzx_actor_create(ctypes.byref(conf), ctypes.byref(self.handle)))
        self.lib = lib
        if device_draws:        # the group's search number is its counter, its slots are the streams
            lib.check(lib.mzx_actor_set_device_draws(self.handle, engine.draw_seed & (2 ** 64 - 1), int(actor.draw_counter),
                                                     c_vp(pin["temperature"]), c_vp(pout["action"])))
        self.resident = resident_wanted(cfg)
        if self.resident:       # games, move log and bookkeeping on the device; the host returns once per chunk of rounds
            lib.check(lib.mzx_actor_set_resident(self.handle, int(getattr(cfg, "device_games_chunk", 16)),
                                                 int(getattr(cfg, "device_games_max_bytes", 2 << 30))))
        self.handoff = self.resident and handoff_wanted(cfg)
        self.pieces = []        # the pieces taken and not released yet (the device hand-off)
        self.backend = actor.model.backend
        if self.handoff:        # finished games stay on the device, in pieces the actor owns
            lib.check(lib.mzx_actor_set_device_handoff(self.handle, 1))

    def resident_stats(self):
        out = (ctypes.c_int64 * 8)()
        self.lib.check(self.lib.mzx_actor_resident_stats(self.handle, ctypes.byref(out)))
        return list(out)

    def close(self):
        for piece in list(self.pieces):       # (their buffers go with the actor: what nobody ingested comes to the host)
            piece.fetch()
        handle, self.handle = self.handle, None
        if handle:
            self.lib.mzx_actor_destroy(handle)
        super().close()


class NativeShard:
    """The state of ``play_rounds`` for a natively stepped shard: one ``mzx_actor`` per slot group."""

    def __init__(self, actor, temperature):
        cfg, B = actor.config, actor.num_games
        spans = actor._slot_spans(B, batched=True)
        self.groups = []
        for first, last in spans:
            single = len(spans) == 1
            game = actor.batched_game if single else type(actor.batched_game)(actor._game_seeds[first:last],
                                                                              _backend=actor.model.backend)
            engine = actor.engine if single else BatchedMCTS(cfg, actor.model, last - first)
            engine.draw_seed = getattr(actor, "draw_seed", engine.draw_seed)
            self.groups.append(_Group(actor, game, first, last - first, engine, temperature))
        self.handles = (ctypes.c_void_p * len(self.groups))(*[g.handle for g in self.groups])
        self.resident = all(g.resident for g in self.groups)
        self.temperatures = set()
        self.sequence = 0
        self.error = None
        self._actor = actor
        self._retry = _lib.RETRY_FN(self._retry_flagged)      # (kept alive: the library calls it during a rounds call)

    def set_draw_counter(self, value):
        """Device draws: every group's next search takes this counter (``SelfPlay.draw_counter``)."""
        for g in self.groups:
            g.lib.check(g.lib.mzx_actor_set_draw_counter(g.handle, int(value) & (2 ** 64 - 1)))

    # ---- the rare path: a search exhausted its tie-break tape (equal priors at every level of a walk) ------------------
    def _retry_flagged(self, ctx, group, count, games):
        """Searches the flagged games of slot group ``group`` again on a longer tape -- same roots, same noise, the stream
        peeked further (BatchedMCTS._complete_run's loop) -- and writes the results into the group's output block."""
        try:
            actor, g = self._actor, self.groups[group]
            cfg, A, n = actor.config, len(actor.config.action_space), g.n
            redo = numpy.array([games[k] for k in range(count)], dtype=numpy.int64)
            vin, vout = g.staging["vin"], g.staging["vout"]
            legal, to_play = vin["legal"].reshape(n, A), vin["to_play"]
            device_draws = "draw_noise" in g.staging
            if device_draws:     # the noise the roots got, and the (stream, counter) the longer tapes are drawn under
                noise = g.staging["draw_noise"].cpu().numpy()
                counter = int(self.groups[group].lib.mzx_actor_draw_counter(g.handle)) - 1
            else:
                noise = vin["noise"].reshape(n, A)
            obs = vin["obs"].reshape(n, -1)
            visits, info = vout["visits"].reshape(n, A), vout["info"].reshape(n, 4)
            n_legal = (legal >= 0).sum(1).astype(numpy.int32)
            words = g.tape_words
            while redo.size:
                words *= 8
                if words > (1 << 22):
                    raise _lib.MzxError("tie-break tape: a search consumed more than 4M random words")
                if device_draws:
                    long_tape = draws.root_draws(actor.model.backend, g.engine.draw_seed, counter, len(redo), A, words,
                                                 streams=g.streams[redo], noise=False)[1].cpu().numpy().view(numpy.uint32)
                else:
                    _, long_tape = actor.bank.root_draws(g.streams[redo], cfg.root_dirichlet_alpha, n_legal[redo], A, words,
                                                         with_noise=False)
                v2, r2, p2, i2 = g.engine._launch(len(redo), obs[redo].copy(), legal[redo].copy(), to_play[redo].copy(),
                                                  noise[redo].copy(), long_tape, words, None)
                visits[redo], vout["root_value"][redo], vout["predicted"][redo], info[redo] = v2, r2, p2, i2
                redo = redo[(i2[:, 1] & 1) != 0]
            return 0
        except Exception as e:      # noqa: BLE001  (must not propagate through the C frame; re-raised by play())
            self.error = e
            return 1

    # ---- one play_rounds call -------------------------------------------------------------------------------------------
    def play(self, temperature, temperature_threshold, min_games, max_rounds):
        import time

        before = self.rounds(temperature, temperature_threshold, min_games, max_rounds)
        t0 = time.perf_counter()
        out = self.collect(before)
        self._actor.stats["native_phase_seconds"][6] += time.perf_counter() - t0      # the finished games wrapped into GameHistory views (Python)
        return out

    def rounds(self, temperature, temperature_threshold, min_games, max_rounds):
        """The library call alone (it holds no interpreter lock: ``continuous_self_play`` runs it on a worker thread while
        the main thread hands the previous call's games over).  Returns the sequence number behind the last game this call
        finished: ``collect(before)`` hands out exactly the games finished so far.

        Resident rounds (``config.device_games``): ``max_rounds`` is exact.  With ``min_games`` the call plays whole chunks
        and stops at the first chunk end with enough finished games.  It may play up to ``chunk_rounds - 1`` rounds more
        than the host loop would."""
        actor = self._actor
        lib, engine = actor.model.backend.lib, actor.engine
        t = float(temperature)
        if t != 0 and not numpy.isinf(t):
            self.temperatures.add(t)
        key = tuple(sorted(self.temperatures))
        stride = engine.num_simulations + 2
        cache = actor.__dict__.setdefault("_pow_tables", {})
        entry = cache.get((key, stride))
        if entry is None:       # visit_count ** (1 / T) over 0 .. num_simulations + 1: numpy's own pow (self_play.py:236-243)
            table = (numpy.ascontiguousarray(numpy.stack([numpy.arange(stride, dtype="int32") ** (1 / x) for x in key]))
                     if key else None)
            entry = cache[(key, stride)] = (table, numpy.array(key, numpy.float64))
        table, distinct = entry
        io = _lib.Rounds()
        io.temperature, io.temperature_threshold = t, int(temperature_threshold or 0)
        io.table_stride = stride
        io.pow_table = None if table is None else table.ctypes.data
        io.table_temperatures = distinct.ctypes.data if distinct.size else None
        io.num_temperatures = int(distinct.size)
        io.min_games, io.max_rounds = int(min(min_games, 1 << 62)), -1 if max_rounds is None else int(max_rounds)
        io.sequence = self.sequence
        io.retry, io.retry_ctx = self._retry, None
        self.error = None
        rc = lib.mzx_selfplay_rounds(self.handles, len(self.groups), ctypes.byref(io), actor.model.backend.stream())
        if self.resident:       # the eight counters of include/mzx.h mzx_actor_resident_stats, summed over the groups
            actor.stats["resident"] = [sum(x) for x in zip(*[g.resident_stats() for g in self.groups])]
        if self.error is not None:
            raise self.error
        lib.check(rc)
        self.sequence = int(io.sequence)
        actor._count_search(int(io.searches), engine, float(io.search_seconds))
        phases = actor.stats.setdefault("native_phase_seconds", [0.0] * 7)      # (diagnostics: where the host time of the calls went)
        for k in range(6):
            phases[k] += float(io.phase_seconds[k])
        return self.sequence

    def _collect_pieces(self, g, before, A, shape, views_all, seq_all, slot_all, records):
        """``collect`` for a group on the device hand-off: its pieces numbered below ``before``, every (piece, length) a
        ``_PieceRecord`` whose arrays are fetched on first touch."""
        lib = g.lib
        counts = (ctypes.c_int64 * 2)()
        lib.check(lib.mzx_actor_finished_device(g.handle, int(before), ctypes.byref(counts)))
        P, G = int(counts[0]), int(counts[1])
        if G == 0:
            return
        info = numpy.zeros((P, _lib.PIECE_INFO_WORDS), numpy.int64)
        slot, length, seq = numpy.empty(G, numpy.int32), numpy.empty(G, numpy.int32), numpy.empty(G, numpy.int64)
        lib.check(lib.mzx_actor_take_device(g.handle, int(before), P, G, info.ctypes.data, slot.ctypes.data, length.ctypes.data,
                                            seq.ctypes.data, ctypes.byref(counts)))
        assert (int(counts[0]), int(counts[1])) == (P, G)
        lo = 0
        for row in info:
            k_piece = int(row[1])
            sl = slice(lo, lo + k_piece)
            lo += k_piece
            piece = _Piece(g, g.backend, row, length[sl].copy(), A, shape)
            g.pieces.append(piece)
            for n in numpy.unique(piece.length).tolist():
                rows_n = numpy.nonzero(piece.length == n)[0]
                k = int(rows_n.size)
                record = _PieceRecord(A, shape, piece, rows_n, n)
                with gc_paused():
                    views = ShardGameHistory.make_many(record, k, n)
                views_all += views
                seq_all.append(seq[sl][rows_n])
                slot_all.append(slot[sl][rows_n])
                records.append((record, n, views))

    def collect(self, before=-1, priorities_for=None):
        """The finished games of every group (numbered below ``before``; -1: all) as ``ShardGameHistory`` views, in the order
        they finished; their slots.  ``priorities_for`` (a configuration with PER on; ``continuous_self_play``'s hand-off):
        the initial PER priorities of every record are computed on the device right here and every view is created with its
        row -- the buffer's save_game reads them for every game.

        ``config.device_handoff``: the same ``ShardGames``, but every record is piece-backed (``_PieceRecord``: its arrays
        are fetched on first touch, nothing is downloaded for a record nobody touches) and ``priorities_for`` is ignored --
        ``ReplayBuffer.save_games`` ingests the pieces on the device, and the ingest computes the priorities."""
        actor = self._actor
        lib, A = actor.model.backend.lib, len(actor.config.action_space)
        shape = tuple(actor.config.observation_shape)
        E = int(numpy.prod(shape))
        views_all, seq_all, slot_all, records = [], [], [], []
        for g in self.groups:
            if g.handoff:       # piece-backed records: nothing of the games is downloaded (priorities_for: the ingest's)
                self._collect_pieces(g, before, A, shape, views_all, seq_all, slot_all, records)
                continue
            counts = (ctypes.c_int64 * 3)()
            lib.check(lib.mzx_actor_finished(g.handle, int(before), ctypes.byref(counts)))
            G, rows = int(counts[0]), int(counts[1])
            if G == 0:
                continue
            slot, length, seq = numpy.empty(G, numpy.int32), numpy.empty(G, numpy.int32), numpy.empty(G, numpy.int64)
            obs = numpy.empty((rows + G, E), numpy.float32)
            acts, tps = numpy.empty(rows + G, numpy.int64), numpy.empty(rows + G, numpy.int64)
            rews = numpy.empty(rows + G, numpy.float64)
            vis, vals = numpy.empty((rows, A), numpy.int32), numpy.empty(rows, numpy.float64)
            mask = numpy.empty((rows, A), numpy.uint8) if counts[2] else None
            illegal = ctypes.c_int32()
            lib.check(lib.mzx_actor_take(g.handle, int(before), slot.ctypes.data, length.ctypes.data, seq.ctypes.data, obs.ctypes.data,
                                         acts.ctypes.data, rews.ctypes.data, tps.ctypes.data, vis.ctypes.data, vals.ctypes.data,
                                         None if mask is None else mask.ctypes.data, ctypes.byref(illegal)))
            game = g.game
            if game.obs_dtype != numpy.float32:       # the dtype the reference game's arrays have (planes of -1 / 0 / 1: exact)
                obs = obs.astype(game.obs_dtype)
            if game.reward_dtype is numpy.int64:
                rews = rews.astype(numpy.int64)
            off1 = numpy.cumsum(length + 1) - (length + 1)
            off0 = numpy.cumsum(length) - length
            for n in numpy.unique(length).tolist():
                rows_n = numpy.nonzero(length == n)[0]
                k = int(rows_n.size)
                record = _ShardRecord(*shard_record_fields(A, shape, G, n, rows_n, off1, off0, obs, acts, rews, tps, vis, vals,
                                                           mask if mask is not None and illegal.value else None))
                vl, totals = record.vals, record.totals
                if priorities_for is not None and getattr(priorities_for, "PER", False) and n > 0:
                    from . import replay
                    record.priorities, record.game_priority = replay.device_priorities(
                        actor.model.backend, numpy.where(totals > 0, vl, 0.0), record.tps, record.rews, priorities_for)
                with gc_paused():
                    views = ShardGameHistory.make_many(record, k, n)
                views_all += views
                seq_all.append(seq if k == G else seq[rows_n])
                slot_all.append(slot if k == G else slot[rows_n])
                records.append((record, n, views))
        if not views_all:
            return ShardGames(), []
        seq, slot = numpy.concatenate(seq_all), numpy.concatenate(slot_all)
        if (seq[1:] > seq[:-1]).all():          # one group, one length: already in finishing order
            out, slots = ShardGames(views_all), slot.tolist()
        else:
            order = numpy.argsort(seq, kind="stable")
            out, slots = ShardGames([views_all[i] for i in order.tolist()]), slot[order].tolist()
        out.records = records
        return out, slots
