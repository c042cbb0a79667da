"""
What ``SelfPlay`` (mzx/self_play.py) keeps per shard: the slot groups of ``play_rounds`` and the bookkeeping rules every
protocol shares -- the temperature of a move, the legal-mask row of a move, finished games as ``ShardGameHistory`` views.

A SLOT GROUP is a run of slots of a shard that is searched with one launch.  A shard is one group, or several that take
turns on the GPU (``SelfPlay._slot_spans``).  ``SlotGroup`` holds what every reader of ``SelfPlay._live["groups"]`` uses;
the protocols add their own state: ``ObjectGroup`` (B plugin ``Game`` objects), ``BatchedGroup`` (the batched plugin
protocol) and ``native_rounds._Group`` (games stepped inside the library).
"""
import numpy

from . import observations as observations_mod
from .history import ShardGameHistory, _ShardRecord, gc_paused


def move_temperature(temperature, moves, threshold):
    """
    The temperature of a game's next move (self_play.py:151-157): ``temperature`` until the game's action history holds
    ``threshold`` entries, 0 from then on.  ``temperature``: a number or one per game; ``moves``: len(action_history), a
    number or one per game (only read with a threshold).
    """
    if not threshold:
        return temperature
    if numpy.isscalar(moves):
        return temperature if moves < threshold else 0
    return numpy.where(numpy.asarray(moves) < threshold, temperature, 0.0)


def legal_mask_row(legal, idx, B, A):
    """
    The legal-mask row of one move of a batched shard: bool [B][A], row ``idx[i]`` set at the actions ``legal[i]`` holds
    (a [len(idx)][A] array padded with -1, or lists).  None when an array says that every action is legal everywhere.
    """
    if isinstance(legal, numpy.ndarray):
        given = legal >= 0
        if given.all():
            return None
        mask = numpy.zeros((B, A), bool)
        mask[numpy.repeat(idx, given.sum(1)), legal[given]] = True
    else:
        mask = numpy.zeros((B, A), bool)
        for r, acts in zip(idx, legal):
            mask[r, acts] = True
    return mask


def shard_views(A, obs, acts, rews, tps, vis, vals, legal_mask, lengths, time_major=False):
    """
    The logged moves of some games as one ``_ShardRecord`` and a ``ShardGameHistory`` view per game (self_play.py:479-511).
    The arrays lie game-major ([game][move]; game i played ``lengths[i]`` moves, shorter games are padded) or, with
    ``time_major``, as a slot group's ring rows lie ([move][game], one length) -- the record views either, nothing is
    transposed here.  ``vis`` None: no move was played.
    """
    if vis is None:
        record = _ShardRecord(A, obs, acts, rews, tps)
    else:
        totals = vis.sum(2)
        ratios = vis / numpy.maximum(totals, 1)[:, :, None]       # true division of small integers == Python's int / int
        plain = totals > 0
        if not time_major:                                        # (the padding behind a shorter game's end is no exception)
            plain |= numpy.arange(vis.shape[1])[None, :] >= numpy.asarray(lengths)[:, None]
        if legal_mask is not None:
            plain &= legal_mask.all(2)
        record = _ShardRecord(A, obs, acts, rews, tps, vis, vals, totals, ratios, plain.all(0 if time_major else 1), legal_mask,
                              time_major=time_major)
    with gc_paused():
        return [ShardGameHistory(record, i, n) for i, n in enumerate(lengths)]


class SlotGroup:
    """Slots ``first .. first + n - 1`` of a shard: their engine, their game object (batched protocols; ``owns_game``: one
    of the group's own, closed with it), their frame store and the search that is queued or running for them."""
    streams_before = None       # (per-object groups: set while a search that may be dropped is queued)

    def __init__(self, first, n, engine, game=None, owns_game=False):
        self.first, self.n, self.engine, self.game, self.owns_game = first, n, engine, game, owns_game
        self.slots = list(range(first, first + n))
        self.streams = numpy.arange(first, first + n, dtype=numpy.int32)
        self.store = self.pending = None

    def close(self):
        if self.owns_game:
            self.game.close()

    # Compatibility only.  Until this class a group was a dict (the native one faked it), and code written against that --
    # scripts around ``SelfPlay._live``, the previous revision's tests -- reads ``g["slots"]`` / ``g.get("pending")``.  Nothing
    # in the package does; new code reads the attributes (tests/test_selfplay_refill.py pins that both spellings agree).
    def __getitem__(self, key):
        try:
            return getattr(self, key)
        except AttributeError:
            raise KeyError(key) from None

    def get(self, key, default=None):
        return getattr(self, key, default)


class ObjectGroup(SlotGroup):
    """A group of per-object games: ``batch`` [n] holds their current observations, ``moved`` [n] their last actions (0 for
    a game that just began), ``temps`` [n] the temperatures they began under; ``streams_before``: the streams' states before
    a search that may be dropped (``SelfPlay._drain_searches``)."""

    def __init__(self, first, n, engine, observation_shape, temperature):
        super().__init__(first, n, engine)
        self.batch = numpy.empty((n,) + tuple(observation_shape), numpy.float32)
        self.moved = numpy.zeros(n, numpy.int32)
        self.temps = numpy.full(n, float(temperature))


class BatchedGroup(SlotGroup):
    """
    A group of slots of a shard behind the batched plugin protocol (``SelfPlay._rounds_batched``): its game object,
    engine, streams, frame store and the LOG of the games in progress -- ring arrays [row][slot], row = round % capacity,
    a move is one contiguous row per field (a game lasts at most ``max_moves`` rounds, so its rows never collide; the
    ring starts small and grows to that bound when a game outlasts it); a finished game's rows are copied out as they
    lie (move-major) and viewed game by game -- no transposition on the actor's path.
    """

    def __init__(self, actor, game, first, n, engine, temperature):
        cfg = actor.config
        super().__init__(first, n, engine, game, owns_game=game is not actor.batched_game)
        obs = numpy.asarray(game.reset())
        assert obs.shape == (n,) + tuple(cfg.observation_shape), \
            f"Observation should match the observation_shape defined in MuZeroConfig. Expected {(n,) + tuple(cfg.observation_shape)} but got {obs.shape}."
        self.everyone, self.obs, self.tp = numpy.arange(n), obs, numpy.asarray(game.to_play()).astype(numpy.int64)
        self.start, self.temps, self.round, self.legal = numpy.zeros(n, numpy.int64), numpy.full(n, float(temperature)), 0, None
        self.counter = int(actor.draw_counter)      # (device draws: the counter of the group's next search)
        self.A, self.max_moves = len(cfg.action_space), int(cfg.max_moves)
        self.ring, self.cap = None, 0
        if cfg.stacked_observations > 0:   # frames stay in HBM; the stacked inputs are assembled there (csrc/mzx_obs.h)
            whole = n == actor.num_games
            self.store = actor._frame_store(n) if whole else observations_mod.FrameStore(cfg, n, actor.model.backend)
            self.store.push(obs, None)

    def _row(self, r, obs, reward):
        """Ring row of round ``r``; allocates / grows the ring so that the rounds of every running game keep their own."""
        need = r - int(self.start.min()) + 1
        if need > self.cap:
            row_bytes = max(1, obs.nbytes)      # (large observations: start with a ring of at most ~256 MB of frames)
            first = max(2, min(16, (256 << 20) // row_bytes))
            cap = min(max(2 * self.cap, need, first), self.max_moves + 1)
            n, A = self.n, self.A
            obs_dtype, rew_dtype = obs.dtype, reward.dtype
            if self.ring is not None:        # rows already logged keep their precision (a plugin may return floats in
                # one round and ints in the next: the copy below must not truncate the earlier rows -- ADVICE r5)
                obs_dtype = numpy.result_type(self.ring["obs"].dtype, obs_dtype)
                rew_dtype = numpy.result_type(self.ring["rew"].dtype, rew_dtype)
            ring = dict(obs=numpy.empty((cap, n) + obs.shape[1:], obs_dtype), tp=numpy.empty((cap, n), numpy.int64),
                        act=numpy.empty((cap, n), numpy.int64), rew=numpy.empty((cap, n), rew_dtype),
                        vis=numpy.empty((cap, n, A), numpy.int32), val=numpy.empty((cap, n), numpy.float64), mask=None)
            if self.ring is not None:
                if self.ring["mask"] is not None:
                    ring["mask"] = numpy.ones((cap, n, A), bool)
                for q in range(int(self.start.min()), r):
                    for name, arr in ring.items():
                        if arr is not None:
                            arr[q % cap] = self.ring[name][q % self.cap]
            self.ring, self.cap = ring, cap
        for name, value in (("obs", obs), ("rew", reward)):      # a plugin may return ints in one round and floats in another
            have = self.ring[name].dtype
            if value.dtype != have and numpy.result_type(value.dtype, have) != have:
                self.ring[name] = self.ring[name].astype(numpy.result_type(value.dtype, have))
        return r % self.cap

    def move_temps(self, temperature_threshold):
        """The temperature of every slot's next move."""
        return move_temperature(self.temps, self.round - self.start + 1, temperature_threshold)

    def play(self, actor, result, temperature, temperature_threshold):
        """One move of every slot after its search: action draw, game step, log, finished games out, slots refilled."""
        cfg, g, n, A = actor.config, self.game, self.n, self.A
        r, start, store = self.round, self.start, self.store
        moves_before = r - start                      # len(action_history) - 1 of every slot's game
        if actor.device_draws:                        # drawn on the device behind the search (csrc/mzx_draws.h)
            actions = numpy.asarray(result.actions, numpy.int64)
        else:
            actions = numpy.asarray(actor._select_actions_bank(result, self.streams, self.move_temps(temperature_threshold)),
                                    numpy.int64)
        obs2, reward, done = g.step(actions, None)
        obs2, reward = numpy.asarray(obs2), numpy.asarray(reward)
        c = self._row(r, self.obs, reward)
        ring = self.ring
        ring["obs"][c], ring["tp"][c], ring["act"][c], ring["rew"][c] = self.obs, self.tp, actions, reward
        ring["vis"][c], ring["val"][c] = result.visit_counts, result.root_values
        mask = legal_mask_row(self.legal, self.everyone, n, A)
        if mask is not None and ring["mask"] is None:
            ring["mask"] = numpy.ones((self.cap, n, A), bool)
        if ring["mask"] is not None:
            ring["mask"][c] = True if mask is None else mask
        tp2 = numpy.asarray(g.to_play()).astype(numpy.int64)
        over = numpy.asarray(done, bool) | (moves_before + 2 > cfg.max_moves)     # len(action_history) <= max_moves, :129
        pushed = actions
        finished, slots = [], []
        if over.any():
            idx = numpy.nonzero(over)[0]
            finished = self._harvest(idx, r, obs2[idx], tp2[idx])
            slots = (idx + self.first).tolist()
            if not obs2.flags.writeable or obs2 is self.obs:
                obs2 = obs2.copy()
            obs2[idx] = numpy.asarray(g.reset_games(idx))       # the slots' next games begin (self_play.py:31-52)
            tp2 = numpy.asarray(g.to_play()).astype(numpy.int64)
            start[idx] = r + 1
            self.temps[idx] = float(temperature)
            pushed = actions.copy()
            pushed[idx] = 0
            if store is not None:
                store.clear_history(idx)
        if store is not None:
            store.push(obs2, pushed)
        self.obs, self.tp = obs2, tp2
        self.round = r + 1
        return finished, slots

    def _harvest(self, idx, r, final_obs, final_tp):
        """GameHistory views of the games of slots ``idx`` that ended with round ``r``: per starting round one record of
        the ring rows as they lie."""
        A, ring, cap = self.A, self.ring, self.cap
        out = [None] * len(idx)
        starts = self.start[idx]
        for st in numpy.unique(starts):
            where = numpy.nonzero(starts == st)[0]
            slots = idx[where]
            n = r - int(st) + 1
            rows = numpy.arange(int(st), r + 1) % cap
            everyone = slots.size == self.n
            contiguous = rows[-1] - rows[0] == n - 1               # the game's rounds did not wrap around the ring
            if everyone and contiguous:
                take = lambda a: a[rows[0]: rows[0] + n]           # (a view: copied into the record's arrays below)
            elif everyone:
                take = lambda a: a[rows]
            else:
                take = lambda a: a[rows[:, None], slots[None, :]]
            k = slots.size
            obs_all = numpy.empty((n + 1, k) + ring["obs"].shape[2:], ring["obs"].dtype)
            obs_all[:n], obs_all[n] = take(ring["obs"]), final_obs[where]
            acts = numpy.zeros((n + 1, k), numpy.int64)
            acts[1:] = take(ring["act"])
            rews = numpy.zeros((n + 1, k), ring["rew"].dtype)
            rews[1:] = take(ring["rew"])
            tps = numpy.empty((n + 1, k), numpy.int64)
            tps[:n], tps[n] = take(ring["tp"]), final_tp[where]
            legal_mask = None if ring["mask"] is None else numpy.array(take(ring["mask"]))
            views = shard_views(A, obs_all, acts, rews, tps, numpy.array(take(ring["vis"])), numpy.array(take(ring["val"])),
                                legal_mask, [n] * k, time_major=True)       # (copies: the ring rows are written again)
            if k == len(idx):
                return views
            for j, w in enumerate(where):
                out[w] = views[j]
        return out
