"""
Hand-off of finished games to the replay buffer (first "next" row).

The stock ``ReplayBuffer.save_game`` (/root/reference/replay_buffer.py:33-65) computes the initial
prioritised-replay priorities of a game with a Python double loop -- every position x ``td_steps``
rewards (``compute_target_value``, :230-262): ~10 ms per 500-move game, i.e. tens of seconds for a shard
of thousands of games, far more than playing them.  ``fill_initial_priorities`` computes the SAME numbers
(same binary64 operations in the same order per position; the loop over the reward horizon is a vector
operation over all positions) and stores them on the ``GameHistory``; ``save_game`` then takes its
"priorities already present" branch (:35-37).  The stock buffer and trainer stay untouched.

``Reanalyse`` (section 8f, second row) mirrors the reference worker of the same name
(replay_buffer.py:306-373): same constructor and ``reanalyse(replay_buffer, shared_storage)`` loop, with the
per-game work -- stacked observations of every position, one batched ``initial_inference``, value decode --
on the device (``mzx.observations.stack_history`` + the network kernels + ``mzx_support_to_scalar``).

``DeviceGameStore`` keeps finished games in HBM (a ragged pool, csrc/mzx_replay.h) so that ``ReplayBuffer(...,
device_store=store).get_batch()`` assembles the trainer's tensors on the device (``mzx_replay_batch``): the draws stay
numpy's, in the reference's order, and only fill index arrays.  ``trainer_tensors`` is the binding line of a trainer.
``DeviceGameStore.reanalyse`` / ``Reanalyse.reanalyse_store`` re-evaluate every resident game in a sweep: a handful of
launches per chunk of positions, the decoded values written straight into the pool (opt-in: ``config.reanalyse_sweep``).
``DeviceGameStore.reanalyse_search`` (``config.reanalyse_search``) SEARCHES every resident position again instead and
refreshes the policy targets together with the root values, in place; ``ReplayBuffer.sync_targets`` writes them back.
A store built with ``max_games`` also holds the PER priorities and a game table: ``ReplayBuffer(..., device_sampler=True)``
then DRAWS the batch on the device (``mzx_replay_sample``, a counter-based generator -- not numpy's draws, hence opt-in)
and scatters the trainer's priorities back there (``mzx_replay_update_priorities``).
"""
import ctypes
import time

import numpy
import torch

from . import _lib, models, observations
from .history import ShardGameHistory, _PieceRecord, _ShardRecord, gc_paused, positions_of

# DeviceGameStore.reanalyse: the stacked observations of one chunk of positions stay within this many bytes (the network's
# activations scale with the same count), and within the 64-lane groups one mzx_replay_batch gather accepts
# (csrc/mzx_lib.cpp replay_obs_launch)
REANALYSE_CHUNK_BYTES = 512 << 20
REPLAY_GATHER_GROUPS = 1 << 26
# DeviceGameStore.add_records: staged bytes per upload + mzx_replay_ingest pair.  add_many sends a run of up to 1 << 22 frame
# floats (16 MiB) as one upload; the bulk path stages every column of a game, so its block is four of those: a whole
# cartpole or connect4 hand-off of thousands of games is one pair, image games split every few hundred frames
INGEST_CHUNK_BYTES = 4 * 4 * (1 << 22)


def n_step_values(game_history, config):
    """
    compute_target_value (replay_buffer.py:230-262) for every position of a game: float64 array [T].
    Per position the accumulation order is the reference's: bootstrap term first, then the rewards i = 0,
    1, ... each as (+-reward) * discount ** i.
    """
    T = len(game_history.root_values)
    td = int(config.td_steps)
    discount = config.discount
    root_values = (game_history.root_values if game_history.reanalysed_predicted_root_values is None
                   else game_history.reanalysed_predicted_root_values)
    rv = numpy.array([float(v) for v in root_values], dtype=numpy.float64)
    tp = numpy.asarray(game_history.to_play_history)
    rewards = numpy.array([float(r) for r in game_history.reward_history], dtype=numpy.float64)
    n_r = rewards.size
    index = numpy.arange(T)
    # bootstrap: +-root_values[index + td] * discount ** td, or the integer 0
    value = numpy.zeros(T, numpy.float64)
    b = index + td
    has = b < T
    if has.any():
        bi = b[has]
        last = numpy.where(tp[bi] == tp[index[has]], rv[bi], -rv[bi])
        value[has] = last * (discount ** td)
    # rewards: enumerate(reward_history[index + 1 : index + td + 1]) -- truncated at the end of the game
    for i in range(td):
        pos = index + 1 + i
        ok = pos < n_r
        if not ok.any():
            break
        k = index[ok]
        r = rewards[pos[ok]]
        signed = numpy.where(tp[k] == tp[k + i], r, -r)
        value[ok] = value[ok] + signed * (discount ** i)
    return value


def fill_initial_priorities(game_history, config):
    """
    replay_buffer.py:39-51: priorities[i] = |root_value_i - target_value_i| ** PER_alpha (float32) and
    game_priority = max.  No-op (returns False) when PER is off, priorities exist, the game is empty or a
    root value is missing (moves played by an opponent carry None, self_play.py:509-511).
    """
    if not getattr(config, "PER", False) or game_history.priorities is not None:
        return False
    roots = game_history.root_values
    if len(roots) == 0 or any(v is None for v in roots):
        return False
    values = n_step_values(game_history, config)
    alpha = config.PER_alpha
    priorities = [numpy.abs(roots[i] - float(values[i])) ** alpha for i in range(len(roots))]
    game_history.priorities = numpy.array(priorities, dtype="float32")
    game_history.game_priority = numpy.max(game_history.priorities)
    return True


def device_priorities(backend, root_values, to_play, rewards, config, want_targets=False):
    """
    ``mzx_replay_priorities`` (include/mzx.h, csrc/mzx_replay.h): the initial priorities of G games of T positions each
    ON THE DEVICE -- root_values [G][T] binary64 (0 for an unvisited root), to_play / rewards [G][T + 1] as the histories
    hold them.  Returns (priorities float32 [G][T], game_priority float32 [G][, targets binary64 [G][T]]) as host arrays.
    The target values are the reference's bit for bit (binary64 multiply / add in its order, ``discount ** i`` from a
    table filled HERE with Python's own float pow -- the reference's expression, replay_buffer.py:247, :260); the final
    ``** PER_alpha`` is a binary64 sqrt for 0.5 (every shipped configuration), the identity for 1.
    """
    lib, dev = backend.lib, backend.device
    rv = numpy.ascontiguousarray(root_values, dtype=numpy.float64)
    G, T = rv.shape
    td = int(config.td_steps)
    up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
    d_rv = up(rv)
    d_rw = up(numpy.ascontiguousarray(rewards, dtype=numpy.float64))
    d_tp = up(numpy.ascontiguousarray(to_play, dtype=numpy.int32))
    d_pw = up(numpy.array([config.discount ** i for i in range(td + 1)], dtype=numpy.float64))
    assert d_rw.shape == (G, T + 1) and d_tp.shape == (G, T + 1)
    d_pri, d_top = backend.empty((G, T), torch.float32), backend.empty((G,), torch.float32)
    d_tg = backend.empty((G, T), torch.float64) if want_targets else None
    lib.check(lib.mzx_replay_priorities(backend.ptr(d_rv), backend.ptr(d_rw), backend.ptr(d_tp), G, T, td, backend.ptr(d_pw),
                                        float(config.PER_alpha), backend.ptr(d_tg), backend.ptr(d_pri), backend.ptr(d_top),
                                        backend.stream()))
    out = (d_pri.cpu().numpy(), d_top.cpu().numpy())
    return out + (d_tg.cpu().numpy(),) if want_targets else out


def fill_initial_priorities_many(histories, config, backend=None):
    """
    ``fill_initial_priorities`` for the games a self-play shard hands out together, in ONE pass per group of games of the
    same length: the loop over the reward horizon (``td_steps`` iterations of a dozen numpy statements) runs once per
    group instead of once per game -- 4096 cartpole games cost one game's worth of interpreter time (per game it was
    0.4 ms, twenty times what playing the game's 32 moves costs).  Groups: games that are still VIEWS of one shard record
    (``mzx.self_play.ShardGameHistory``, the batched protocol: the record's arrays are used as they are), and ordinary
    ``GameHistory`` objects of equal length (the per-object plugin surface: their lists are stacked).  Same binary64
    operations in the same order per position, the power through the same scalar ``pow``, the same float32 rounding:
    bit-identical to the per-game function (tests/test_replay_handoff.py).  Games the per-game function would skip
    (priorities present, a missing root value) or treat differently (reanalysed values) go through it one by one.
    Returns the number of games that got priorities.

    ``backend`` (a ``mzx._lib.Backend``: what ``SelfPlay.continuous_self_play`` passes): the groups are computed ON THE
    DEVICE (``device_priorities``: one upload of a group's root values / rewards / to_play, one kernel, one download) --
    the horizon loop and the power leave the interpreter altogether; same float32 priorities
    (tests/test_replay_handoff.py on the serial build, tests/test_gpu_parity.py on the device against the reference's
    own save_game outputs).
    """
    if not getattr(config, "PER", False):
        return 0
    filled, views, plain = 0, {}, {}
    jobs = []
    grouped = getattr(histories, "records", None)
    if grouped and any(getattr(record, "on_device", False) for record, _, _ in grouped):
        # records whose games are still on the device (config.device_handoff): the ingest computes their priorities there,
        # nothing of them is fetched for it; whatever else the hand-off holds goes game by game
        skip = {id(h) for record, _, members in grouped if getattr(record, "on_device", False) for h in members}
        rest = [h for h in histories if id(h) not in skip]
        return fill_initial_priorities_many(rest, config, backend) if rest else 0
    if (grouped and all(record.priorities is not None for record, _, _ in grouped)
            and sum(len(members) for _, _, members in grouped) == len(histories)):
        return 0        # (every record came with its priorities: the views were created with their rows)
    if grouped and backend is not None and all(len(h.__dict__) == 2 for _, _, members in grouped for h in members) and all(
            record.priorities is None for record, _, _ in grouped):
        # the shard's own grouping (mzx.self_play.ShardGames): fresh views of whole records, in record order (nothing of them
        # materialised or assigned yet) -- the record's arrays as they lie, the result stored ON the record: a view
        # resolves its row of it on first access (ShardGameHistory._PER); nothing is done per game
        for record, T, members in grouped:
            if T > 0:
                k = len(members)
                rv = numpy.where(record.totals[:k, :T] > 0, record.vals[:k, :T], 0.0)        # root.value() or 0
                record.priorities, record.game_priority = device_priorities(backend, rv, record.tps[:k, : T + 1],
                                                                            record.rews[:k, : T + 1], config)
                filled += k
        if sum(len(m) for _, _, m in grouped) == len(histories):
            histories = ()
        else:
            done = {id(h) for _, _, members in grouped for h in members}
            histories = [h for h in histories if id(h) not in done]
    for h in histories:
        if h.priorities is not None:
            continue
        view = h.__dict__.get("_view")
        if h.reanalysed_predicted_root_values is not None:
            filled += bool(fill_initial_priorities(h, config))
        elif view is not None and view[2] > 0 and not any(name in h.__dict__ for name in ("root_values", "reward_history",
                                                                                           "to_play_history")):
            views.setdefault((id(view[0]), view[2]), (view[0], view[2], []))[2].append((h, view[1]))
        else:
            roots = h.root_values
            if len(roots) == 0 or len(h.reward_history) != len(roots) + 1 or len(h.to_play_history) != len(roots) + 1:
                filled += bool(fill_initial_priorities(h, config))      # (empty, or not a finished game's shape)
            else:
                plain.setdefault(len(roots), []).append(h)
    for record, T, members in views.values():
        rows = numpy.array([i for _, i in members])
        rv = numpy.where(record.totals[rows, :T] > 0, record.vals[rows, :T], 0.0).astype(numpy.float64)   # root.value() or 0
        jobs.append((rv, numpy.asarray(record.tps[rows, : T + 1]), numpy.asarray(record.rews[rows, : T + 1]).astype(numpy.float64),
                     [h for h, _ in members]))
    for T, members in plain.items():
        if len(members) < 4:       # (nothing to share)
            for h in members:
                filled += bool(fill_initial_priorities(h, config))
            continue
        with gc_paused():
            roots = [h.root_values for h in members]
            if any(v is None for row in roots for v in row):      # opponent moves carry None (self_play.py:509-511)
                keep = [h for h, row in zip(members, roots) if not any(v is None for v in row)]
                roots = [h.root_values for h in keep]
                members = keep
            if not members:
                continue
            jobs.append((numpy.array(roots, dtype=numpy.float64), numpy.array([h.to_play_history for h in members]),
                         numpy.array([h.reward_history for h in members], dtype=numpy.float64), members))
    td, discount, alpha = int(config.td_steps), config.discount, config.PER_alpha
    for rv, tp, rewards, members in jobs:
        k, T = rv.shape
        if backend is not None:
            priorities, top = device_priorities(backend, rv, tp, rewards, config)
            with gc_paused():
                for h, p, t in zip(members, priorities, top):      # (rows of the downloaded array: nothing else refers to it)
                    d = h.__dict__
                    d["priorities"] = p
                    d["game_priority"] = t
            filled += k
            continue
        value = numpy.zeros((k, T), numpy.float64)
        m = T - td
        if m > 0:          # bootstrap: +-root_values[index + td] * discount ** td
            value[:, :m] = numpy.where(tp[:, td:td + m] == tp[:, :m], rv[:, td:td + m], -rv[:, td:td + m]) * (discount ** td)
        same, term = numpy.empty((k, T), bool), numpy.empty((k, T), numpy.float64)
        for i in range(td):      # rewards index + 1 + i, truncated at the end of the game
            m = T - i
            if m <= 0:
                break
            # value[:m] + where(to_play[k] == to_play[k + i], r, -r) * discount ** i, in two reused buffers (a dozen
            # half-megabyte temporaries per iteration cost more in page faults than the arithmetic)
            r, sg = rewards[:, 1 + i: 1 + i + m], term[:, :m]
            numpy.equal(tp[:, :m], tp[:, i:i + m], out=same[:, :m])
            numpy.negative(r, out=sg)
            numpy.copyto(sg, r, where=same[:, :m])
            sg *= (discount ** i)
            value[:, :m] += sg
        with gc_paused():
            gaps = numpy.abs(rv - value).ravel().tolist()
            priorities = numpy.array([g ** alpha for g in gaps], dtype="float32").reshape(k, T)   # the scalar pow, as :44
            top = priorities.max(axis=1)
            for j, h in enumerate(members):
                h.priorities = priorities[j].copy()
                h.game_priority = top[j]
        filled += k
    return filled


class StoreFull(RuntimeError):
    """The pool of a ``DeviceGameStore`` has no contiguous room for the game(s): release older games first."""


class DeviceGameStore:
    """
    Finished games resident on the device, for ``ReplayBuffer(..., device_store=...)`` and ``Reanalyse``.

    One RAGGED pool of ``max_positions`` rows (include/mzx.h ``mzx_replay_pool``): a game of T searched positions takes
    T + 1 contiguous rows -- one per history index -- of the columns frames [C][H][W] fp32, actions i32, rewards f64,
    to_play i32, root_values f64 (the reanalysed values when the history carries them, as ``n_step_values`` reads them),
    child_visits [A] f64 and the derived n-step ``values`` f64 (``mzx_replay_values``: compute_target_value bit for bit).
    The allocator is circular because the stock buffer only ever evicts its oldest game (replay_buffer.py:58-61): a new
    game goes to the head, wraps to row 0 when the room up to the end of the pool is too short, and the rows of the
    oldest resident games are what a release gives back.  ``games`` maps game_id -> (base, T) in allocation order.
    A game is uploaded ONCE (``add`` / ``add_many``); batches are gathered from the pool (``batch``, ``stacked``).

    ``max_games`` (a sensible value: ``config.replay_buffer_size``) adds the state of the device-side sampler
    (include/mzx.h ``mzx_replay_sampler``): ``priorities`` f32 [rows] (row base + i: position i; the padding row stays 0),
    ``owner`` i32 [rows] (scratch of the scatter, -1 between calls) and a table of ``max_games`` slots, slot = game_id %
    max_games -- ``slot_game`` (-1: empty), ``slot_base``, ``slot_len``, ``slot_priority`` (the game's largest priority)
    and ``slot_sum`` (their binary64 sum).  Game ids only grow and the stock buffer holds a contiguous range of them, so
    a buffer of at most ``max_games`` games never collides; a game whose slot is held by a resident game raises
    ``StoreFull``.  ``add_many`` uploads ``game_history.priorities`` (nothing with PER off: the columns stay 0) and
    refreshes the slots of the ingested games in one launch; ``drop`` empties the slot; slot changes are batched on the
    host and flushed with one small upload before the next launch that reads the table; ``update`` leaves priorities
    alone.  ``sample`` / ``update_priorities`` / ``priorities_of`` are the sampler's surface.  Without ``max_games`` none
    of this is allocated.

    ``legal_masks=True`` adds the legal-mask column of ``reanalyse_search``: u32 [rows][ceil(A / 32)], bit ``a`` of a row
    set when action ``a`` is legal at that position.  ``add_many`` fills it from ``game_history.legal_actions`` (T lists,
    what ``SelfPlay`` records with ``config.reanalyse_search``); a history WITHOUT the attribute gets all-ones rows, i.e.
    every action is treated as legal -- the store cannot tell such a history from one of a game whose positions really
    offer every action, so feed a game with fewer legal actions than ``A`` only histories that carry the attribute.  The
    sweep's roots see the legal actions in increasing action order.  Without the flag nothing is allocated and every
    action is legal at every root.
    """

    def __init__(self, config, backend, max_positions, max_games=None, legal_masks=False):
        self.config, self.backend = config, backend
        self.shape = tuple(int(v) for v in config.observation_shape)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ValueError("observation_shape must be (channels, height, width)")
        self.A = len(config.action_space)
        self.k = int(config.stacked_observations)
        self.rows = int(max_positions)
        if self.rows < 1 or self.A < 1:
            raise ValueError("max_positions and the action space must be positive")
        z = backend.zeros
        self.frames = z((self.rows,) + self.shape, torch.float32)
        self.actions, self.to_play = z((self.rows,), torch.int32), z((self.rows,), torch.int32)
        self.rewards, self.root_values, self.values = (z((self.rows,), torch.float64) for _ in range(3))
        self.child_visits = z((self.rows, self.A), torch.float64)
        self.sample_shape = (self.shape[0] * (self.k + 1) + self.k,) + self.shape[1:]
        # the optional legal-mask column of reanalyse_search: u32 words held as int32 (the same bits)
        self.mask_words = -(-self.A // 32)
        self.legal_mask = z((self.rows, self.mask_words), torch.int32) if legal_masks else None
        self.search_sweep_counter = 0      # reanalyse_search calls so far: the counter of the sweep's tie-break stream
        pool = self.pool = _lib.ReplayPool()
        pool.d_frames, pool.d_actions, pool.d_rewards = self.frames.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr()
        pool.d_to_play, pool.d_root_values = self.to_play.data_ptr(), self.root_values.data_ptr()
        pool.d_child_visits, pool.d_values = self.child_visits.data_ptr(), self.values.data_ptr()
        pool.rows, pool.action_space_size = self.rows, self.A
        pool.channels, pool.height, pool.width = self.shape
        td = int(config.td_steps)
        self._discount_pow = self._up(numpy.array([config.discount ** i for i in range(td + 1)], dtype=numpy.float64))
        self.games = {}       # game_id -> (base, T), oldest allocation first
        self._with_positions = 0      # resident games of T > 0 (what the sampler can draw from)
        self._head = 0        # next free row
        # add_records: the pinned staging block, its device twin and the event recorded behind the last ingest that read it
        self._stage = self._stage_dev = self._stage_event = None
        self.ingest_calls = 0         # mzx_replay_ingest calls so far (add_records: one per staged chunk)
        self.export_calls = 0         # mzx_replay_export calls so far (download_games: one per call)
        self.max_games = None if max_games is None else int(max_games)
        self.sampler = None
        if self.max_games is not None:
            if self.max_games < 1:
                raise ValueError("max_games must be positive")
            slots = self.max_games
            self.priorities, self.owner = z((self.rows,), torch.float32), torch.full((self.rows,), -1, dtype=torch.int32,
                                                                                   device=backend.device)
            self.slot_game = torch.full((slots,), -1, dtype=torch.int64, device=backend.device)
            self.slot_base, self.slot_len = z((slots,), torch.int64), z((slots,), torch.int32)
            self.slot_priority, self.slot_sum = z((slots,), torch.float32), z((slots,), torch.float64)
            self._tile_prefix = z((2 * -(-slots // 256),), torch.float64)
            self._raw = z((1,), torch.float64)
            self._slot_owner = {}      # slot -> game_id of the resident game (host mirror of slot_game)
            self._slot_dirty = {}      # slot -> (game_id, base, T) not yet uploaded
            space = [int(a) for a in config.action_space]
            self._action_space = None if space == list(range(self.A)) else self._up(numpy.array(space, dtype=numpy.int32))
            sampler = self.sampler = _lib.ReplaySampler()
            sampler.d_priorities, sampler.d_owner = self.priorities.data_ptr(), self.owner.data_ptr()
            sampler.d_slot_game, sampler.d_slot_base, sampler.d_slot_len = (self.slot_game.data_ptr(), self.slot_base.data_ptr(),
                                                                            self.slot_len.data_ptr())
            sampler.d_slot_priority, sampler.d_slot_sum = self.slot_priority.data_ptr(), self.slot_sum.data_ptr()
            sampler.rows, sampler.slots = self.rows, slots
            sampler.d_tile_prefix, sampler.d_raw, sampler.raw_capacity = self._tile_prefix.data_ptr(), self._raw.data_ptr(), 1

    def __contains__(self, game_id):
        return game_id in self.games

    def __len__(self):
        return len(self.games)

    def _up(self, array):
        return torch.from_numpy(array).to(self.backend.device, non_blocking=True)

    # ---- allocator
    def _find(self, n, head, tail):
        """Base of n contiguous free rows given the head and the base of the oldest resident game (None: empty), or None."""
        if n > self.rows:
            return None
        if tail is None:
            return 0
        if head > tail:                     # free: [head, rows) and [0, tail)
            if self.rows - head >= n:
                return head
            return 0 if tail >= n else None
        return head if tail - head >= n else None      # wrapped (or full): free is [head, tail)

    def _place(self, lengths):
        """Bases for games of the given T, allocated in order; raises StoreFull and leaves the store as it was."""
        head = self._head
        tail = next(iter(self.games.values()))[0] if self.games else None
        bases = []
        for T in lengths:
            base = self._find(T + 1, head, tail)
            if base is None:
                raise StoreFull(f"no room for a game of {T} positions in a pool of {self.rows} rows")
            bases.append(base)
            head = base + T + 1
            if tail is None:
                tail = base
        self._head = head
        return bases

    def drop(self, game_id):
        """Release a game's rows.  Rows come back when every OLDER game has been released too (the tail moves on)."""
        self._with_positions -= self.games[game_id][1] > 0
        del self.games[game_id]
        if self.sampler is not None:
            slot = game_id % self.max_games
            del self._slot_owner[slot]
            self._slot_dirty[slot] = (-1, 0, 0)

    # ---- ingest
    def _columns(self, gh):
        T = len(gh.root_values)
        if not (len(gh.observation_history) == len(gh.action_history) == len(gh.reward_history) == len(gh.to_play_history) == T + 1):
            raise ValueError("not a finished game: the histories must have len(root_values) + 1 entries")
        roots = gh.root_values if gh.reanalysed_predicted_root_values is None else gh.reanalysed_predicted_root_values
        visits = numpy.zeros((T + 1, self.A), numpy.float64)
        if T:
            visits[:T] = numpy.array(gh.child_visits, dtype=numpy.float64).reshape(T, self.A)
        return (numpy.array([int(a) for a in gh.action_history], dtype=numpy.int32),
                numpy.array([float(r) for r in gh.reward_history], dtype=numpy.float64),
                numpy.array([int(p) for p in gh.to_play_history], dtype=numpy.int32),
                numpy.array([float(v) for v in roots] + [0.0], dtype=numpy.float64), visits)

    def _mask_rows(self, gh, T):
        """The T + 1 rows of the legal-mask column of a game: bit a of a row set when action a is legal at that position
        (``game_history.legal_actions``, T lists); all-ones -- the full action space -- for a history without the attribute
        and for the padding row T."""
        rows = numpy.full((T + 1, self.mask_words), 0xFFFFFFFF, numpy.uint32)
        legal = getattr(gh, "legal_actions", None)
        if legal is None:
            return rows.view(numpy.int32)
        if len(legal) != T:
            raise ValueError("legal_actions must hold one list per searched position")
        rows[:T] = 0
        for t, actions in enumerate(legal):
            acts = numpy.asarray(actions, dtype=numpy.int64).reshape(-1)
            if acts.size and (acts.min() < 0 or acts.max() >= self.A):
                raise ValueError("legal_actions outside the action space")
            numpy.bitwise_or.at(rows[t], acts >> 5, (numpy.uint32(1) << (acts & 31).astype(numpy.uint32)))
        return rows.view(numpy.int32)

    def _run_values(self, entries):
        be, lib = self.backend, self.backend.lib
        base = self._up(numpy.array([b for b, _ in entries], dtype=numpy.int64))
        length = self._up(numpy.array([T for _, T in entries], dtype=numpy.int32))
        lib.check(lib.mzx_replay_values(ctypes.byref(self.pool), be.ptr(base), be.ptr(length), len(entries),
                                        int(self.config.td_steps), be.ptr(self._discount_pow), be.stream()))

    def add(self, game_id, game_history):
        self.add_many([(game_id, game_history)])

    def add_many(self, items):
        """
        Ingest the games [(game_id, game_history), ...] of one hand-off: per contiguous run of rows ONE upload per column
        (two runs when the allocation wraps), then ONE values launch for all of them.  Raises StoreFull -- with the store
        unchanged -- when they do not fit.
        """
        items = list(items)
        if not items:
            return
        for game_id, _ in items:
            if game_id in self.games:
                raise ValueError(f"game {game_id} is already resident")
        columns = [self._columns(gh) for _, gh in items]
        lengths = [len(gh.root_values) for _, gh in items]
        if self.legal_mask is not None:
            masks = [self._mask_rows(gh, T) for (_, gh), T in zip(items, lengths)]
        if self.sampler is not None:
            priorities = [self._priority_rows(gh, T) for (_, gh), T in zip(items, lengths)]
            taken = dict(self._slot_owner)
            for game_id, _ in items:
                if taken.setdefault(game_id % self.max_games, game_id) != game_id:
                    raise StoreFull(f"slot {game_id % self.max_games} of game {game_id} is held by resident game "
                                    f"{taken[game_id % self.max_games]} ({self.max_games} slots)")
        bases = self._place(lengths)
        for (game_id, _), base, T in zip(items, bases, lengths):
            self.games[game_id] = (base, T)
            self._with_positions += T > 0
            if self.sampler is not None:
                self._slot_owner[game_id % self.max_games] = game_id
                self._slot_dirty[game_id % self.max_games] = (game_id, base, T)
        pool_columns = (self.actions, self.rewards, self.to_play, self.root_values, self.child_visits)
        lo = 0
        while lo < len(items):
            hi = lo + 1
            while hi < len(items) and bases[hi] == bases[hi - 1] + lengths[hi - 1] + 1:
                hi += 1
            b0, b1 = bases[lo], bases[hi - 1] + lengths[hi - 1] + 1
            for c, column in enumerate(pool_columns):
                column[b0:b1].copy_(self._up(numpy.concatenate([columns[i][c] for i in range(lo, hi)])))
            if self.sampler is not None and self.config.PER:
                self.priorities[b0:b1].copy_(self._up(numpy.concatenate([priorities[i] for i in range(lo, hi)])))
            if self.legal_mask is not None:
                self.legal_mask[b0:b1].copy_(self._up(numpy.concatenate([masks[i] for i in range(lo, hi)])))
            if (b1 - b0) * int(numpy.prod(self.shape)) < (1 << 22):      # small frames: one upload for the run
                frames = numpy.array([numpy.asarray(o) for i in range(lo, hi) for o in items[i][1].observation_history])
                self.frames[b0:b1].copy_(observations._frames_to_device(self.backend, frames.reshape((b1 - b0,) + self.shape)))
            else:                                                         # whole games through the pinned staging block
                for i in range(lo, hi):
                    self.frames[bases[i]:bases[i] + lengths[i] + 1].copy_(
                        observations._history_to_device(self.backend, items[i][1].observation_history, self.shape))
            lo = hi
        self._run_values(list(zip(bases, lengths)))
        if self.sampler is not None:
            self._flush_slots()
            slots = self._up(numpy.array([g % self.max_games for g, _ in items], dtype=numpy.int32))
            be, lib = self.backend, self.backend.lib
            lib.check(lib.mzx_replay_sampler_refresh(ctypes.byref(self.sampler), be.ptr(slots), len(items), be.stream()))

    # ---- bulk ingest of shard records
    def _fresh_view(self, gh, known=None):
        """The ``(record, row, T)`` of a history that is still a fresh view of a shard record -- nothing of it materialised
        or assigned, no reanalysed values: ``fill_initial_priorities_many``'s test -- else None.  ``known``: the ids of the
        records the hand-off came with."""
        d = gh.__dict__
        view = d.get("_view")
        if view is None or d.get("reanalysed_predicted_root_values") is not None or "legal_actions" in d:
            return None
        if known is not None and id(view[0]) not in known:
            return None
        for name in ShardGameHistory._LAZY:
            if name in d:
                return None
        if view[0].priorities is None and d.get("priorities") is not None:      # (priorities of its own: add_many uploads them)
            return None
        return view

    def add_records(self, items, records=None, chunk_bytes=None):
        """
        ``add_many`` for the games of a shard hand-off -- ``items`` [(game_id, game_history), ...] in hand-off order,
        ``records`` the ``ShardGames.records`` grouping the views came from -- with nothing built per game: the pool ends
        up bit for bit as ``add_many(items)`` leaves it (tests/replay_ingest_cases.py).

        Games that are still FRESH VIEWS of a record (``_fresh_view``) take the bulk path: residency, slots and room are
        checked for the whole hand-off, rows are allocated in the order of ``items`` (the bases ``add_many`` would give),
        the host bookkeeping is filled in, pending slot drops are flushed, and then every record's arrays go into the
        store's pinned staging block AS THEY LIE -- ``record.obs[:k]`` and its siblings, or one fancy-index gather per
        record when only some of its games are handed over; observations become float32 and rewards binary64 on the way --
        followed by ONE upload and ONE ``mzx_replay_ingest`` (three launches: rows, n-step values, slots).  The staging
        block (section by section, each 16-byte aligned: len i32, base / game_id / src1 / src0 i64 per game; observations
        f32, actions i64, rewards f64, to_play i64 per history row; visits i32 [A], root values f64, and optionally the
        legal mask u8 [A] and the priorities f32 per searched position) is owned by the store, grown on demand and guarded
        by an event recorded behind the ingest, which is waited for before the block is overwritten.  A hand-off that
        stages more than ``chunk_bytes`` (default ``INGEST_CHUNK_BYTES``) is split at game boundaries into several such
        pairs.  The bound is approximate: a game is counted with the bytes of its rows, not with the padding that aligns
        the sections, and a single game beyond it travels alone.  There is one block, not two: a chunk is copied into it
        only after the previous chunk's ingest has finished.

        Priorities (a store with ``max_games``, ``config.PER``): a record that carries ``priorities`` has them staged; for one
        without, the kernel computes them (``mzx_replay_priorities``' function) and the host views stay without: the
        device columns are authoritative, ``ReplayBuffer.sync_priorities()`` brings them back.

        Every other game -- a plain ``GameHistory``, a view with a materialised or assigned field -- goes through
        ``add_many``.  A mixed hand-off is ingested in runs: maximal runs of fresh views and of other games, each run in
        turn in ``items`` order, so order and bases are those of ``add_many(items)``.  ``StoreFull`` (no room, or a slot
        held by a resident game) is raised before anything is stored and leaves the store unchanged.
        """
        items = list(items)
        if not items:
            return
        known = {id(record) for record, _, _ in records} if records else None
        views = [self._fresh_view(gh, known) for _, gh in items]
        if not any(v is not None for v in views):
            return self.add_many(items)
        for game_id, _ in items:
            if game_id in self.games:
                raise ValueError(f"game {game_id} is already resident")
        lengths = [len(gh.root_values) if v is None else v[2] for (_, gh), v in zip(items, views)]
        if self.sampler is not None:
            taken = dict(self._slot_owner)
            for game_id, _ in items:
                if taken.setdefault(game_id % self.max_games, game_id) != game_id:
                    raise StoreFull(f"slot {game_id % self.max_games} of game {game_id} is held by resident game "
                                    f"{taken[game_id % self.max_games]} ({self.max_games} slots)")
        head = self._head
        self._place(lengths)          # room for the whole hand-off, or StoreFull with the store unchanged
        self._head = head             # (the runs below allocate the same rows again, in the same order)
        limit = INGEST_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
        lo = 0
        while lo < len(items):
            hi = lo + 1
            while hi < len(items) and (views[hi] is None) == (views[lo] is None):
                hi += 1
            if views[lo] is None:
                self.add_many(items[lo:hi])
            else:
                self._ingest_views(items[lo:hi], views[lo:hi], limit)
            lo = hi

    def _ingest_views(self, items, views, limit):
        """A run of fresh views: allocation and host bookkeeping as add_many, then the staged chunks."""
        self._reserve([(game_id, v[2]) for (game_id, _), v in zip(items, views)])
        self._stage_views(items, views, limit)

    def _reserve(self, entries):
        """The host half of ``add_many`` for games ``[(game_id, T), ...]`` whose rows ``_stage_views`` fills later: the same
        checks in the same order (ValueError for a resident id, StoreFull -- with the store unchanged -- for a slot held
        by a resident game or no room), the same allocation, the same entries in ``games`` and ``_slot_owner``.  The table
        slots are written by the ingest, not through ``_slot_dirty``."""
        for game_id, _ in entries:
            if game_id in self.games:
                raise ValueError(f"game {game_id} is already resident")
        if self.sampler is not None:
            taken = {}
            for game_id, _ in entries:
                slot = game_id % self.max_games
                holder = self._slot_owner.get(slot, taken.setdefault(slot, game_id))
                if holder != game_id:
                    raise StoreFull(f"slot {slot} of game {game_id} is held by resident game {holder} ({self.max_games} slots)")
        bases = self._place([T for _, T in entries])
        for (game_id, T), base in zip(entries, bases):
            self.games[game_id] = (base, T)
            self._with_positions += T > 0
            if self.sampler is not None:
                self._slot_owner[game_id % self.max_games] = game_id

    def _stage_views(self, items, views, limit=None):
        """The device half for reserved games that are fresh views: the staged chunks, each one upload and one ingest."""
        if not items:
            return
        limit = INGEST_CHUNK_BYTES if limit is None else limit
        groups = {}
        sampled, slots = self.sampler is not None, self.max_games
        for (game_id, _), (record, row, T) in zip(items, views):
            base = self.games[game_id][0]
            group = groups.get((id(record), T))
            if group is None:
                group = groups[(id(record), T)] = (record, T, [], [], [])
            group[2].append(row)
            group[3].append(base)
            group[4].append(game_id)
        if sampled:
            for game_id, _ in items:       # (the kernel writes these slots: a pending entry must not overwrite them later)
                self._slot_dirty.pop(game_id % slots, None)
            self._flush_slots()
        F, A = int(numpy.prod(self.shape)), self.A
        per = sampled and bool(self.config.PER)
        chunk, used, carried = [], 0, None
        for record, T, rows, base, ids in groups.values():
            rows, base, ids = numpy.array(rows, dtype=numpy.int64), numpy.array(base, dtype=numpy.int64), numpy.array(ids, dtype=numpy.int64)
            game_bytes = (T + 1) * (4 * F + 24) + T * (5 * A + 12) + 36
            has = None if not (per and T) else record.priorities is not None
            if chunk and has is not None and carried is not None and has != carried:      # staged and computed priorities apart
                self._ingest_chunk(chunk)
                chunk, used, carried = [], 0, None
            carried = has if has is not None else carried
            k, lo = len(rows), 0
            while lo < k:
                room = (limit - used) // game_bytes
                if room < 1:
                    if chunk:
                        self._ingest_chunk(chunk)
                        chunk, used = [], 0
                        continue
                    room = 1          # (a game beyond the limit travels alone)
                hi = min(k, lo + room)
                chunk.append((record, T, rows[lo:hi], base[lo:hi], ids[lo:hi]))
                used += (hi - lo) * game_bytes
                lo = hi
        if chunk:
            self._ingest_chunk(chunk)

    def _staging(self, nbytes):
        """The pinned staging block as a numpy byte array of at least ``nbytes``, free to be overwritten."""
        on_gpu = self.backend.device.type == "cuda"
        if self._stage is None or self._stage.numel() < nbytes:
            capacity = max(nbytes, 2 * (0 if self._stage is None else self._stage.numel()))
            self._stage = torch.empty(capacity, dtype=torch.uint8, pin_memory=on_gpu)
            self._stage_dev = torch.empty(capacity, dtype=torch.uint8, device=self.backend.device)
        elif self._stage_event is not None:
            self._stage_event.synchronize()
        return self._stage.numpy()

    def _ingest_chunk(self, pieces):
        """One upload and one ``mzx_replay_ingest``: ``pieces`` [(record, T, rows of the record, bases, game ids)]."""
        be, lib = self.backend, self.backend.lib
        F, A = int(numpy.prod(self.shape)), self.A
        lens = numpy.concatenate([numpy.full(len(p[2]), p[1], numpy.int64) for p in pieces])
        G = int(lens.size)
        R0 = int(lens.sum())
        R1 = R0 + G
        per = self.sampler is not None and bool(self.config.PER)
        searched = [p for p in pieces if p[1] > 0]
        with_mask = any(p[0].legal_mask is not None for p in searched)
        with_priorities = per and bool(searched) and all(p[0].priorities is not None for p in searched)
        sections = [("len", numpy.int32, G), ("base", numpy.int64, G), ("game_id", numpy.int64, G), ("src1", numpy.int64, G),
                    ("src0", numpy.int64, G), ("obs", numpy.float32, R1 * F), ("acts", numpy.int64, R1), ("rews", numpy.float64, R1),
                    ("tps", numpy.int64, R1), ("vis", numpy.int32, R0 * A), ("vals", numpy.float64, R0)]
        if with_mask:
            sections.append(("mask", numpy.uint8, R0 * A))
        if with_priorities:
            sections.append(("pri", numpy.float32, R0))
        offsets, total = {}, 0
        for name, dtype, count in sections:
            offsets[name] = total
            total = -(-(total + count * numpy.dtype(dtype).itemsize) // 16) * 16
        total = max(total, 16)
        host = self._staging(total)
        col = {name: host[offsets[name]:offsets[name] + count * numpy.dtype(dtype).itemsize].view(dtype)
               for name, dtype, count in sections}
        col["len"][:] = lens
        col["base"][:] = numpy.concatenate([p[3] for p in pieces])
        col["game_id"][:] = numpy.concatenate([p[4] for p in pieces])
        col["src1"][:] = numpy.cumsum(lens + 1) - (lens + 1)
        col["src0"][:] = numpy.cumsum(lens) - lens
        o1 = o0 = 0
        put = lambda dst, src: numpy.copyto(dst, numpy.asarray(src).reshape(dst.shape), casting="unsafe")
        for record, T, rows, _, _ in pieces:
            k = len(rows)
            first = int(rows[0])
            sel = slice(first, first + k) if int(rows[-1]) - first == k - 1 and (k < 3 or bool((numpy.diff(rows) == 1).all())) else rows
            n1, n0 = k * (T + 1), k * T
            put(col["obs"][o1 * F:(o1 + n1) * F].reshape(k, T + 1, F), record.obs[sel, :T + 1])
            put(col["acts"][o1:o1 + n1].reshape(k, T + 1), record.acts[sel, :T + 1])
            put(col["rews"][o1:o1 + n1].reshape(k, T + 1), record.rews[sel, :T + 1])
            put(col["tps"][o1:o1 + n1].reshape(k, T + 1), record.tps[sel, :T + 1])
            if T:
                put(col["vis"][o0 * A:(o0 + n0) * A].reshape(k, T, A), record.vis[sel, :T])
                put(col["vals"][o0:o0 + n0].reshape(k, T), record.vals[sel, :T])
                if with_mask:
                    if record.legal_mask is None:
                        col["mask"][o0 * A:(o0 + n0) * A] = 1
                    else:
                        put(col["mask"][o0 * A:(o0 + n0) * A].reshape(k, T, A), record.legal_mask[sel, :T])
                if with_priorities:
                    put(col["pri"][o0:o0 + n0].reshape(k, T), record.priorities[sel, :T])
            o1, o0 = o1 + n1, o0 + n0
        dev = self._stage_dev
        dev[:total].copy_(self._stage[:total], non_blocking=True)
        at = lambda name: dev.data_ptr() + offsets[name] if name in offsets else None
        io = _lib.ReplayIngestIO()
        io.d_len, io.d_base, io.d_game_id, io.d_src1, io.d_src0 = at("len"), at("base"), at("game_id"), at("src1"), at("src0")
        io.d_observations, io.d_actions, io.d_rewards, io.d_to_play = at("obs"), at("acts"), at("rews"), at("tps")
        io.d_visits, io.d_root_values, io.d_legal_mask, io.d_priorities = at("vis"), at("vals"), at("mask"), at("pri")
        io.d_discount_pow, io.per_alpha = self._discount_pow.data_ptr(), float(getattr(self.config, "PER_alpha", 1.0))
        io.total_rows, io.num_games, io.td_steps, io.per, io.action_space_size = R1, G, int(self.config.td_steps), int(per), A
        io.channels, io.height, io.width = self.shape
        lib.check(lib.mzx_replay_ingest(ctypes.byref(self.pool), None if self.sampler is None else ctypes.byref(self.sampler),
                                        be.ptr(self.legal_mask), self.rows if self.legal_mask is not None else 0,
                                        ctypes.byref(io), be.stream()))
        self.ingest_calls += 1
        if be.device.type == "cuda":
            if self._stage_event is None:
                self._stage_event = torch.cuda.Event()
            self._stage_event.record(torch.cuda.current_stream(be.device))

    # ---- the device hand-off
    def ingest_piece(self, piece, bases, game_ids):
        """
        The games of a piece a resident shard kept on the device (``mzx.native_rounds._Piece``, ``config.device_handoff``)
        become pool rows without touching the host: ONE small upload -- ``bases`` / ``game_ids`` per game of the piece, in
        the piece's order, base -1 for a game that is not to be stored (evicted again within its hand-off: the ingest passes
        it over) -- and ONE ``mzx_replay_ingest`` whose d_len / d_src1 / d_src0 and staged arrays point into the piece;
        then the piece is released behind the ingest.  The rows were reserved by ``_reserve``; the priorities are computed
        by the kernel.
        """
        be, lib = self.backend, self.backend.lib
        G = piece.games
        table = numpy.empty((2, G), numpy.int64)
        table[0], table[1] = bases, game_ids
        if self.sampler is not None:
            for base, game_id in zip(table[0].tolist(), table[1].tolist()):
                if base >= 0:        # (the kernel writes these slots: a pending entry must not overwrite them later)
                    self._slot_dirty.pop(game_id % self.max_games, None)
            self._flush_slots()
        d_table = self._up(table)
        ptr = piece.ptr
        io = _lib.ReplayIngestIO()
        io.d_len, io.d_src1, io.d_src0 = ptr["len"], ptr["src1"], ptr["src0"]
        io.d_base, io.d_game_id = d_table.data_ptr(), d_table.data_ptr() + 8 * G
        io.d_observations, io.d_actions, io.d_rewards, io.d_to_play = ptr["obs"], ptr["acts"], ptr["rews"], ptr["tps"]
        io.d_visits, io.d_root_values, io.d_legal_mask, io.d_priorities = ptr["vis"], ptr["vals"], ptr["mask"], None
        per = self.sampler is not None and bool(self.config.PER)
        io.d_discount_pow, io.per_alpha = self._discount_pow.data_ptr(), float(getattr(self.config, "PER_alpha", 1.0))
        io.total_rows, io.num_games, io.td_steps, io.per, io.action_space_size = piece.rows0 + G, G, int(self.config.td_steps), int(per), self.A
        io.channels, io.height, io.width = self.shape
        lib.check(lib.mzx_replay_ingest(ctypes.byref(self.pool), None if self.sampler is None else ctypes.byref(self.sampler),
                                        be.ptr(self.legal_mask), self.rows if self.legal_mask is not None else 0,
                                        ctypes.byref(io), be.stream()))
        self.ingest_calls += 1
        piece.release(be.stream())
        del d_table      # (torch's caching allocator keeps the block for this stream: the ingest reads it in stream order)

    def game_record(self, game_id, obs_dtype=None, integer_rewards=False):
        """A resident game as a host ``_ShardRecord`` of one game (``download_games``: one export): observations in
        ``obs_dtype``, rewards as integers where the game's are, ``ratios`` the pool's quotients and ``vals`` its root
        values -- the visit counts are not kept, so every row counts as visited and the record hands out its own rows."""
        got = self.download_games([game_id], legal_mask=self.legal_mask is not None, priorities=False)
        T = int(got["lengths"][0])
        obs = got["observations"]
        if obs_dtype is not None and numpy.dtype(obs_dtype) != numpy.float32:
            obs = obs.astype(obs_dtype)
        rews = got["rewards"].astype(numpy.int64) if integer_rewards else got["rewards"]
        mask = got.get("legal_mask")
        legal = None if mask is None or mask.all() else mask.astype(bool)[None]
        return _ShardRecord(self.A, obs[None], got["actions"][None], rews[None], got["to_play"][None], None, got["root_values"][None],
                            numpy.ones((1, T), numpy.int64), got["child_visits"][None], numpy.ones(1, bool), legal)

    # ---- reading games back
    def download_games(self, game_ids, legal_mask=None, priorities=None):
        """
        The resident games ``game_ids`` as host arrays: ONE ``mzx_replay_export`` (a launch that packs their pool rows
        game-major and ragged, the ingest's staged layout) and one download per column, whatever the number of games.
        Returns a dict: ``lengths`` i32 [G]; ``first1`` / ``first0`` i64 [G], the first packed row of every game in the
        arrays of T + 1 and of T entries per game; ``observations`` f32 [sum(T + 1)] + observation_shape, ``actions`` /
        ``to_play`` i64 and ``rewards`` f64 [sum(T + 1)]; ``child_visits`` f64 [sum T][A] -- the pool's quotients, bit
        for bit --, ``root_values`` f64 [sum T] (the pool's column: the reanalysed values after a sweep); and, where the
        store holds the column (``legal_mask`` / ``priorities``: None takes what is there, True insists), ``legal_mask``
        u8 [sum T][A] and ``priorities`` f32 [sum T].  A game that is not resident raises ``LookupError`` naming its id
        before anything is launched.
        """
        be, lib = self.backend, self.backend.lib
        ids = [int(g) for g in game_ids]
        for g in ids:
            if g not in self.games:
                raise LookupError(f"game {g} is not resident in the device store")
        with_mask = self.legal_mask is not None if legal_mask is None else bool(legal_mask)
        with_priorities = self.sampler is not None if priorities is None else bool(priorities)
        if with_mask and self.legal_mask is None:
            raise ValueError("this DeviceGameStore was built without legal_masks")
        if with_priorities:
            self._need_sampler()
        entries = [self.games[g] for g in ids]
        lens = numpy.array([T for _, T in entries], dtype=numpy.int64)
        G, R0 = len(ids), int(lens.sum())
        R1, n0 = R0 + G, max(R0, 1)       # (games without a position: the arrays of T entries still need an address)
        first1, first0 = numpy.cumsum(lens + 1) - (lens + 1), numpy.cumsum(lens) - lens
        table = numpy.empty((3, G), numpy.int64)
        table[0], table[1], table[2] = [b for b, _ in entries], first1, first0
        d_table, d_len = self._up(table), self._up(lens.astype(numpy.int32))
        out = {"observations": be.empty((R1,) + self.shape, torch.float32), "actions": be.empty((R1,), torch.int64),
               "rewards": be.empty((R1,), torch.float64), "to_play": be.empty((R1,), torch.int64),
               "child_visits": be.empty((n0, self.A), torch.float64), "root_values": be.empty((n0,), torch.float64)}
        if with_mask:
            out["legal_mask"] = be.empty((n0, self.A), torch.uint8)
        if with_priorities:
            out["priorities"] = be.empty((n0,), torch.float32)
        io = _lib.ReplayExportIO()
        io.d_base, io.d_dst1, io.d_dst0 = (d_table.data_ptr() + 8 * G * i for i in range(3))
        io.d_len = d_len.data_ptr()
        io.d_observations, io.d_actions, io.d_rewards = (out[n].data_ptr() for n in ("observations", "actions", "rewards"))
        io.d_to_play, io.d_child_visits, io.d_root_values = (out[n].data_ptr() for n in ("to_play", "child_visits", "root_values"))
        io.d_legal_mask = out["legal_mask"].data_ptr() if with_mask else None
        io.d_priorities = out["priorities"].data_ptr() if with_priorities else None
        io.total_rows, io.num_games = R1, G
        lib.check(lib.mzx_replay_export(ctypes.byref(self.pool), None if self.sampler is None else ctypes.byref(self.sampler),
                                        be.ptr(self.legal_mask), self.rows if self.legal_mask is not None else 0,
                                        ctypes.byref(io), be.stream()))
        self.export_calls += 1
        whole = ("observations", "actions", "rewards", "to_play")
        out = {name: t.cpu().numpy()[:R1 if name in whole else R0] for name, t in out.items()}
        out["lengths"], out["first1"], out["first0"] = lens.astype(numpy.int32), first1, first0
        return out

    # ---- the sampler's state
    def _priority_rows(self, gh, T):
        """The T + 1 rows of the priority column of a game: its float32 priorities and the padding 0 (zeros with PER off)."""
        rows = numpy.zeros(T + 1, numpy.float32)
        if self.config.PER and T:
            if gh.priorities is None or len(gh.priorities) != T:
                raise ValueError("with PER a game enters the store with its priorities (fill_initial_priorities before save_game)")
            rows[:T] = numpy.asarray(gh.priorities, dtype=numpy.float32)
        return rows

    def _need_sampler(self):
        if self.sampler is None:
            raise ValueError("this DeviceGameStore was built without max_games: it has no sampler state")

    def _flush_slots(self):
        """The slot changes since the last flush, as ONE upload ([k][4] i64: slot, game, base, T) scattered into the table."""
        if not self._slot_dirty:
            return
        packed = self._up(numpy.array([(s,) + v for s, v in self._slot_dirty.items()], dtype=numpy.int64))
        self._slot_dirty = {}
        index = packed[:, 0]
        self.slot_game.index_copy_(0, index, packed[:, 1])
        self.slot_base.index_copy_(0, index, packed[:, 2])
        self.slot_len.index_copy_(0, index, packed[:, 3].to(torch.int32))

    def priorities_of(self, game_id):
        """(priorities float32 [T], game_priority float32) of a resident game, downloaded."""
        self._need_sampler()
        base, T = self.games[game_id]
        self._flush_slots()
        return (self.priorities[base:base + T].cpu().numpy(),
                numpy.float32(self.slot_priority[game_id % self.max_games].cpu().numpy()))

    def sample(self, n, seed, call_counter, total_samples, per, num_unroll_steps=None, uniforms=None):
        """
        ``mzx_replay_sample``: n draws of the two-level distribution (include/mzx.h) as device tensors ``(base i64 [n], len
        i32 [n], pos i32 [n], absorbing_actions i32 [n, U + 1], game_id i64 [n], weight f32 [n] or None without per)``
        -- the first four are what ``mzx_replay_batch`` takes.  A pure function of the store's state and ``(seed,
        call_counter)``; ``uniforms`` (f64 [n, 2], host or device) replaces the generator's two uniforms per sample.
        Nothing is downloaded and nothing synchronises.  Raises ValueError when no game with a position is resident.
        """
        self._need_sampler()
        be, lib = self.backend, self.backend.lib
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        if not self._with_positions:
            raise ValueError("no game with a position is resident: nothing to draw from")
        self._flush_slots()
        U = int(self.config.num_unroll_steps if num_unroll_steps is None else num_unroll_steps)
        per = bool(per)
        if per and self._raw.numel() < n:
            self._raw = be.empty((n,), torch.float64)
            self.sampler.d_raw, self.sampler.raw_capacity = self._raw.data_ptr(), n
        base, game_id = be.empty((n,), torch.int64), be.empty((n,), torch.int64)
        length, pos = be.empty((n,), torch.int32), be.empty((n,), torch.int32)
        tape = be.empty((n, U + 1), torch.int32)
        weight = be.empty((n,), torch.float32) if per else None
        io = _lib.ReplaySampleIO()
        io.seed, io.call_counter = int(seed) & (2 ** 64 - 1), int(call_counter) & (2 ** 64 - 1)
        io.total_samples, io.num_samples, io.per, io.num_unroll_steps, io.num_actions = int(total_samples), n, int(per), U, self.A
        io.d_action_space = None if self._action_space is None else self._action_space.data_ptr()
        if uniforms is not None:
            if not torch.is_tensor(uniforms):
                uniforms = torch.from_numpy(numpy.ascontiguousarray(uniforms, dtype=numpy.float64))
            uniforms = uniforms.to(be.device, torch.float64).contiguous()
            if tuple(uniforms.shape) != (n, 2):
                raise ValueError("uniforms must be [n, 2]")
            io.d_uniforms = uniforms.data_ptr()
        io.d_base, io.d_len, io.d_pos, io.d_absorbing_actions = base.data_ptr(), length.data_ptr(), pos.data_ptr(), tape.data_ptr()
        io.d_game_id = game_id.data_ptr()
        io.d_weight = None if weight is None else weight.data_ptr()
        lib.check(lib.mzx_replay_sample(ctypes.byref(self.sampler), ctypes.byref(io), be.stream()))
        return base, length, pos, tape, game_id, weight

    def update_priorities(self, new, game_id, pos):
        """
        ``mzx_replay_update_priorities`` (update_priorities, replay_buffer.py:205-228): ``new`` [n, steps] float32 (device
        tensor or array), ``game_id`` i64 [n] / ``pos`` i32 [n] as ``sample`` returned them (or host arrays).  A game that
        has left the store is passed over; where windows overlap the highest sample index wins.
        """
        self._need_sampler()
        be, lib = self.backend, self.backend.lib
        dev = lambda x, dtype: (x if torch.is_tensor(x) else torch.from_numpy(numpy.ascontiguousarray(x))).detach().to(
            be.device, dtype).contiguous()
        new = dev(new, torch.float32)
        if new.dim() != 2:
            raise ValueError("priorities must be [n, steps]")
        game_id, pos = dev(game_id, torch.int64).reshape(-1), dev(pos, torch.int32).reshape(-1)
        n, steps = new.shape
        if game_id.numel() != n or pos.numel() != n:
            raise ValueError("one (game_id, position) per row of priorities")
        self._flush_slots()
        lib.check(lib.mzx_replay_update_priorities(ctypes.byref(self.sampler), be.ptr(new), be.ptr(game_id), be.ptr(pos), n, steps,
                                                   be.stream()))

    def update(self, game_id, game_history):
        """Reanalyse's update_game_history (replay_buffer.py:197-203): new root values, the n-step values recomputed."""
        base, T = self.games[game_id]
        if len(game_history.root_values) != T:
            raise ValueError("update: the game's length changed")
        roots = (game_history.root_values if game_history.reanalysed_predicted_root_values is None
                 else game_history.reanalysed_predicted_root_values)
        if T:
            self.root_values[base:base + T].copy_(self._up(numpy.array([float(v) for v in roots], dtype=numpy.float64)))
            self._run_values([(base, T)])

    # ---- gathers
    def batch(self, game_ids, positions, absorbing_actions=None, num_unroll_steps=None, observations=True, targets=True):
        """
        ``mzx_replay_batch`` for the samples (game_ids[n], positions[n]): returns (observation [n, C', H, W] fp32 or None,
        (value, reward [n, U + 1] f64, policy [n, U + 1, A] f64, action, gradient_scale [n, U + 1] i64) or None) as
        device tensors.  ``absorbing_actions`` [n, U + 1]: the actions drawn for steps past the end of a game.
        """
        be, lib = self.backend, self.backend.lib
        n = len(game_ids)
        entries = [self.games[g] for g in game_ids]
        base = numpy.array([b for b, _ in entries], dtype=numpy.int64)
        length = numpy.array([T for _, T in entries], dtype=numpy.int32)
        pos = numpy.ascontiguousarray(positions, dtype=numpy.int32).reshape(n)
        if n and (pos.min() < 0 or (pos > length).any()):
            raise ValueError("position outside its game")
        U = int(self.config.num_unroll_steps if num_unroll_steps is None else num_unroll_steps)
        tape = None
        if targets:
            tape = self._up(numpy.zeros((n, U + 1), numpy.int32) if absorbing_actions is None else numpy.ascontiguousarray(
                absorbing_actions, dtype=numpy.int32).reshape(n, U + 1))
        return self.gather(self._up(base), self._up(length), self._up(pos), tape, U, observations, targets)

    def gather(self, base, length, pos, tape=None, num_unroll_steps=None, observations=True, targets=True):
        """``batch`` for samples that are already device arrays (base i64 / len i32 / pos i32 [n], tape i32 [n, U + 1]):
        what ``sample`` returns goes in unchanged, no host copy in between.  Without a tape the absorbing steps take action 0."""
        be, lib = self.backend, self.backend.lib
        n = int(base.shape[0])
        if targets and tape is None:
            U = int(self.config.num_unroll_steps if num_unroll_steps is None else num_unroll_steps)
            tape = be.zeros((n, U + 1), torch.int32)
        io = _lib.ReplayBatchIO()
        keep = [base, length, pos]
        io.d_base, io.d_len, io.d_pos = (t.data_ptr() for t in keep)
        io.num_samples, io.stacked_observations = n, self.k
        obs = out = None
        if observations:
            obs = be.empty((n,) + self.sample_shape, torch.float32)
            io.d_observation = obs.data_ptr()
        if targets:
            U = int(self.config.num_unroll_steps if num_unroll_steps is None else num_unroll_steps)
            keep.append(tape)
            value, reward = be.empty((n, U + 1), torch.float64), be.empty((n, U + 1), torch.float64)
            policy = be.empty((n, U + 1, self.A), torch.float64)
            action, scale = be.empty((n, U + 1), torch.int64), be.empty((n, U + 1), torch.int64)
            io.num_unroll_steps, io.d_absorbing_actions = U, keep[-1].data_ptr()
            io.d_value, io.d_reward, io.d_policy = value.data_ptr(), reward.data_ptr(), policy.data_ptr()
            io.d_action, io.d_gradient_scale = action.data_ptr(), scale.data_ptr()
            out = (value, reward, policy, action, scale)
        if n:
            lib.check(lib.mzx_replay_batch(ctypes.byref(self.pool), ctypes.byref(io), be.stream()))
        return obs, out

    def stacked(self, game_id, count=None):
        """get_stacked_observations(i, k, A) for i = 0 .. count-1 (default: every searched position) of a resident game."""
        T = self.games[game_id][1]
        count = T if count is None else int(count)
        return self.batch([game_id] * count, numpy.arange(count), targets=False)[0]

    # ---- reanalyse sweep
    def reanalyse_chunk_limit(self):
        """Positions one ``mzx_replay_batch`` gather accepts (the scalar path's piece count: the smaller bound)."""
        pieces = -(-self.shape[1] * self.shape[2] // 256)
        return max(1, (REPLAY_GATHER_GROUPS - 1) // (self.sample_shape[0] * pieces))

    def reanalyse_chunk_positions(self):
        """Default chunk of ``reanalyse``: REANALYSE_CHUNK_BYTES of stacked observations, within one gather launch."""
        sample_bytes = 4 * int(numpy.prod(self.sample_shape))
        return max(1, min(REANALYSE_CHUNK_BYTES // sample_bytes, self.reanalyse_chunk_limit()))

    def reanalyse(self, model, game_ids=None, chunk_positions=None):
        """
        Reanalyse (replay_buffer.py:343-367) as a SWEEP over resident games -- every one in allocation order, or
        ``game_ids`` --: their positions form one flat sequence that is evaluated under ``model``'s current weights in
        chunks of ``chunk_positions`` (default ``reanalyse_chunk_positions()``), whatever the games' lengths.  Per chunk, on
        the backend's stream: ``mzx_replay_positions`` (the chunk's samples, built on the device), ``mzx_replay_batch`` with
        the observation pointer only, ``model.initial_inference``, ``mzx_replay_reanalyse_write`` (decode, the float32 into
        the sweep's output, its binary64 into the pool's root_values).  Then ONE ``mzx_replay_values`` launch for the games
        swept and ONE download.  Returns {game_id: float32 array [T]} (views of that download) -- what ``reanalyse_game``
        returns per game; the pool is left as ``update`` with those arrays would leave it.  An unknown game raises KeyError;
        no other column is touched.  Host work per sweep is O(games): nothing is built or uploaded per position.
        """
        be, lib = self.backend, self.backend.lib
        ids = list(dict.fromkeys(self.games if game_ids is None else game_ids))
        entries = [self.games[g] for g in ids]
        if not ids:
            return {}
        lengths = numpy.array([T for _, T in entries], dtype=numpy.int64)
        first = numpy.concatenate([[0], numpy.cumsum(lengths)[:-1]]).astype(numpy.int64)
        total = int(lengths.sum())
        if total == 0:
            return {g: numpy.zeros((0,), numpy.float32) for g in ids}
        chunk = self.reanalyse_chunk_positions() if chunk_positions is None else int(chunk_positions)
        if chunk < 1:
            raise ValueError("chunk_positions must be positive")
        chunk = min(chunk, total, self.reanalyse_chunk_limit())
        G = len(ids)
        d_base = self._up(numpy.array([b for b, _ in entries], dtype=numpy.int64))
        d_len, d_first = self._up(lengths.astype(numpy.int32)), self._up(first)
        s_base, s_len, s_pos = be.empty((chunk,), torch.int64), be.empty((chunk,), torch.int32), be.empty((chunk,), torch.int32)
        obs = be.empty((chunk,) + self.sample_shape, torch.float32)
        out = be.empty((total,), torch.float32)
        io = _lib.ReplayBatchIO()
        io.d_base, io.d_len, io.d_pos, io.d_observation = s_base.data_ptr(), s_len.data_ptr(), s_pos.data_ptr(), obs.data_ptr()
        io.stacked_observations = self.k
        support = int(self.config.support_size)
        for lo in range(0, total, chunk):
            n = min(chunk, total - lo)
            lib.check(lib.mzx_replay_positions(be.ptr(d_base), be.ptr(d_len), be.ptr(d_first), G, total, lo, n, be.ptr(s_base),
                                               be.ptr(s_len), be.ptr(s_pos), be.stream()))
            io.num_samples = n
            lib.check(lib.mzx_replay_batch(ctypes.byref(self.pool), ctypes.byref(io), be.stream()))
            value_logits = model.initial_inference(obs[:n])[0]
            lib.check(lib.mzx_replay_reanalyse_write(be.ptr(value_logits), n, support, be.ptr(s_base), be.ptr(s_pos),
                                                     be.ptr(out[lo:lo + n]), be.ptr(self.root_values), be.stream()))
        self._run_values([e for e in entries if e[1] > 0])
        host = out.cpu().numpy()
        return {g: host[f:f + T] for g, f, T in zip(ids, first.tolist(), lengths.tolist())}

    def reanalyse_search(self, engine, game_ids=None, chunk_positions=None, seed=None):
        """
        MuZero Reanalyse with fresh SEARCHES: every position of the resident games -- all of them in allocation order, or
        ``game_ids`` -- is searched again under the current weights of ``engine`` (a ``BatchedMCTS`` over a ``HipNetwork``
        on this store's backend; its ``num_simulations`` and ``max_trees`` are the caller's choice), and the normalised
        visit counts and root values replace the pool's ``child_visits`` and ``root_values`` rows in place.  The positions
        form one flat sequence taken in chunks of ``min(chunk_positions or engine.max_trees, engine.max_trees,
        reanalyse_chunk_limit())``.  Per chunk, on the backend's stream and with nothing built, uploaded or synchronised
        on the host: ``mzx_replay_positions``, ``mzx_replay_batch`` (observation pointer only),
        ``mzx_replay_search_inputs``, ``mzx_search_run``, ``mzx_replay_search_write``.  Then ONE ``mzx_replay_values``
        launch for the games swept and ONE download, of the skipped counter.  Returns ``{"positions", "skipped", "chunks"}``.

        The roots get no exploration noise and draw their tie-breaks from a counter-based stream keyed by ``seed``
        (default ``config.seed``) and the store's ``search_sweep_counter``, which advances by one per sweep run: the targets of a
        sweep are a pure function of the pool, the weights and those two numbers.  A position whose search exhausted its
        tie-break tape or its nodes, or whose legal mask is empty, keeps its old targets and counts as skipped.

        Legal actions: a store built with ``legal_masks=True`` searches every root over the actions its mask row holds, in
        INCREASING action order (the order the ``legal_actions()`` of the reference's tic-tac-toe, connect4 and gomoku
        return); without the column every action is legal at every root.  Priorities are not touched.  An unknown game
        raises KeyError, an engine of another action space or observation size ValueError.
        """
        from .search import TAPE_WORDS

        be, lib = self.backend, self.backend.lib
        if engine.backend is not be:
            raise ValueError("reanalyse_search: the engine must live on the store's backend")
        if engine.A != self.A or int(engine.model.input_size) != int(numpy.prod(self.sample_shape)):
            raise ValueError(f"reanalyse_search: the engine searches {engine.A} actions over {int(engine.model.input_size)} "
                             f"observation floats, the store holds {self.A} and {int(numpy.prod(self.sample_shape))}")
        ids = list(dict.fromkeys(self.games if game_ids is None else game_ids))
        entries = [self.games[g] for g in ids]
        chunk = engine.max_trees if chunk_positions is None else int(chunk_positions)
        if chunk < 1:
            raise ValueError("chunk_positions must be positive")
        seed = int(self.config.seed if seed is None else seed) & (2 ** 64 - 1)
        lengths = numpy.array([T for _, T in entries], dtype=numpy.int64)
        total = int(lengths.sum())
        if total == 0:
            return {"positions": 0, "skipped": 0, "chunks": 0}
        if total >= 2 ** 32:
            raise ValueError("reanalyse_search: a sweep takes fewer than 2**32 positions")
        chunk = min(chunk, engine.max_trees, self.reanalyse_chunk_limit(), total)
        sweep = self.search_sweep_counter          # (a refused or empty call above consumes no counter value)
        self.search_sweep_counter = sweep + 1
        first = numpy.concatenate([[0], numpy.cumsum(lengths)[:-1]]).astype(numpy.int64)
        G = len(ids)
        d_base = self._up(numpy.array([b for b, _ in entries], dtype=numpy.int64))
        d_len, d_first = self._up(lengths.astype(numpy.int32)), self._up(first)
        s_base, s_len, s_pos = be.empty((chunk,), torch.int64), be.empty((chunk,), torch.int32), be.empty((chunk,), torch.int32)
        obs = be.empty((chunk,) + self.sample_shape, torch.float32)
        to_play, flags = be.empty((chunk,), torch.int32), be.empty((chunk,), torch.int32)
        legal, tape = be.empty((chunk, self.A), torch.int32), be.empty((chunk, TAPE_WORDS), torch.int32)
        visits, info = be.empty((chunk, self.A), torch.int32), be.empty((chunk, 4), torch.int32)
        root_value, predicted = be.empty((chunk,), torch.float64), be.empty((chunk,), torch.float64)
        skipped = be.zeros((1,), torch.int32)
        batch_io = _lib.ReplayBatchIO()
        batch_io.d_base, batch_io.d_len, batch_io.d_pos = s_base.data_ptr(), s_len.data_ptr(), s_pos.data_ptr()
        batch_io.d_observation, batch_io.stacked_observations = obs.data_ptr(), self.k
        search_io = _lib.SearchIO(be.ptr(obs), be.ptr(legal), be.ptr(to_play), None, be.ptr(tape), be.ptr(visits),
                                  be.ptr(root_value), be.ptr(predicted), be.ptr(info))
        chunks = 0
        for lo in range(0, total, chunk):
            n = min(chunk, total - lo)
            lib.check(lib.mzx_replay_positions(be.ptr(d_base), be.ptr(d_len), be.ptr(d_first), G, total, lo, n, be.ptr(s_base),
                                               be.ptr(s_len), be.ptr(s_pos), be.stream()))
            batch_io.num_samples = n
            lib.check(lib.mzx_replay_batch(ctypes.byref(self.pool), ctypes.byref(batch_io), be.stream()))
            lib.check(lib.mzx_replay_search_inputs(ctypes.byref(self.pool), be.ptr(self.legal_mask), be.ptr(s_base), be.ptr(s_pos),
                                                   n, TAPE_WORDS, seed, sweep, lo, be.ptr(to_play), be.ptr(legal), be.ptr(tape),
                                                   be.ptr(flags), be.stream()))
            arena = engine.arena(n)
            lib.check(lib.mzx_search_run(engine.handle(n, TAPE_WORDS), ctypes.byref(search_io), be.ptr(arena), arena.numel(),
                                         be.stream()))
            lib.check(lib.mzx_replay_search_write(be.ptr(visits), be.ptr(root_value), be.ptr(info), be.ptr(flags), n, self.A,
                                                  be.ptr(s_base), be.ptr(s_pos), be.ptr(self.child_visits),
                                                  be.ptr(self.root_values), be.ptr(skipped), be.stream()))
            chunks += 1
        engine.arena_used_externally()
        self._run_values([e for e in entries if e[1] > 0])
        return {"positions": total, "skipped": int(skipped.cpu().numpy()[0]), "chunks": chunks}

    def download_targets(self, game_ids=None):
        """{game_id: (child_visits [T, A] f64, root_values [T] f64)} of the resident games (or ``game_ids``) as the pool
        holds them: one download per column."""
        ids = list(dict.fromkeys(self.games if game_ids is None else game_ids))
        entries = [self.games[g] for g in ids]
        visits, roots = self.child_visits.cpu().numpy(), self.root_values.cpu().numpy()
        return {g: (visits[b:b + T].copy(), roots[b:b + T].copy()) for g, (b, T) in zip(ids, entries)}


def trainer_tensors(batch, device):
    """
    The tensors ``Trainer.update_weights`` builds from a batch (trainer.py:140-153) -- observation fp32, action int64
    [batch, U + 1, 1], target value / reward / policy fp32, PER weight fp32 (None without PER), gradient scale fp32 -- from
    the second element of ``get_batch()``'s result, whether it holds device tensors (a buffer with a ``device_store``) or
    the host lists / arrays of the stock path.
    """
    def t(x):
        return x if torch.is_tensor(x) else torch.tensor(numpy.array(x))

    observation, action, value, reward, policy, weight, scale = batch
    return (t(observation).float().to(device), t(action).long().to(device).unsqueeze(-1), t(value).float().to(device),
            t(reward).float().to(device), t(policy).float().to(device),
            None if weight is None else t(weight).float().to(device), t(scale).float().to(device))


class DeviceIndexBatch:
    """
    ``index_batch`` of a ``get_batch()`` drawn on the device: the two device tensors ``game_id`` (i64 [n]) and ``pos`` (i32
    [n]).  ``ReplayBuffer.update_priorities`` takes it as it is -- nothing leaves the device.  Iterating, indexing or
    ``tolist()`` downloads ONCE and yields the reference's ``[[game_id, pos], ...]``.
    """

    def __init__(self, game_id, pos):
        self.game_id, self.pos = game_id, pos
        self._host = None

    def tolist(self):
        if self._host is None:
            self._host = [[int(g), int(p)] for g, p in zip(self.game_id.cpu().tolist(), self.pos.cpu().tolist())]
        return self._host

    def __len__(self):
        return int(self.game_id.shape[0])

    def __iter__(self):
        return iter(self.tolist())

    def __getitem__(self, i):
        return self.tolist()[i]


def _stock_replay_buffer_class():
    """
    The user's own ``ReplayBuffer`` (the reference's replay_buffer.py:11-303, importable wherever its trainer runs):
    storage, eviction and sampling stay ITS code.  Under Ray the module attribute is an ActorClass; the plain class
    behind it is what gets instantiated here (wrap the accelerated buffer with ``ray.remote`` like the reference).
    """
    import importlib
    try:
        module = importlib.import_module("replay_buffer")
    except ModuleNotFoundError as e:
        raise ModuleNotFoundError(
            "mzx.replay.ReplayBuffer wraps the reference's own buffer: module 'replay_buffer' (replay_buffer.py of "
            "muzero-general) must be importable -- put the reference checkout on sys.path, or pass the class / an "
            "instance as ReplayBuffer(..., stock=...)") from e
    return _plain_class(module.ReplayBuffer)


def _plain_class(cls):
    """The class behind a ``ray.remote`` wrapper (``ActorClass.__ray_metadata__.modified_class``), else ``cls`` itself."""
    meta = getattr(cls, "__ray_metadata__", None)
    return getattr(meta, "modified_class", cls)


class ReplayBuffer:
    """
    The stock replay buffer with its two per-element Python loops of the hand-off replaced -- by COMPOSITION: an
    instance of the reference's own ``ReplayBuffer`` (replay_buffer.py:11-303; pass the class or an instance as
    ``stock``, default: ``import replay_buffer``) keeps storage, eviction, priority feedback and every sampling draw;
    this class adds

      * ``save_game``: initial PER priorities through ``fill_initial_priorities`` before the stock ``save_game``,
        which then takes its "priorities already present" branch (:35-37);
      * ``get_batch`` / ``make_target`` (:70-138, :264-303): the reference evaluates, per sample and unroll step,
        ``compute_target_value`` with its own ``td_steps`` loop -- batch x (unroll + 1) x td_steps interpreter
        iterations per training step.  Here the n-step values of every position of a sampled game are one
        vectorised pass (``n_step_values``, same binary64 operations in the same order per position, cached per
        game until its root values are reanalysed or the game leaves the buffer), and a batch is gathers from
        per-game arrays.

    The numpy draws happen in the reference's order -- the stock ``sample_n_games`` (:166-184), then per sample its
    position (:193-202) followed by the random actions of its absorbing steps (:301) -- so with the same seed and
    buffer the batches are IDENTICAL to the reference's, element for element (tests/test_replay_batch.py runs the
    two side by side).  The tensors come back as numpy arrays instead of nested lists (``trainer.py:55-75`` feeds
    them to ``torch.tensor`` either way).  Attributes (``buffer``, ``num_played_games``, ``total_samples``, ...)
    read through to the stock object.

    ``device_store`` (a ``DeviceGameStore``; opt-in, nothing changes without it): the games also live on the device --
    ``save_game`` / ``update_game_history`` / the stock eviction keep the store in step, the games of an
    ``initial_buffer`` are ingested -- and ``get_batch`` returns DEVICE tensors: the draws below only fill index arrays
    and the tape of absorbing-step actions, one ``mzx_replay_batch`` call gathers observations and targets from the pool
    (same tuple, ``index_batch`` stays a host list; ``trainer_tensors`` binds it to a trainer).  The one deliberate
    difference from the reference: the pool adds a capacity bound in POSITIONS to ``replay_buffer_size`` in games.  When
    a new game does not fit after the rows of already evicted games are released, the oldest games leave both the
    store and the stock buffer (the stock buffer's own eviction statements, replay_buffer.py:59-61).

    ``device_sampler=True`` (opt-in on top of a store built with ``max_games``; ValueError otherwise): the DRAWS move to
    the device too.  ``get_batch`` calls ``store.sample`` -- seed ``config.seed``, a counter that advances by one per call;
    the reference's two-level distribution over a counter-based generator, so the batches are not numpy's -- and gathers
    from the sampled arrays with no host copy in between; ``index_batch`` is a ``DeviceIndexBatch``.
    ``update_priorities(priorities, index_info)`` with such an index runs the device scatter (``priorities``: a device
    tensor or an array); with a host list it stays the stock method.  With the sampler on, the DEVICE columns are
    authoritative: ``priorities`` / ``game_priority`` of the host ``GameHistory`` objects go stale until
    ``sync_priorities()`` writes them back (do that before pickling the buffer for a checkpoint).
    """

    def __init__(self, initial_checkpoint, initial_buffer, config, stock=None, device_store=None, device_sampler=False):
        if device_sampler and (device_store is None or device_store.sampler is None):
            raise ValueError("device_sampler=True needs a device_store built with max_games")
        factory = _plain_class(stock) if stock is not None else _stock_replay_buffer_class()
        # a class (also the one behind a ray.remote ActorClass) is instantiated; anything that already has the buffer's
        # methods is taken as the instance to wrap
        built = factory(initial_checkpoint, initial_buffer, config) if isinstance(factory, type) else factory
        object.__setattr__(self, "_stock", built)
        object.__setattr__(self, "_arrays", {})   # game_id -> (game_history, per-game numpy views); dropped when the game changes or leaves
        object.__setattr__(self, "_store", device_store)
        object.__setattr__(self, "_sampler", bool(device_sampler))
        object.__setattr__(self, "_sample_calls", 0)
        if device_store is not None:
            self._store_sync(list(self._stock.buffer.items()))

    @property
    def device_store(self):
        return self._store

    def _store_sync(self, new_games):
        """Games the stock buffer no longer holds leave the store; ``new_games`` enter it, the oldest games making room."""
        store, stock = self._store, self._stock
        for game_id in [g for g in store.games if g not in stock.buffer]:
            store.drop(game_id)
        new_games = [(g, h) for g, h in new_games if g in stock.buffer]
        while new_games:
            try:
                return store.add_many(new_games)
            except StoreFull:
                if len(stock.buffer) <= 1:
                    raise
            del_id = self._evict_oldest()
            new_games = [(g, h) for g, h in new_games if g != del_id]

    def _evict_oldest(self):
        """The capacity bound in positions: the stock buffer's eviction (replay_buffer.py:59-61), applied once more."""
        store, stock = self._store, self._stock
        del_id = stock.num_played_games - len(stock.buffer)
        stock.total_samples -= positions_of(stock.buffer[del_id])
        del stock.buffer[del_id]
        self._arrays.pop(del_id, None)
        if del_id in store:
            store.drop(del_id)
        return del_id

    def _store_reserve(self, game_id, T):
        """``_store_sync`` of one game that the stock buffer has just saved, on the host alone: the game gets its rows and
        its slot (``DeviceGameStore._reserve``), the oldest games making room exactly as they do for ``add_many`` -- the
        rows are filled later, by one ingest for the whole hand-off."""
        store, stock = self._store, self._stock
        while game_id in stock.buffer:
            try:
                return store._reserve([(game_id, T)])
            except StoreFull:
                if len(stock.buffer) <= 1:
                    raise
            self._evict_oldest()

    def __getattr__(self, name):
        if name in ("_stock", "_arrays", "_store", "_sampler", "_sample_calls"):
            raise AttributeError(name)
        return getattr(self._stock, name)

    def __setattr__(self, name, value):
        # the buffer's state lives in the stock object: writes to its public attributes (buffer, num_played_games, ...)
        # land there, like the reads above
        if name.startswith("_"):
            object.__setattr__(self, name, value)
        else:
            setattr(self._stock, name, value)

    # ---- storage / sampling: the stock buffer's own code (explicit so that ray.remote sees the methods)
    def get_buffer(self):
        return self._stock.get_buffer()

    def update_priorities(self, priorities, index_info):
        if isinstance(index_info, DeviceIndexBatch):
            if self._store is None or self._store.sampler is None:
                raise ValueError("a DeviceIndexBatch belongs to a buffer with a device sampler")
            return self._store.update_priorities(priorities, index_info.game_id, index_info.pos)
        return self._stock.update_priorities(priorities, index_info)

    def sync_priorities(self):
        """The device priorities and game priorities written back into the resident ``GameHistory`` objects (for
        checkpoints: the reference pickles the buffer).  One download of the two columns; a no-op with PER off."""
        store = self._store
        if store is None or store.sampler is None or not self._stock.config.PER:
            return
        store._flush_slots()
        priorities, top = store.priorities.cpu().numpy(), store.slot_priority.cpu().numpy()
        for game_id, game_history in self._stock.buffer.items():
            if game_id in store:
                base, T = store.games[game_id]
                if T:
                    game_history.priorities = priorities[base:base + T].copy()
                    game_history.game_priority = top[game_id % store.max_games]

    def sync_targets(self):
        """The device targets written back into the resident ``GameHistory`` objects after ``reanalyse_search`` (for
        checkpoints and a host-side ``get_batch``): ``child_visits`` as a list of lists, ``root_values`` as a list of floats,
        ``reanalysed_predicted_root_values = None`` -- the pool's root values ARE the searched ones.  One download per
        column; a no-op without a device store.  A game whose host history has another length than the store's copy raises
        ValueError before anything is written: a checkpoint must not mix synchronised and stale games."""
        store = self._store
        if store is None:
            return
        targets = store.download_targets([g for g in self._stock.buffer if g in store])
        odd = [g for g, (_, roots) in targets.items() if positions_of(self._stock.buffer[g]) != len(roots)]
        if odd:
            raise ValueError(f"sync_targets: games {odd[:8]} changed length since they entered the device store")
        for game_id, (visits, roots) in targets.items():
            game_history = self._stock.buffer[game_id]
            game_history.child_visits = visits.tolist()
            game_history.root_values = roots.tolist()
            game_history.reanalysed_predicted_root_values = None
            self._arrays.pop(game_id, None)

    def sample_game(self, force_uniform=False):
        return self._stock.sample_game(force_uniform)

    def sample_n_games(self, n_games, force_uniform=False):
        return self._stock.sample_n_games(n_games, force_uniform)

    def sample_position(self, game_history, force_uniform=False):
        return self._stock.sample_position(game_history, force_uniform)

    def compute_target_value(self, game_history, index):
        return self._stock.compute_target_value(game_history, index)

    def save_game(self, game_history, shared_storage=None):
        fill_initial_priorities(game_history, self._stock.config)    # no-op for games it does not cover
        if self._store is not None and len(game_history.root_values) + 1 > self._store.rows:
            raise StoreFull(f"a game of {len(game_history.root_values)} positions exceeds the device store's {self._store.rows} rows")
        out = self._stock.save_game(game_history, shared_storage)
        if self._store is not None:
            self._store_sync([(self._stock.num_played_games - 1, game_history)])
        if self._arrays and self._stock.buffer:                      # evicted games take their cached arrays along
            oldest = next(iter(self._stock.buffer))                  # game ids only grow (replay_buffer.py:53-62)
            for game_id in [g for g in self._arrays if g < oldest]:
                del self._arrays[game_id]
        return out

    def save_games(self, histories, shared_storage=None):
        """
        ``save_game`` for every game of a hand-off.  Without a device store, or for ``histories`` without ``records`` (a
        plain list), exactly that loop.  With a device store and a shard's ``ShardGames``: the initial priorities through
        ``fill_initial_priorities_many`` (records that came with theirs return at once); the size check of ``save_game`` for
        EVERY game before anything is stored; then per game the stock ``save_game`` for the stock buffer's own bookkeeping
        -- ``buffer``, the counters, eviction by ``replay_buffer_size``; called without ``shared_storage``, the two counters
        are published once at the end -- and the HOST half of the store's synchronisation (``_store_reserve``): the game
        gets the rows and the slot ``add_many`` would give it at that point, the oldest games leaving store and stock
        buffer when it does not fit, statement for statement what the loop does.  Nothing touches the device until the
        end: ONE ``DeviceGameStore`` ingest (``_stage_views``: one upload, one ``mzx_replay_ingest`` per chunk) fills the
        rows of the games that are still resident; a game of the hand-off that was evicted again within it is never
        uploaded.  Stock buffer, counters, residency, bases and pool contents are those of the loop, whatever is evicted
        (tests/replay_ingest_cases.py: ``check_save_games``).  A game that is no fresh view of the hand-off's records (a
        plain ``GameHistory``, a materialised view) goes through ``save_game`` in its turn, the games before it ingested
        first.  After an exception the games saved so far are in both, as after the loop.
        """
        store, stock = self._store, self._stock
        records = getattr(histories, "records", None)
        if store is None or not records:
            for game_history in histories:
                self.save_game(game_history, shared_storage)
            return
        config = stock.config
        known = {id(record) for record, _, _ in records}
        views = []             # (taken first: the steps below read fields of a view, which materialises them)
        for game_history in histories:
            view = store._fresh_view(game_history, known)
            T = len(game_history.root_values) if view is None else view[2]
            if T + 1 > store.rows:
                raise StoreFull(f"a game of {T} positions exceeds the device store's {store.rows} rows")
            views.append(view)
        # the device hand-off: a fresh view of a LIVE piece-backed record never comes to the host -- provided the hand-off
        # brings every game of its piece (a piece is ingested whole); any other piece is fetched, and its records are
        # ordinary host records from here on
        covered = {}
        for view in views:
            if view is not None and isinstance(view[0], _PieceRecord) and view[0].live:
                covered[id(view[0].piece)] = covered.get(id(view[0].piece), 0) + 1
        for record, _, _ in records:
            if isinstance(record, _PieceRecord) and record.live and covered.get(id(record.piece), 0) != record.piece.games:
                record.piece.fetch()
        on_device = [view is not None and isinstance(view[0], _PieceRecord) and view[0].live for view in views]
        fill_initial_priorities_many(histories, config, backend=store.backend)
        for game_id in [g for g in store.games if g not in stock.buffer]:
            store.drop(game_id)
        pending = []           # reserved fresh views whose rows are not filled yet: (game_id, game_history), view, on the device

        def flush():
            host = [(item, view) for item, view, device in pending if item[0] in store.games and not device]
            pieces = {}          # id(piece) -> piece, base and game id per game of the piece, the records' rows -> game id
            for (game_id, _), (record, row, _) in [(item, view) for item, view, device in pending if device]:
                piece = record.piece
                entry = pieces.get(id(piece))
                if entry is None:
                    entry = pieces[id(piece)] = (piece, numpy.full(piece.games, -1, numpy.int64), numpy.full(piece.games, -1, numpy.int64), {})
                j = int(record.rows_n[row])
                entry[1][j] = store.games[game_id][0] if game_id in store.games else -1
                entry[2][j] = game_id
                entry[3].setdefault(id(record), (record, {}))[1][row] = game_id
            del pending[:]
            store._stage_views([item for item, _ in host], [view for _, view in host])
            for piece, bases, ids, bound in pieces.values():
                store.ingest_piece(piece, bases, ids)
                game = piece.group.game
                for record, rows in bound.values():
                    record.bind(store, rows, game.obs_dtype, game.reward_dtype is numpy.int64)

        try:
            for game_history, view, device in zip(histories, views, on_device):
                if view is None:                  # any other game: the per-game path, behind the games before it
                    flush()
                    self.save_game(game_history, None)
                    continue
                oldest = next(iter(stock.buffer), None)
                if device:
                    # the stock buffer's bookkeeping, replay_buffer.py:53-61, with T from the hand-off's lengths (its PER
                    # branch :34-51 would read the game: the device columns are authoritative)
                    stock.buffer[stock.num_played_games] = game_history
                    stock.num_played_games += 1
                    stock.num_played_steps += view[2]
                    stock.total_samples += view[2]
                    if config.replay_buffer_size < len(stock.buffer):
                        del_id = stock.num_played_games - len(stock.buffer)
                        stock.total_samples -= positions_of(stock.buffer[del_id])
                        del stock.buffer[del_id]
                else:
                    stock.save_game(game_history, None)
                if oldest is not None and oldest not in stock.buffer and oldest in store:      # evicted by replay_buffer_size
                    store.drop(oldest)
                game_id = stock.num_played_games - 1
                self._store_reserve(game_id, view[2])
                pending.append(((game_id, game_history), view, device))
        finally:
            flush()
        if self._arrays and stock.buffer:
            oldest = next(iter(stock.buffer))
            for game_id in [g for g in self._arrays if g < oldest]:
                del self._arrays[game_id]
        if shared_storage:
            set_info = shared_storage.set_info
            set_info = getattr(set_info, "remote", set_info)
            set_info("num_played_games", stock.num_played_games)
            set_info("num_played_steps", stock.num_played_steps)

    def update_game_history(self, game_id, game_history):
        self._arrays.pop(game_id, None)          # reanalysed root values change the n-step targets
        out = self._stock.update_game_history(game_id, game_history)
        if self._store is not None and game_id in self._store and self._stock.buffer.get(game_id) is game_history:
            self._store.update(game_id, game_history)
        return out

    # ---- position draw
    def _sample_position_fast(self, game_history):
        """
        sample_position (:186-202) without the interpreter loop of ``sum(priorities)`` and without
        ``numpy.random.choice``'s argument checks -- same numbers, same single draw: Python's ``sum`` over a float32
        array is the sequential float32 accumulation ``cumsum`` performs; ``choice(n, p=p)`` widens p to binary64,
        takes ``cdf = p.cumsum(); cdf /= cdf[-1]`` and bisects one ``random_sample()`` from the right.
        """
        if not self._stock.config.PER:
            return numpy.random.randint(0, len(game_history.root_values)), None      # choice(n) == randint(0, n)
        pr = game_history.priorities
        if pr.dtype != numpy.float32 or pr.ndim != 1 or pr.size == 0:
            return self._stock.sample_position(game_history)
        position_probs = pr / numpy.cumsum(pr, dtype=numpy.float32)[-1]
        cdf = position_probs.astype(numpy.float64).cumsum()
        cdf /= cdf[-1]
        position_index = int(cdf.searchsorted(numpy.random.random_sample(), side="right"))
        return position_index, position_probs[position_index]

    # ---- targets (replay_buffer.py:264-303 as gathers)
    def _build_arrays(self, game_history):
        """Per-game arrays a batch gathers from: n-step values [T], rewards / actions [T + 1], child visits [T][A]."""
        T = len(game_history.root_values)
        return dict(
            T=T,
            values=n_step_values(game_history, self._stock.config) if T else numpy.zeros(0),
            rewards=numpy.array([float(r) for r in game_history.reward_history], dtype=numpy.float64),
            actions=numpy.array([int(a) for a in game_history.action_history], dtype=numpy.int64),
            visits=numpy.array(game_history.child_visits, dtype=numpy.float64).reshape(T, -1),
        )

    def _game_arrays(self, game_id, game_history):
        hit = self._arrays.get(game_id)
        if hit is not None and hit[0] is game_history:
            return hit[1]
        arrays = self._build_arrays(game_history)
        self._arrays[game_id] = (game_history, arrays)
        return arrays

    def make_target(self, game_history, state_index, _arrays=None):
        """replay_buffer.py:264-303 for one position: (values, rewards, policies, actions) as arrays.  Without the
        arrays of a buffered game (``get_batch`` passes them) they are built on the fly, nothing is cached."""
        cfg = self._stock.config
        g = _arrays if _arrays is not None else self._build_arrays(game_history)
        U, T = cfg.num_unroll_steps, g["T"]
        A = g["visits"].shape[1] if T else len(cfg.action_space)
        idx = state_index + numpy.arange(U + 1)
        inside, at_end = idx < T, idx == T
        safe = numpy.minimum(idx, max(T - 1, 0))
        values = numpy.where(inside, g["values"][safe] if T else 0.0, 0.0)
        rewards = numpy.where(inside | at_end, g["rewards"][numpy.minimum(idx, T)], 0.0)
        policies = numpy.where(inside[:, None], g["visits"][safe] if T else 0.0, 1 / A)
        actions = g["actions"][numpy.minimum(idx, T)].copy()
        if idx[-1] > T:                          # States past the end of games are treated as absorbing states
            space = cfg.action_space
            for k in range(max(0, T + 1 - state_index), U + 1):
                actions[k] = space[numpy.random.randint(0, len(space))]    # == numpy.random.choice(space), same draw
        return values, rewards, policies, actions

    def _get_batch_device(self):
        """get_batch with a device store: the same draws in the same order, the tensors gathered by mzx_replay_batch."""
        cfg, store = self._stock.config, self._store
        U, space = cfg.num_unroll_steps, cfg.action_space
        n = cfg.batch_size
        total_samples = self._stock.total_samples
        index_batch, weight_batch = [], [] if cfg.PER else None
        tape = numpy.zeros((n, U + 1), numpy.int32)
        for i, (game_id, game_history, game_prob) in enumerate(self._stock.sample_n_games(n)):
            game_pos, pos_prob = self._sample_position_fast(game_history)
            index_batch.append([game_id, game_pos])
            for k in range(max(0, len(game_history.root_values) + 1 - game_pos), U + 1):     # absorbing steps (:301)
                tape[i, k] = space[numpy.random.randint(0, len(space))]    # == numpy.random.choice(space), same draw
            if cfg.PER:
                weight_batch.append(1 / (total_samples * game_prob * pos_prob))
        if cfg.PER:
            weight_batch = numpy.array(weight_batch, dtype="float32") / max(weight_batch)
            weight_batch = torch.from_numpy(weight_batch).to(store.backend.device, non_blocking=True)
        observation_batch, (value_batch, reward_batch, policy_batch, action_batch, gradient_scale_batch) = store.batch(
            [g for g, _ in index_batch], [p for _, p in index_batch], tape, U)
        return (index_batch, (observation_batch, action_batch, value_batch, reward_batch, policy_batch, weight_batch,
                              gradient_scale_batch))

    def _get_batch_sampled(self):
        """get_batch with the device sampler: draw, gather -- launches on the backend's stream, nothing per sample here."""
        cfg, store = self._stock.config, self._store
        call = self._sample_calls
        self._sample_calls = call + 1
        base, length, pos, tape, game_id, weight_batch = store.sample(
            cfg.batch_size, cfg.seed, call, self._stock.total_samples, cfg.PER, cfg.num_unroll_steps)
        observation_batch, (value_batch, reward_batch, policy_batch, action_batch, gradient_scale_batch) = store.gather(
            base, length, pos, tape, cfg.num_unroll_steps)
        return (DeviceIndexBatch(game_id, pos), (observation_batch, action_batch, value_batch, reward_batch, policy_batch,
                                                 weight_batch, gradient_scale_batch))

    def get_batch(self):
        if self._sampler:
            return self._get_batch_sampled()
        if self._store is not None:
            return self._get_batch_device()
        cfg = self._stock.config
        U, A = cfg.num_unroll_steps, len(cfg.action_space)
        n = cfg.batch_size
        total_samples = self._stock.total_samples
        index_batch, observation_batch = [], []
        action_batch = numpy.empty((n, U + 1), numpy.int64)
        value_batch = numpy.empty((n, U + 1), numpy.float64)
        reward_batch = numpy.empty((n, U + 1), numpy.float64)
        policy_batch = numpy.empty((n, U + 1, A), numpy.float64)
        gradient_scale_batch = numpy.empty((n, U + 1), numpy.int64)
        weight_batch = [] if cfg.PER else None
        for i, (game_id, game_history, game_prob) in enumerate(self._stock.sample_n_games(n)):
            game_pos, pos_prob = self._sample_position_fast(game_history)
            values, rewards, policies, actions = self.make_target(game_history, game_pos,
                                                                  self._game_arrays(game_id, game_history))
            index_batch.append([game_id, game_pos])
            observation_batch.append(game_history.get_stacked_observations(game_pos, cfg.stacked_observations, A))
            action_batch[i], value_batch[i], reward_batch[i], policy_batch[i] = actions, values, rewards, policies
            gradient_scale_batch[i] = min(U, len(game_history.action_history) - game_pos)
            if cfg.PER:
                weight_batch.append(1 / (total_samples * game_prob * pos_prob))
        if cfg.PER:
            weight_batch = numpy.array(weight_batch, dtype="float32") / max(weight_batch)
        # observation_batch: batch, channels, height, width; action / value / reward / gradient_scale: batch,
        # num_unroll_steps + 1; policy_batch: batch, num_unroll_steps + 1, len(action_space); weight_batch: batch
        return (index_batch, (observation_batch, action_batch, value_batch, reward_batch, policy_batch, weight_batch,
                              gradient_scale_batch))


def _remote(method, *args, **kwargs):
    """Call an actor method (``.remote`` + ``ray.get``) or a plain method alike."""
    if hasattr(method, "remote"):
        import ray
        return ray.get(method.remote(*args, **kwargs))
    return method(*args, **kwargs)


class Reanalyse:
    """
    replay_buffer.py:306-373 -- refreshes ``reanalysed_predicted_root_values`` of stored games with the
    latest network.  ``reanalyse_game`` is the per-game step (new, reusable); ``reanalyse`` the worker loop.
    """

    def __init__(self, initial_checkpoint, config, _backend=None, device_store=None):
        self.config = config
        # a DeviceGameStore (default: the replay buffer's own, when ``reanalyse`` is handed a local buffer that has one):
        # games resident in it are stacked from the pool instead of being uploaded again
        self.device_store = device_store
        # Fix random generator seed (replay_buffer.py:318-319)
        numpy.random.seed(self.config.seed)
        torch.manual_seed(self.config.seed)
        # the network lives on the GPU whatever config.reanalyse_on_gpu says: the engine has no CPU path
        self.model = models.MuZeroNetwork(self.config, _backend=_backend)
        self.model.set_weights(initial_checkpoint["weights"])
        self.model.eval()
        self.num_reanalysed_games = initial_checkpoint["num_reanalysed_games"]
        self._search_engine = None      # reanalyse_store(search=True): built on first use

    def reanalyse_game(self, game_history, game_id=None):
        """
        replay_buffer.py:343-367: float32 array [len(root_values)] of decoded root values under the current weights.
        With ``game_id`` of a game resident in ``device_store`` the stacked observations are gathered from the pool
        (samples (game, 0 .. T-1) of ``mzx_replay_batch``) -- same planes, nothing uploaded.
        """
        n = len(game_history.root_values)
        backend = self.model.backend
        store = self.device_store
        if store is not None and game_id is not None and game_id in store and store.games[game_id][1] == n:
            stacked = store.stacked(game_id, n)
        else:
            stacked = observations.stack_history(backend, self.config, game_history.observation_history,
                                                 game_history.action_history, count=n)
        if n == 0:
            return numpy.zeros((0,), numpy.float32)
        value_logits = self.model.initial_inference(stacked)[0]
        values = models.support_to_scalar(value_logits, self.config.support_size, _backend=backend)
        return torch.squeeze(values).detach().cpu().numpy()

    def reanalyse_store(self, replay_buffer, game_ids=None, search=None):
        """
        The sweep as a worker step (``DeviceGameStore.reanalyse`` under the current weights): every game of the buffer's
        device store that the stock buffer still holds -- or those of ``game_ids`` -- gets its float32 array [T] as
        ``reanalysed_predicted_root_values`` (what ``reanalyse_game`` would assign), its cached host arrays are dropped and
        it counts in ``num_reanalysed_games``; the pool's root values and n-step values are already refreshed in place.  A
        game the stock buffer has evicted is passed over.  Needs an in-process ``ReplayBuffer`` with a device store (device
        pointers do not cross processes).  Returns the number of games refreshed.

        ``search`` (default ``config.reanalyse_search``, False when the config has no such field): the games are SEARCHED
        again instead (``DeviceGameStore.reanalyse_search``) -- policy targets and root values refreshed in the pool; the
        host histories go stale until ``replay_buffer.sync_targets()``.  The worker builds its ``BatchedMCTS`` once:
        ``config.reanalyse_search_trees`` roots per chunk (default 1024), ``config.reanalyse_search_simulations``
        simulations (default ``config.num_simulations``).
        """
        store = replay_buffer.device_store if isinstance(replay_buffer, ReplayBuffer) else None
        if store is None:
            raise ValueError("reanalyse_store needs an in-process mzx.replay.ReplayBuffer with a device_store")
        buffer = replay_buffer.buffer
        ids = [g for g in (store.games if game_ids is None else game_ids) if g in buffer or g not in store]
        if getattr(self.config, "reanalyse_search", False) if search is None else search:
            if self._search_engine is None:
                from .search import BatchedMCTS
                self._search_engine = BatchedMCTS(
                    self.config, self.model, int(getattr(self.config, "reanalyse_search_trees", 1024)),
                    num_simulations=int(getattr(self.config, "reanalyse_search_simulations", self.config.num_simulations)))
            ids = list(dict.fromkeys(ids))
            store.reanalyse_search(self._search_engine, ids)
            for game_id in ids:
                replay_buffer._arrays.pop(game_id, None)      # the cached host targets are stale
            self.num_reanalysed_games += len(ids)
            return len(ids)
        done = 0
        for game_id, values in store.reanalyse(self.model, ids).items():
            game_history = buffer.get(game_id)
            if game_history is None or len(game_history.root_values) != len(values):
                continue
            game_history.reanalysed_predicted_root_values = values
            replay_buffer._arrays.pop(game_id, None)      # reanalysed root values change the n-step targets
            done += 1
        self.num_reanalysed_games += done
        return done

    def reanalyse(self, replay_buffer, shared_storage):
        get = lambda key: _remote(shared_storage.get_info, key)
        while get("num_played_games") < 1:
            time.sleep(0.1)
        if self.device_store is None and isinstance(replay_buffer, ReplayBuffer):
            self.device_store = replay_buffer.device_store
        # opt-in (config.reanalyse_sweep): every resident game per iteration instead of one drawn game
        sweep = (getattr(self.config, "reanalyse_sweep", False) and isinstance(replay_buffer, ReplayBuffer)
                 and replay_buffer.device_store is not None)
        while get("training_step") < self.config.training_steps and not get("terminate"):
            self.model.set_weights(get("weights"))
            if sweep and self.config.use_last_model_value:
                self.reanalyse_store(replay_buffer)
                _remote(shared_storage.set_info, "num_reanalysed_games", self.num_reanalysed_games)
                continue
            game_id, game_history, _ = _remote(replay_buffer.sample_game, force_uniform=True)
            # Use the last model to provide a fresher, stable n-step value (See paper appendix Reanalyze)
            if self.config.use_last_model_value:
                game_history.reanalysed_predicted_root_values = self.reanalyse_game(game_history, game_id)
            _remote(replay_buffer.update_game_history, game_id, game_history)
            self.num_reanalysed_games += 1
            _remote(shared_storage.set_info, "num_reanalysed_games", self.num_reanalysed_games)
