"""
Host-side mirror of the reference's self-play surface, driving the batched HIP search.

Same names / arguments / error behaviour as /root/reference/self_play.py:
  SelfPlay(initial_checkpoint, Game, config, seed)      :11-29
  SelfPlay.continuous_self_play(shared_storage, replay_buffer, test_mode)  :31-108
  SelfPlay.play_game(temperature, temperature_threshold, render, opponent, muzero_player)  :110-183
  SelfPlay.select_action(node, temperature)              :222-245
  MCTS(config).run(model, observation, legal_actions, to_play, add_exploration_noise)  :260-361
  Node / GameHistory / MinMaxStats                        :433-570
plus the batched forms the reference lacks ("Batch MCTS" is an open TODO in its
README): ``BatchedMCTS`` searches B roots per call and ``SelfPlay(..., num_games=B)``
plays B games in lock-step on one GPU (the game shard of this process).

Division of labour: Python owns the plugin ``Game`` objects, the per-game numpy
``RandomState`` streams and the ``GameHistory`` records; everything between "stacked
observation" and "root visit counts" runs on the device behind include/mzx.h.

Random streams.  The reference draws from the process-global numpy stream in
this order per move: Dirichlet noise (:473), one ``choice`` per tied argmax
(:371), the action sample (:229-243).  A batched engine needs one stream per
game: game i of a shard uses ``RandomState(seed + i)`` -- the stream the
reference's i-th actor has (muzero.py:185) -- and with ``num_games == 1`` the
process-global stream itself, so a single game reproduces the reference draw for
draw.  Tie draws happen on the device from a tape of the stream's next raw
words (numpy's masked rejection, exactly); the host then advances the stream by
the number of words the device consumed.

How the actor is laid out.  A move of a shard is written down in ONE place per protocol: ``_start_game`` / ``_log_moves``
for per-object games (``_play_shard``, ``_rounds_shard`` and the stream-bank branch of ``_play``; the render / opponent /
``Node`` branch of ``_play`` logs game by game as the reference does), ``shard_play.legal_mask_row`` /
``shard_play.shard_views`` for the batched protocol (``_play_batched`` game-major, ``BatchedGroup`` in ring rows).  The
rules they share are single functions: ``shard_play.move_temperature``, ``_count_search``, ``_slot_spans``.
``play_rounds`` is ``_run_rounds`` over slot groups (``shard_play.SlotGroup``) with the protocol's own begin / consume and
queue-ahead rule; ``_live`` is ``{"groups": [...]}`` (+ ``"native"``: the ``NativeShard``) while games are in progress.
"""
import contextlib
import ctypes
import math
import time
import warnings

import numpy
import torch

from . import _lib, _rng, models, native_rounds, replay
from . import observations as observations_mod
from .shard_play import BatchedGroup as _BatchedGroup, ObjectGroup, SlotGroup, legal_mask_row, move_temperature, shard_views  # noqa: F401
# round 6: the records / tree facades and the batched search live in modules of their own; every name stays importable
# from here (the reference has them all in self_play.py)
from .history import GameHistory, MinMaxStats, Node, ShardGameHistory, ShardGames, _ShardRecord, gc_paused  # noqa: F401
from .search import TAPE_WORDS, BatchedMCTS, MCTS, PendingSearch, SearchResult, _validate  # noqa: F401


def _remote(method, *args):
    """Call a storage/replay method that may be a Ray actor method (``.remote``) or a plain one."""
    if hasattr(method, "remote"):
        import ray
        return ray.get(method.remote(*args))
    return method(*args)


class SelfPlay:
    """
    self_play.py:11-245.  ``num_games`` (new, default 1) is the number of games
    this process plays in lock-step on its GPU; game i is seeded ``seed + i``.
    """

    def __init__(self, initial_checkpoint, Game, config, seed, num_games=1, _backend=None):
        _validate(config)
        self.config = config
        self.num_games = int(num_games)
        self.batched_game = None
        if getattr(Game, "batched", False):
            # optional batched plugin protocol (mzx.synthetic.make_synthetic_batched_game documents it): ONE
            # object steps the whole shard, the per-move host work is a handful of numpy calls
            self._game_seeds = [seed + i for i in range(self.num_games)]
            # (a natively stepped game -- mzx.games.NativeBatchedGame -- lives in the library this actor's model runs on)
            self.batched_game = (Game(self._game_seeds, _backend=_backend) if getattr(Game, "native", False)
                                 else Game(self._game_seeds))
            self.games = []
            self.game = self.batched_game
        else:
            self.games = [Game(seed + i) for i in range(self.num_games)]
            self.game = self.games[0]

        # Fix random generator seed (self_play.py:21-23)
        numpy.random.seed(seed)
        torch.manual_seed(seed)
        # game 0 of a single-game actor draws from the process-global stream like the reference; a shard of
        # games uses the native stream bank, stream i = RandomState(seed + i) (muzero.py:185 seeds actor i so)
        self.rngs = [numpy.random.mtrand._rand]
        self.bank = None

        # Initialize the network (self_play.py:25-29)
        self.model = models.MuZeroNetwork(self.config, _backend=_backend)
        self.model.set_weights(initial_checkpoint["weights"])
        self.model.eval()
        self.engine = BatchedMCTS(self.config, self.model, self.num_games)
        # config.device_draws: noise, tie words and action choice drawn on the device as a function of (config.seed, slot,
        # counter) -- csrc/mzx_draws.h; not numpy's draws (opt-in), no host stream is read.  Batched shards only.
        # The key is THIS actor's seed -- the number that seeds its games and, on host draws, its streams -- not config.seed:
        # the ranks of a job share a configuration (rank r is seeded config.seed + r * num_games) and must not draw alike.
        self.device_draws = bool(getattr(self.config, "device_draws", False))
        self.draw_seed = int(seed)
        self.engine.draw_seed = self.draw_seed
        self._draw_counter = 0
        if self.num_games > 1 or self.batched_game is not None:
            self.bank = _rng.StreamBank(self.model.backend.lib, [(seed + i) & 0xFFFFFFFF for i in range(self.num_games)])
        self.stats = {"searches": 0, "simulations": 0, "search_seconds": 0.0}
        self._live = None       # state of the games in progress under play_rounds

    @property
    def draw_counter(self):
        """Device draws: the counter of the next search (of every slot group: they advance together).  Saved with a
        checkpoint and set on a fresh actor in the same game state, it continues the same games.  A search queued ahead and
        not yet consumed is dropped first (as the setter and ``close_game`` do), so the value read is the one to restore."""
        self._drain_searches()
        live = self._live
        if self.device_draws and live is not None:
            if live.get("native") is not None:
                return max(int(g.lib.mzx_actor_draw_counter(g.handle)) for g in live["groups"])
            return max(int(g.counter) for g in live["groups"])
        return self._draw_counter

    @draw_counter.setter
    def draw_counter(self, value):
        self._drain_searches()
        self._draw_counter = int(value)
        live = self._live
        if self.device_draws and live is not None:
            if live.get("native") is not None:
                live["native"].set_draw_counter(self._draw_counter)
            else:
                for g in live["groups"]:
                    g.counter = self._draw_counter

    def _no_device_draws(self, what):
        if self.device_draws:
            raise NotImplementedError(f"config.device_draws covers the batched game protocol (play_games / play_rounds of a "
                                      f"batched game); {what} draws from numpy streams and would mix the two generators")

    # ------------------------------------------------------------------ loops
    def continuous_self_play(self, shared_storage, replay_buffer, test_mode=False):
        """
        self_play.py:31-108.  With a ``mzx.shared_storage.ShardedStorage`` (one self-play process per GPU under
        torch.distributed) the per-game weight pull (:37) becomes the storage's ``refresh``: a NON-BLOCKING step of
        an asynchronous exchange (one six-word control all-reduce in flight at a time; when the trainer published
        new weights ONE RCCL broadcast of the flat buffer) -- a rank never waits for another one inside this loop,
        it plays on with the control values and weights it has; the stop condition is evaluated on the same
        exchange by every rank, ``finish`` drains the sequence.  This rank's games are seeded ``seed + i`` with ``seed`` =
        ``shard_seeds(config.seed, num_games)[0]`` (muzero.py:185).
        """
        native_rounds.check_handoff_buffer(self.config, replay_buffer)      # (config.device_handoff: a local device buffer)
        sharded = hasattr(shared_storage, "refresh")
        get = (shared_storage.get_info if sharded else (lambda key: _remote(shared_storage.get_info, key)))
        if sharded:
            # what every rank must evaluate alike / how often the trainer publishes (trainer.py: checkpoint_interval)
            if getattr(shared_storage, "training_steps", 0) is None:
                shared_storage.training_steps = self.config.training_steps
            if getattr(shared_storage, "checkpoint_interval", 0) is None:
                shared_storage.checkpoint_interval = getattr(self.config, "checkpoint_interval", 10)
            shared_storage.refresh(self.model, block=True)     # the trainer's weights before the first game
        save_game = replay_buffer.save_game
        save_is_remote = hasattr(save_game, "remote")
        # a local buffer that takes a whole hand-off at once (mzx.replay.ReplayBuffer.save_games: with a device store the
        # games reach the pool through one bulk ingest instead of a dozen runtime calls per game)
        save_games = getattr(replay_buffer, "save_games", None)
        if save_games is not None and hasattr(save_games, "remote"):
            save_games = None

        def hand_off(histories):
            # initial PER priorities, on the device (replay_buffer.py:39-51 would loop in Python) -- the games a shard
            # hands out together in ONE pass over their record; save_game then takes its "priorities already present" branch
            replay.fill_initial_priorities_many(histories, self.config, backend=self.model.backend)
            if save_is_remote:
                for game_history in histories:
                    _remote(save_game, game_history, shared_storage)
            elif save_games is not None:
                save_games(histories, shared_storage)
            else:
                for game_history in histories:
                    save_game(game_history, shared_storage)

        # A natively played shard (mzx/native_rounds.py) spends its rounds inside ONE library call that needs no
        # interpreter: the hand-off of the games call k returned -- priorities, save_game of every game: Python per game, as
        # much wall time as playing them -- runs on this thread WHILE a worker thread is inside call k + 1.  Weights are
        # only set between calls, with no call in flight; a game reaches the buffer one call later than it would otherwise
        # (``config.self_play_overlap_handoff = False``: strictly in turn).
        overlap = (not test_mode and native_rounds.usable(self) and getattr(self.config, "refill_finished_games", True)
                   and getattr(self.config, "self_play_overlap_handoff", True))
        waiting, executor = None, None
        if overlap:
            import concurrent.futures
            executor = concurrent.futures.ThreadPoolExecutor(max_workers=1)
            on_gpu = self.model.backend.device.type == "cuda"
            stream = torch.cuda.current_stream(self.model.backend.device) if on_gpu else None

            def rounds_on_worker(temperature, threshold):
                # ONLY the library call runs here (no interpreter lock held inside it); wrapping the finished games into
                # GameHistory views is Python and stays on the main thread, inside the hand-off the call overlaps with
                shard = self._native_shard(temperature)
                if stream is None:
                    return shard.rounds(temperature, threshold, self.num_games, None)
                torch.cuda.set_device(self.model.backend.device)      # (device and stream are thread-local in torch)
                with torch.cuda.stream(stream):
                    return shard.rounds(temperature, threshold, self.num_games, None)

        while get("training_step") < self.config.training_steps and not get("terminate"):
            if not sharded:
                self.model.set_weights(get("weights"))
            if overlap:
                future = executor.submit(rounds_on_worker, self.config.visit_softmax_temperature_fn(trained_steps=get("training_step")),
                                         self.config.temperature_threshold)
                try:
                    if waiting is not None:          # the games the previous call finished (numbered below `waiting`)
                        t0 = time.perf_counter()
                        histories, slots = self._live["native"].collect(waiting, priorities_for=self.config)
                        self.finished_slots = slots
                        t1 = time.perf_counter()
                        hand_off(histories)
                        t2 = time.perf_counter()
                        spent = self.stats.setdefault("handoff_seconds", [0.0, 0.0, 0.0])     # collect (+ priorities), save_game, idle
                        spent[0] += t1 - t0
                        spent[1] += t2 - t1
                finally:
                    t3 = time.perf_counter()
                    waiting = future.result()
                    self.stats.setdefault("handoff_seconds", [0.0, 0.0, 0.0])[2] += time.perf_counter() - t3
            elif not test_mode:
                # every slot of the shard is one reference actor: its next game starts the moment one ends (:31-52), so
                # every search runs at full width (``refill_finished_games = False``: whole shards in lock-step)
                play = self.play_rounds if getattr(self.config, "refill_finished_games", True) else (
                    lambda t, th: self.play_games(t, th, False, "self", 0))
                hand_off(play(self.config.visit_softmax_temperature_fn(trained_steps=get("training_step")),
                              self.config.temperature_threshold))
            else:
                game_history = self.play_game(
                    0, self.config.temperature_threshold, False,
                    "self" if len(self.config.players) == 1 else self.config.opponent, self.config.muzero_player,
                )
                _remote(shared_storage.set_info, {
                    "episode_length": len(game_history.action_history) - 1,
                    "total_reward": sum(game_history.reward_history),
                    "mean_value": numpy.mean([value for value in game_history.root_values if value]),
                })
                if 1 < len(self.config.players):
                    _remote(shared_storage.set_info, {
                        "muzero_reward": sum(
                            reward for i, reward in enumerate(game_history.reward_history)
                            if game_history.to_play_history[i - 1] == self.config.muzero_player),
                        "opponent_reward": sum(
                            reward for i, reward in enumerate(game_history.reward_history)
                            if game_history.to_play_history[i - 1] != self.config.muzero_player),
                    })
            if not test_mode and self.config.self_play_delay:
                time.sleep(self.config.self_play_delay)
            if sharded:
                shared_storage.refresh(self.model)     # played counts out, control + (new) weights in
            if not test_mode and self.config.ratio:
                while (get("training_step") / max(1, get("num_played_steps")) < self.config.ratio
                       and get("training_step") < self.config.training_steps and not get("terminate")):
                    time.sleep(0.5)
                    if sharded:
                        shared_storage.refresh(self.model)
        if executor is not None:
            executor.shutdown(wait=True)
            if waiting is not None:          # the games of the last call
                histories, slots = self._live["native"].collect(waiting, priorities_for=self.config)
                self.finished_slots = slots
                hand_off(histories)
        if sharded and hasattr(shared_storage, "finish"):
            shared_storage.finish(self.model)
        self.close_game()

    def play_game(self, temperature, temperature_threshold, render, opponent, muzero_player):
        """self_play.py:110-183: one game (game slot 0, process-global numpy stream)."""
        self._no_device_draws("play_game")
        return self._play([0], temperature, temperature_threshold, render, opponent, muzero_player)[0]

    def play_games(self, temperature, temperature_threshold, render, opponent, muzero_player):
        """All ``num_games`` games of this shard in lock-step; returns their GameHistory list."""
        self._end_live()        # (games in progress under play_rounds end here: every game object is reset)
        if self.batched_game is not None:
            if opponent != "self" or render:
                raise NotImplementedError("the batched game protocol covers self-play without rendering")
            return self._play_batched(temperature, temperature_threshold)
        self._no_device_draws("the per-object game path (opponents, human play, rendering, unbatched shards)")
        if self.bank is not None and opponent == "self" and not render:
            return self._play_shard(temperature, temperature_threshold)
        return self._play(list(range(self.num_games)), temperature, temperature_threshold, render, opponent,
                          muzero_player)

    def _end_live(self, forget=True):
        """Ends the games in progress under ``play_rounds``: queued searches drained, the slot groups closed (their own game
        objects, native actors).  ``forget=False`` (``close_game``): the closed groups stay in ``_live``, where a finished run's
        groups and their engines' counters are still looked at -- not ``draw_counter``: a native actor's is gone with its handle."""
        self._drain_searches()
        live = self._live
        if live is None:
            return
        if forget:
            if self.device_draws:
                self._draw_counter = self.draw_counter        # (the next shard's searches go on counting)
            self._live = None
        for group in live["groups"]:
            group.close()

    def _check_observation(self, observation):
        # self_play.py:132-137 (same messages); ndarray observations of the right shape take the fast exit
        shape = self.config.observation_shape
        if getattr(observation, "shape", None) == shape:
            return
        got = numpy.array(observation).shape
        assert len(got) == 3, \
            f"Observation should be 3 dimensionnal instead of {len(got)} dimensionnal. Got observation of shape: {got}"
        assert got == shape, \
            f"Observation should match the observation_shape defined in MuZeroConfig. Expected {shape} but got {got}."

    def _count_search(self, n, engine, seconds):
        """``stats``: ``n`` searches of ``engine`` that took ``seconds`` of this thread's time."""
        stats = self.stats
        stats["search_seconds"] += seconds
        stats["searches"] += n
        stats["simulations"] += n * engine.num_simulations

    @staticmethod
    def _move_temps(temperature, histories, slots, threshold):
        """``move_temperature`` of the games of ``slots`` (their lengths are only read with a threshold)."""
        return move_temperature(temperature, [len(histories[s].action_history) for s in slots] if threshold else None, threshold)

    # ------------------------------------------------------------------ the ledger of per-object games
    @property
    def _record_legal(self):
        """config.reanalyse_search: the legal actions of every searched position go into the history (``legal_actions``, one
        list of ints per position) -- what DeviceGameStore(legal_masks=True) turns into the mask rows of its search sweep."""
        return bool(getattr(self.config, "reanalyse_search", False))

    def _start_game(self, s, batch, first=0):
        """A new game on slot ``s`` (self_play.py:118-123): its history; the first observation lands in ``batch[s - first]``
        (``batch`` None: nowhere)."""
        game, gh = self.games[s], GameHistory()
        observation = game.reset()
        gh.action_history.append(0)
        gh.observation_history.append(observation)
        gh.reward_history.append(0)
        gh.to_play_history.append(game.to_play())
        if self._record_legal:
            gh.legal_actions = []
        self._check_observation(observation)
        if batch is not None:
            batch[s - first] = observation
        return gh

    def _log_moves(self, slots, histories, result, actions, legal, batch, first, on_over):
        """
        One searched move of the per-object games of ``slots`` (self_play.py:139-172): game ``slots[k]`` plays ``actions[k]``
        and logs root ``k`` of ``result`` in ``histories[slots[k]]``; its new observation lands in ``batch[slots[k] - first]``.
        ``legal``: the lists the search was given.  ``on_over(k, s)`` is called for a game that is over (:129).  Everything
        that is not a call into a plugin object or an append to one of its history's lists is done once for the whole move:
        child_visits rows (visit / total, self_play.py:496-511) and root values come from two array operations.
        """
        cfg, games = self.config, self.games
        A, max_moves, record_legal = len(cfg.action_space), cfg.max_moves, self._record_legal
        shape = cfg.observation_shape if isinstance(cfg.observation_shape, tuple) else tuple(cfg.observation_shape)
        vis = result.visit_counts
        totals = vis.sum(1)
        rows = (vis / numpy.maximum(totals, 1)[:, None]).tolist()     # int / int true division, as Python's
        values = result.root_values.tolist()
        plain = bool((totals > 0).all()) and all(len(l) == A for l in result.legal_actions)
        for k, s in enumerate(slots):
            game, gh, action = games[s], histories[s], actions[k]
            if record_legal:
                gh.legal_actions.append([int(a) for a in legal[k]])
            observation, reward, done = game.step(action)
            if plain:
                gh.child_visits.append(rows[k])
                gh.root_values.append(values[k])
            else:      # illegal actions get 0, an unvisited root reports value 0 (self_play.py:496-511, :446-449)
                total, legal_set = int(totals[k]), set(result.legal_actions[k])
                gh.child_visits.append([int(vis[k][a]) / total if a in legal_set else 0 for a in cfg.action_space])
                gh.root_values.append(values[k] if total else 0)
            gh.action_history.append(action)
            gh.observation_history.append(observation)
            gh.reward_history.append(reward)
            gh.to_play_history.append(game.to_play())
            if getattr(observation, "shape", None) != shape:
                self._check_observation(observation)
            batch[s - first] = observation
            if done or len(gh.action_history) > max_moves:
                on_over(k, s)

    def _play_shard(self, temperature, temperature_threshold):
        """
        play_game (self_play.py:110-183) for all games of the shard through the REFERENCE plugin surface (B
        unmodified ``Game`` objects): self-play, no rendering, native stream bank.  Observations land in one persistent
        float32 batch as they are produced, legal-action lists are validated once per distinct list, actions and the
        history rows of a move come from array operations (``_log_moves``).
        Game by game the result equals the single-game actor's (tests/test_selfplay_shard.py).
        """
        cfg, games, G = self.config, self.games, len(self.games)
        batch = getattr(self, "_obs_batch", None)
        if batch is None or batch.shape != (G,) + tuple(cfg.observation_shape):
            batch = self._obs_batch = numpy.empty((G,) + tuple(cfg.observation_shape), numpy.float32)
        histories = [self._start_game(s, batch) for s in range(G)]
        store = None
        if cfg.stacked_observations > 0:
            store = self._frame_store(G)
            store.push(batch, None)
        active = list(range(G))
        moved = numpy.zeros(G, numpy.int32)
        while active:
            everyone = len(active) == G
            legal = [games[s].legal_actions() for s in active]
            to_play = [games[s].to_play() for s in active]
            if store is not None:
                stacked = store.stacked(None if everyone else active)
            else:
                stacked = batch if everyone else batch[active]
            t0 = time.perf_counter()
            result = self.engine.run(stacked, legal, to_play, True, (self.bank, active))
            self._count_search(len(active), self.engine, time.perf_counter() - t0)
            actions = self._select_actions_bank(result, active, self._move_temps(temperature, histories, active, temperature_threshold))
            over = set()
            self._log_moves(active, histories, result, actions, legal, batch, 0, lambda k, s: over.add(s))
            still = [s for s in active if s not in over]
            if store is not None and still:
                moved[active] = actions
                store.push(batch, moved)
            active = still
        return histories

    def _play(self, slots, temperature, temperature_threshold, render, opponent, muzero_player):
        """play_game (self_play.py:110-183) for the games of ``slots``, opponents and rendering included.  Moves searched on
        the stream bank are logged in bulk unless rendered; every other move goes through a ``Node`` as in the reference.
        Within a move the bulk-logged games are stepped first, then the others in slot order: when a shard mixes searched
        and opponent positions in one move, the plugin objects are not called in slot order (they are independent games)."""
        cfg = self.config
        A, G, record_legal = len(cfg.action_space), len(self.games), self._record_legal
        # the slots' current frames, for the frame store and the bulk ledger; a lone game without either keeps none
        with_store = cfg.stacked_observations > 0 and opponent == "self"
        frame = numpy.zeros((G,) + tuple(cfg.observation_shape), numpy.float32) if with_store or self.bank is not None else None
        histories = [None] * G
        for s in slots:
            histories[s] = self._start_game(s, frame)
            if render:
                self.games[s].render()
        # stacked observations of a self-play shard are assembled on the device from a frame store
        # (one upload of the new frames per move) instead of per-game numpy concatenations
        store = None
        if with_store:
            store = self._frame_store(G)
            store.push(frame, None)
        active = list(slots)
        while active:
            searching, stacked, stacked_by_slot = [], [], {}
            for s in active:
                gh = histories[s]
                self._check_observation(gh.observation_history[-1])
                st = None if store is not None else gh.get_stacked_observations(-1, cfg.stacked_observations, A)
                if opponent == "self" or muzero_player == self.games[s].to_play():
                    searching.append(s)
                    stacked.append(st)
                else:
                    stacked_by_slot[s] = st      # what THIS game's opponent sees (self_play.py:161-165)
            result, batch_actions, over = None, None, set()
            if searching:
                t0 = time.perf_counter()
                legal_lists = [self.games[s].legal_actions() for s in searching]
                result = self.engine.run(
                    stacked if store is None else store.stacked(searching),
                    legal_lists,
                    [self.games[s].to_play() for s in searching], True,
                    (self.bank, searching) if self.bank is not None else [self.rngs[s] for s in searching],
                )
                self._count_search(len(searching), self.engine, time.perf_counter() - t0)
                if self.bank is not None:
                    batch_actions = self._select_actions_bank(
                        result, searching, self._move_temps(temperature, histories, searching, temperature_threshold))
            position = {s: k for k, s in enumerate(searching)}
            # shard bookkeeping in bulk: with the stream bank the per-game Node objects are only needed for rendering
            in_bulk = batch_actions is not None and not render
            if in_bulk:
                self._log_moves(searching, histories, result, batch_actions, legal_lists, frame, 0, lambda k, s: over.add(s))
            for s in active:
                if in_bulk and s in position:
                    continue
                gh, game = histories[s], self.games[s]
                if s in position:
                    root = result.root(position[s])
                    t = move_temperature(temperature, len(gh.action_history), temperature_threshold)
                    action = batch_actions[position[s]] if batch_actions is not None else self._select_action(root, t, self.rngs[s])
                    if render:
                        print(f'Tree depth: {result.max_tree_depth[position[s]]}')
                        print(f"Root value for player {game.to_play()}: {root.value():.2f}")
                else:
                    action, root = self.select_opponent_action(opponent, stacked_by_slot[s], game)
                if record_legal:
                    gh.legal_actions.append([int(a) for a in (legal_lists[position[s]] if s in position else game.legal_actions())])
                observation, reward, done = game.step(action)
                if render:
                    print(f"Played action: {game.action_to_string(action)}")
                    game.render()
                gh.store_search_statistics(root, cfg.action_space)
                gh.action_history.append(action)
                gh.observation_history.append(observation)
                gh.reward_history.append(reward)
                gh.to_play_history.append(game.to_play())
                if done or len(gh.action_history) > cfg.max_moves:
                    over.add(s)
            still = [s for s in active if s not in over]
            if store is not None and still:
                moved = numpy.zeros(G, numpy.int32)
                for s in active:
                    frame[s] = numpy.asarray(histories[s].observation_history[-1])
                    moved[s] = histories[s].action_history[-1]
                store.push(frame, moved)
            active = still
        return [histories[s] for s in slots]

    def _play_batched(self, temperature, temperature_threshold):
        """
        play_game (self_play.py:110-183) for a shard behind the batched plugin protocol: per move ONE game
        call, ONE search, ONE action draw for all running games; the per-game GameHistory objects
        (field-identical to the per-object path, tests/test_selfplay_shard.py) are materialised at the end.
        While every game of the shard is still running (the common case) no index gathers / scatters happen.
        """
        cfg, g, B = self.config, self.batched_game, self.num_games
        A, k = len(cfg.action_space), int(cfg.stacked_observations)
        obs = numpy.asarray(g.reset())
        assert obs.shape == (B,) + tuple(cfg.observation_shape), \
            f"Observation should match the observation_shape defined in MuZeroConfig. Expected {(B,) + tuple(cfg.observation_shape)} but got {obs.shape}."
        obs_hist, act_hist, rew_hist = [obs], [numpy.zeros(B, numpy.int64)], [numpy.zeros(B, numpy.int64)]
        tp_hist = [numpy.asarray(g.to_play()).astype(numpy.int64)]
        visits_hist, value_hist, legal_hist = [], [], []
        alive = numpy.ones(B, bool)
        n_alive = B
        length = numpy.zeros(B, numpy.int64)
        everyone_idx = numpy.arange(B)
        move = 0
        store = None
        if k > 0:   # frames stay in HBM; the stacked inputs are assembled there (csrc/mzx_obs.h)
            store = self._frame_store(B)
            store.push(obs, None)
        while n_alive and move + 1 <= cfg.max_moves:      # len(action_history) <= max_moves, :129
            everyone = n_alive == B
            idx = everyone_idx if everyone else numpy.nonzero(alive)[0]
            if store is not None:
                stacked = store.stacked(None if everyone else idx)
            else:
                stacked = obs_hist[-1] if everyone else obs_hist[-1][idx]
            legal = g.legal_actions()
            if not everyone:
                legal = legal[idx] if isinstance(legal, numpy.ndarray) else [legal[i] for i in idx]
            to_play = tp_hist[-1] if everyone else tp_hist[-1][idx]
            t0 = time.perf_counter()
            t = move_temperature(temperature, move + 1, temperature_threshold)
            if self.device_draws:       # one fused move: streams are the shard slots, one counter per move
                result = self.engine.run(stacked, legal, to_play, True, None, streams=idx, counter=self._draw_counter, temperature=t)
                self._draw_counter += 1
            else:
                result = self.engine.run(stacked, legal, to_play, True, (self.bank, idx))
            self._count_search(len(idx), self.engine, time.perf_counter() - t0)
            chosen = result.actions if self.device_draws else self._select_actions_bank(result, idx, t)
            if everyone:
                actions = numpy.asarray(chosen, numpy.int64)
                visits, values = result.visit_counts, result.root_values
            else:
                actions = numpy.zeros(B, numpy.int64)
                actions[idx] = chosen
                visits = numpy.zeros((B, A), numpy.int32)
                visits[idx] = result.visit_counts
                values = numpy.zeros(B, numpy.float64)
                values[idx] = result.root_values
            obs, reward, done = g.step(actions, alive if everyone else alive.copy())
            visits_hist.append(visits); value_hist.append(values); legal_hist.append(legal_mask_row(legal, idx, B, A))
            obs_hist.append(numpy.asarray(obs)); act_hist.append(actions)
            if store is not None:
                store.push(obs_hist[-1], actions)
            rew_hist.append(numpy.asarray(reward)); tp_hist.append(numpy.asarray(g.to_play()).astype(numpy.int64))
            if everyone:
                length += 1
            else:
                length[idx] += 1
            done = numpy.asarray(done, bool)
            if done.any():
                alive = alive & ~done
                n_alive = int(alive.sum())
            move += 1
        # ---- per-game records: transpose once to game-major, a view per game
        by_game = lambda seq: numpy.ascontiguousarray(numpy.swapaxes(numpy.stack(seq), 0, 1))
        vis = vals = legal_mask = None
        if visits_hist:
            vis, vals = by_game(visits_hist), by_game(value_hist)              # [B][n_moves][A], [B][n_moves]
            if any(m is not None for m in legal_hist):
                legal_mask = by_game([numpy.ones((B, A), bool) if m is None else m for m in legal_hist])
        return shard_views(A, by_game(obs_hist), by_game(act_hist), by_game(rew_hist), by_game(tp_hist), vis, vals, legal_mask,
                           length.tolist())

    # ------------------------------------------------------------------ continuous play: finished slots are refilled
    def play_rounds(self, temperature, temperature_threshold, min_games=None, max_rounds=None):
        """
        Self-play of the shard WITHOUT lock-step game boundaries: the reference actor starts its next game the moment
        one ends (self_play.py:31-52) -- here every slot s of the shard is such an actor (its ``Game`` object and its
        numpy stream ``RandomState(seed + s)`` live on from game to game, exactly the sequence a lone reference-style
        actor seeded ``seed + s`` produces, tests/test_selfplay_refill.py), and ALL slots are searched together in every
        round: when the game of slot s ends its GameHistory is handed out and the slot restarts at once, so every
        search launch runs at the full shard width (``play_games`` searches a thinning batch until the longest game of
        the shard ends: connect4 games average 21 moves and last up to 42).

        Plays rounds (one move of every slot) until at least ``min_games`` games have finished (default: one shard's
        worth) or ``max_rounds`` rounds were played; returns the games that finished, in the order they did.  Games in
        progress stay in the shard and continue with the next call.  ``temperature`` applies to the games that START
        during this call (the reference reads it once per game, self_play.py:39-41); weights may be refreshed between
        calls, i.e. between two searches -- a game can straddle a refresh (deliberate: the alternative is lock-step).
        Batched games need the optional ``reset_games(idx)`` hook; without it, and for a single-game actor, this falls
        back to ``play_games``.
        """
        if native_rounds.handoff_wanted(self.config):
            native_rounds.check_handoff(self)       # (NotImplementedError without config.device_games)
        if native_rounds.resident_wanted(self.config):
            native_rounds.check_resident(self)      # (NotImplementedError for what the resident loop does not cover)
        if self.bank is None or (self.batched_game is not None and not hasattr(self.batched_game, "reset_games")):
            self.finished_slots = list(range(self.num_games))
            return self.play_games(temperature, temperature_threshold, False, "self", 0)
        min_games = self.num_games if min_games is None else int(min_games)
        self.finished_slots = []      # slot of every returned game, in the same order (slot s = the actor seeded seed + s)
        if self.batched_game is not None:
            return self._rounds_batched(temperature, temperature_threshold, min_games, max_rounds)
        self._no_device_draws("the per-object shard")
        return self._rounds_shard(temperature, temperature_threshold, min_games, max_rounds)

    def _slot_spans(self, G, batched):
        """
        The slots of a shard of G games as ONE group, or as several that take turns on the GPU: while the search of one
        group runs, the host steps, draws and logs another.  Slots are independent actors (own game, own stream) and the
        library searches a network on ONE arithmetic whatever the shard size (wide residual networks: csrc/mzx_row_search.h
        wide_search_route), so which slots share a launch does not change what any of them plays -- bit for bit, on the
        device too (tests/test_gpu_parity.py: 1024 connect4 games, two groups against one).
        ``config.self_play_pipeline``: True / False; unset, the protocol's own threshold:
          per-object games (``batched`` False): from 1024 games on.  The Python work of the reference plugin surface (a third
            of the wall for connect4 at 1024 games) hides behind the other half's search, and each half still fills the
            chip: the residual whole-search kernels run a workgroup per tree or pair of trees, so a search of fewer than
            ~512 trees takes as long as one of 512 and two half searches would cost more than they hide.  Always two groups.
          the batched protocol: when the host side of a move weighs as much as its search -- a fully connected network (one
            whole-search launch of a fraction of a millisecond) from 2048 games on.  Residual networks are search-bound
            (connect4 at 1024 games: 98 % of the wall is the search, and two searches of 512 trees cost 14 % more than one
            of 1024): one group.  ``config.self_play_groups``: how many groups take turns (default two).  A round of k
            groups lasts max(search + host work of ONE group, k x host work of a group), so a latency-bound search (C2:
            0.2 ms for 1024 trees as for 4096) would want more, smaller groups -- measured on the natively played C2 shard
            (profiles/r06_native_rounds.txt): four groups of 1024 on four streams 5.1 M steps/s against 10.3 M with two
            (queueing a search took 97 us instead of 40).
        """
        cfg = self.config
        want = getattr(cfg, "self_play_pipeline", None)
        if want is None:
            want = (cfg.network == "fullyconnected" and G >= 2048) if batched else G >= 1024
        if not want or G < 2:
            return [(0, G)]
        groups = max(2, min(int(getattr(cfg, "self_play_groups", None) or 2), G)) if batched else 2
        edges = [(G * g + groups - 1) // groups for g in range(groups + 1)]
        return [(edges[g], edges[g + 1]) for g in range(groups) if edges[g + 1] > edges[g]]

    def _search_job(self, group, stacked, legal, to_play, stream):
        """One search of a slot group of per-object games (runs on the worker thread when the shard is pipelined, under the
        submitting thread's device and stream: both are thread-local in torch)."""
        t0 = time.perf_counter()
        if stream is not None:
            torch.cuda.set_device(self.model.backend.device)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            result = group.engine.run(stacked, legal, to_play, True, (self.bank, group.slots))
        return result, time.perf_counter() - t0

    def _run_rounds(self, groups, begin, consume, may_queue_ahead, min_games, max_rounds):
        """
        The round loop of ``play_rounds``: a round is one move of every slot -- every group without a pending search begins
        one, then the groups are consumed in order -- until ``min_games`` games finished or ``max_rounds`` rounds were played.
        ``begin(group, done, rounds)`` queues the group's next search (``group.pending``; ``done`` games finished so far in
        round ``rounds`` of this call); ``consume(group)`` completes it, plays the group's move and returns the games that
        ended.  Several groups take turns: right after its move a group's NEXT search is begun, so that it runs while the
        host plays the groups after it, when another round can follow and ``may_queue_ahead(k, done)`` agrees.  The protocols
        differ in that rule alone:
          per-object games   queue unless this is KNOWN to be the last round (``done < min_games``).  The search may then
                             wait across the end of the call: ``begin`` keeps the streams' states when the call may end
                             first (``_drain_searches`` gives the draws back), ``_rounds_shard`` waits for the worker.
          batched protocol   queue only when CERTAIN to be consumed in this call: even if every game of the groups still to
                             play ended now, the call would go on.  Nothing is in flight between calls.
        """
        finished, rounds = [], 0
        while len(finished) < min_games and (max_rounds is None or rounds < max_rounds):
            for group in groups:
                if group.pending is None:     # (a pipelined per-object shard may hold a search from the end of the last call)
                    begin(group, len(finished), rounds)
            for k, group in enumerate(groups):
                finished.extend(consume(group))
                if (k + 1 < len(groups) and (max_rounds is None or rounds + 1 < max_rounds)
                        and may_queue_ahead(k, len(finished))):
                    begin(group, len(finished), rounds)
            rounds += 1
        return finished

    def _rounds_shard(self, temperature, temperature_threshold, min_games, max_rounds):
        """``play_rounds`` through the reference plugin surface (B ``Game`` objects); bookkeeping as ``_play_shard``.  Two
        slot groups: the search of one runs on a worker thread (inside the C call / the stream synchronisation, both of
        which release the GIL) while this thread steps the other group's ``Game`` objects."""
        cfg, games, G = self.config, self.games, len(self.games)
        live = self._live
        if live is None:
            live = self._live = dict(histories=[None] * G, groups=[])
            spans = self._slot_spans(G, batched=False)
            for first, last in spans:
                n = last - first
                group = ObjectGroup(first, n, self.engine if len(spans) == 1 else BatchedMCTS(cfg, self.model, n),
                                    cfg.observation_shape, temperature)
                live["groups"].append(group)
                for s in group.slots:
                    live["histories"][s] = self._start_game(s, group.batch, first)
                if cfg.stacked_observations > 0:
                    group.store = (self._frame_store(G) if len(spans) == 1 else
                                   observations_mod.FrameStore(cfg, n, self.model.backend))
                    group.store.push(group.batch, None)
        histories, groups = live["histories"], live["groups"]
        pipelined = len(groups) > 1
        if pipelined and getattr(self, "_search_worker", None) is None:
            import concurrent.futures
            self._search_worker = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="mzx-search")

        def begin(group, done, rounds):
            slots = group.slots
            legal = [games[s].legal_actions() for s in slots]
            to_play = [games[s].to_play() for s in slots]
            stacked = group.store.stacked(None) if group.store is not None else group.batch
            if pipelined:
                device = self.model.backend.device
                stream = torch.cuda.current_stream(device) if device.type == "cuda" else None
                # A search queued across the end of this call is consumed by the NEXT play_rounds call; should play_games /
                # close_game come instead, its result is dropped -- and the root noise / tie words it drew are given back
                # (_drain_searches), so that the slots' streams stay those of lone actors.  The states are only kept when
                # this call can actually end before the result is consumed.
                may_be_last = done + G >= min_games or (max_rounds is not None and rounds + 2 >= max_rounds)
                group.streams_before = [self.bank.get_state(s) for s in slots] if may_be_last else None
                group.pending = self._search_worker.submit(self._search_job, group, stacked, legal, to_play, stream)
            else:
                job = self._search_job(group, stacked, legal, to_play, None)
                group.pending = PendingSearch(lambda: job)

        def consume(group):
            pending, group.pending = group.pending, None
            result, seconds = pending.result()
            slots, first, store = group.slots, group.first, group.store
            self._count_search(group.n, group.engine, seconds)
            actions = self._select_actions_bank(result, slots, self._move_temps(group.temps, histories, slots, temperature_threshold))
            group.moved[:] = actions
            finished, restarted = [], []

            def over(k, s):     # self_play.py:129: the game is over ... and the slot's next game begins (:31-52)
                finished.append(histories[s])
                self.finished_slots.append(s)
                histories[s] = self._start_game(s, group.batch, first)
                group.temps[k], group.moved[k] = temperature, 0
                restarted.append(k)

            self._log_moves(slots, histories, result, actions, result.legal_actions, group.batch, first, over)
            if store is not None:
                store.clear_history(restarted)
                store.push(group.batch, group.moved)
            return finished

        finished = self._run_rounds(groups, begin, consume, lambda k, done: done < min_games, min_games, max_rounds)
        # nothing runs on the worker between calls (the caller may load new weights): a search queued for the next round
        # finishes here, its result waits in the group (a round is one move of EVERY slot, so the call ends on a round
        # boundary; the slots of that group have already drawn their root noise for the next move -- in the order a lone
        # actor draws it)
        for group in groups:
            if group.pending is not None:
                group.pending.result()
        return finished

    def _rounds_batched(self, temperature, temperature_threshold, min_games, max_rounds):
        """
        ``play_rounds`` behind the batched plugin protocol: per round and slot group ONE game call, ONE library call for
        the host side of the search (``mzx_selfplay_search``: draws, staging, upload, launch, download), ONE for the
        streams' advance and the action draw (``mzx_selfplay_select``).  A move is logged as one row of a handful
        of ring arrays (``shard_play.BatchedGroup``); a finished game is a copy of its slot's rows, handed out as a
        ``ShardGameHistory`` view (games that started and ended together share one record).

        Slot groups (``_slot_spans``): a large shard of a cheaply searched network runs as two groups with their own
        game object, engine and staging that take turns on the GPU -- the search of one group is queued, the host
        draws / steps / logs the other group, then waits for the first (an event behind the asynchronous library call;
        no worker thread).  Slots are independent actors with their own stream: which of them share a launch changes
        nothing any of them plays (tests/test_selfplay_refill.py, tests/test_selfplay_move.py); games finish in the
        order (round, slot) either way.
        """
        cfg, B = self.config, self.num_games
        if native_rounds.usable(self):
            # the game steps inside the library: the whole loop below runs there (mzx_selfplay_rounds), same schedule, same
            # draws, same games (mzx/native_rounds.py; config.native_rounds = False keeps this loop on such a game)
            finished, slots = self._native_shard(temperature).play(temperature, temperature_threshold, min_games, max_rounds)
            self.finished_slots += slots
            return finished
        if self._live is None:
            spans = self._slot_spans(B, batched=True)
            groups = []
            for first, last in spans:
                game = self.batched_game if len(spans) == 1 else type(self.batched_game)(self._game_seeds[first:last])
                engine = self.engine if len(spans) == 1 else BatchedMCTS(cfg, self.model, last - first)
                engine.draw_seed = self.draw_seed
                groups.append(_BatchedGroup(self, game, first, last - first, engine, temperature))
            self._live = dict(groups=groups)
        groups = self._live["groups"]

        def begin(group, done, rounds):
            t0 = time.perf_counter()
            legal = group.legal = group.game.legal_actions()
            stacked = group.store.stacked(None) if group.store is not None else group.obs
            if self.device_draws:     # the group's search number is its counter, its slots are the streams
                group.pending = group.engine.run(stacked, legal, group.tp, True, None, streams=group.streams,
                                                 counter=group.counter, _asynchronous=True,
                                                 temperature=group.move_temps(temperature_threshold))
                group.counter += 1
            else:
                group.pending = group.engine.run(stacked, legal, group.tp, True, (self.bank, group.streams),
                                                 _defer_advance=True, _asynchronous=True)
            self._count_search(0, group.engine, time.perf_counter() - t0)

        def consume(group):
            t0 = time.perf_counter()
            pending, group.pending = group.pending, None
            result = pending.result()
            self._count_search(group.n, group.engine, time.perf_counter() - t0)
            finished, slots = group.play(self, result, temperature, temperature_threshold)
            self.finished_slots += slots
            return finished

        return self._run_rounds(groups, begin, consume,
                                lambda k, done: done + sum(g.n for g in groups[k + 1:]) < min_games, min_games, max_rounds)

    def _native_shard(self, temperature):
        """The actors of a natively played shard (created with the first round; ``temperature``: of the games that start then)."""
        if self._live is None:
            shard = native_rounds.NativeShard(self, temperature)
            self._live = dict(groups=shard.groups, native=shard)
        return self._live["native"]

    def _frame_store(self, num_games):
        """The shard's device frame store: allocated once per actor, rewound for every game."""
        store = getattr(self, "_store", None)
        if store is None or store.G != num_games:
            store = self._store = observations_mod.FrameStore(self.config, num_games, self.model.backend)
        else:
            store.reset()
        return store

    def _drain_searches(self):
        """
        A search a pipelined ``play_rounds`` call queued for its next round and nobody will consume (``play_games`` or
        ``close_game`` follows): waited for, dropped, and the draws it took from its slots' streams are undone.  A failure
        of the worker thread surfaces here instead of disappearing.
        """
        for group in (self._live or {}).get("groups", ()):
            pending, group.pending = group.pending, None
            if pending is None:
                continue
            if self.device_draws:
                group.counter -= 1        # (the dropped search's draws are a function of this counter: taken again)
            try:
                pending.result()
            except Exception as e:       # (the search is being discarded anyway; the failure is not)
                warnings.warn(f"a queued self-play search failed on the worker thread: {e!r}")
            before, group.streams_before = group.streams_before, None
            if before is not None and self.bank is not None:
                for s, state in zip(group.slots, before):
                    self.bank.set_state(s, state)

    def close_game(self):
        self._end_live(forget=False)
        worker = getattr(self, "_search_worker", None)
        if worker is not None:
            worker.shutdown(wait=True)
            self._search_worker = None
        if self.batched_game is not None:
            self.batched_game.close()
        for g in self.games:
            g.close()

    def select_opponent_action(self, opponent, stacked_observations, game=None):
        """self_play.py:188-220"""
        game = self.game if game is None else game
        if opponent == "human":
            root, mcts_info = MCTS(self.config).run(self.model, stacked_observations, game.legal_actions(),
                                                    game.to_play(), True)
            print(f'Tree depth: {mcts_info["max_tree_depth"]}')
            print(f"Root value for player {game.to_play()}: {root.value():.2f}")
            print(f"Player {game.to_play()} turn. MuZero suggests {game.action_to_string(self.select_action(root, 0))}")
            return game.human_to_action(), root
        elif opponent == "expert":
            return game.expert_agent(), None
        elif opponent == "random":
            assert game.legal_actions(), f"Legal actions should not be an empty array. Got {game.legal_actions()}."
            assert set(game.legal_actions()).issubset(set(self.config.action_space)), \
                "Legal actions should be a subset of the action space."
            return numpy.random.choice(game.legal_actions()), None
        else:
            raise NotImplementedError(
                'Wrong argument: "opponent" argument should be "self", "human", "expert" or "random"'
            )

    def _select_actions_bank(self, result, searching, temps):
        """
        SelfPlay.select_action (self_play.py:222-245) for all searched games of a move, the draws taken from
        the native stream bank.  Same arithmetic as the reference per game: int32 counts ** (1 / T), the
        sequential Python ``sum``, numpy.random.choice's cumulative sum / renormalisation / right-bisection.
        """
        k = len(searching)
        A = self.engine.A
        if self.engine.fused_move and getattr(result, "legal_array", None) is not None and A <= 4096:
            return self._select_actions_native(result, temps)
        counts = numpy.zeros((k, A), numpy.int32)     # in CHILD order (= legal-action order), zero padded
        n = numpy.empty(k, numpy.int32)
        if isinstance(result.legal_actions, numpy.ndarray):
            legal_arr = result.legal_actions
            n[:] = (legal_arr >= 0).sum(1)
            counts = numpy.where(legal_arr >= 0, numpy.take_along_axis(result.visit_counts, numpy.maximum(legal_arr, 0), 1), 0).astype(numpy.int32)
        elif result.shared_legal is not None:          # one list for every game: gather its columns once
            shared = numpy.asarray(result.shared_legal, numpy.int64)
            n[:] = shared.size
            counts[:, : shared.size] = result.visit_counts[:, shared]
        else:
            for r, legal in enumerate(result.legal_actions):
                n[r] = len(legal)
                counts[r, : n[r]] = result.visit_counts[r][legal]
        actions = numpy.zeros(k, numpy.int64)
        temps = numpy.full(k, float(temps)) if numpy.isscalar(temps) else numpy.asarray(temps, dtype=numpy.float64)
        greedy = numpy.nonzero(temps == 0)[0]
        if greedy.size:
            masked = numpy.where(numpy.arange(A)[None, :] < n[greedy, None], counts[greedy], -1)
            actions[greedy] = numpy.argmax(masked, axis=1)           # first maximum, like numpy.argmax on the child list
        uniform = numpy.nonzero(numpy.isinf(temps))[0]
        if uniform.size:
            actions[uniform] = self.bank.randint([searching[r] for r in uniform], n[uniform])
        rest = numpy.nonzero((temps != 0) & ~numpy.isinf(temps))[0]
        distinct = numpy.unique(temps[rest]) if rest.size else ()
        for t in distinct:
            # the whole-batch shortcut (no index gather) only when ONE temperature covers every game: with several,
            # each game must be drawn exactly once, under its own temperature
            rows = rest if (rest.size == k and len(distinct) == 1) else rest[temps[rest] == t]
            dist = counts[rows] ** (1 / float(t))                    # int32 ** float -> float64 pow, elementwise (numpy's own)
            # sum / normalise / cumulative sum / bisection + the one random_sample() per game: native, one call
            stream = searching if rows.size == k else [searching[r] for r in rows]
            actions[rows] = self.bank.choice_weighted(stream, dist, n[rows])
        if isinstance(result.legal_actions, numpy.ndarray):
            return result.legal_actions[numpy.arange(k), actions].astype(numpy.int64)
        if result.shared_legal is not None:
            return [result.shared_legal[a] for a in actions.tolist()]
        return [result.legal_actions[r][int(actions[r])] for r in range(k)]

    def _select_actions_native(self, result, temps):
        """
        ``mzx_selfplay_select``: the streams consume the search's tie-break words (when ``run`` deferred that), then
        every game's action is drawn -- one pass over the bank on the library's host threads.  The power
        ``visit_count ** (1 / T)`` stays numpy's own: a table over 0 .. num_simulations per temperature, computed
        with the reference's expression (int32 array ** float) and indexed by the library.
        """
        lib, bank = self.model.backend.lib, self.bank
        B, A = result.legal_array.shape
        if numpy.isscalar(temps):
            single, temps = float(temps), numpy.full(B, float(temps))
        else:
            temps = numpy.ascontiguousarray(temps, dtype=numpy.float64)
            first = temps[0]
            single = float(first) if (temps == first).all() else None       # the common case: one temperature for the shard
        if single is not None:
            key = () if single == 0 or math.isinf(single) else (single,)
        else:
            finite = temps[(temps != 0) & ~numpy.isinf(temps)]
            key = tuple(numpy.unique(finite).tolist())
        # power tables (visit_count ** (1 / T) over 0 .. num_simulations + 1, numpy's own pow) per set of temperatures, kept
        stride = self.engine.num_simulations + 2
        peak = int(result.visit_counts.max()) if key else 0
        if peak >= stride:
            stride = peak + 1
        cache = self.__dict__.setdefault("_pow_tables", {})
        entry = cache.get((key, stride))
        if entry is None:
            distinct = numpy.array(key, numpy.float64)
            table = (numpy.ascontiguousarray(numpy.stack([numpy.arange(stride, dtype="int32") ** (1 / t) for t in key]))
                     if key else None)
            entry = cache[(key, stride)] = (table, distinct)
        table, distinct = entry
        mv = _lib.Move()
        mv.num_games, mv.action_space_size, mv.num_threads = B, A, bank.threads
        mv.streams, mv.legal_actions = result.streams.ctypes.data, result.legal_array.ctypes.data
        visits = numpy.ascontiguousarray(result.visit_counts, dtype=numpy.int32)
        actions = numpy.empty(B, numpy.int64)
        words = result.pending_words
        result.pending_words = None
        lib.check(lib.mzx_selfplay_select(bank.handle, ctypes.byref(mv), result.n_legal.ctypes.data,
                                          None if words is None else words.ctypes.data, visits.ctypes.data,
                                          temps.ctypes.data, None if table is None else table.ctypes.data, stride,
                                          distinct.ctypes.data if distinct.size else None, int(distinct.size),
                                          actions.ctypes.data))
        if isinstance(result.legal_actions, numpy.ndarray):
            return actions
        return actions.tolist()

    @staticmethod
    def _select_action(node, temperature, rng):
        visit_counts = numpy.array([child.visit_count for child in node.children.values()], dtype="int32")
        actions = [action for action in node.children.keys()]
        if temperature == 0:
            action = actions[numpy.argmax(visit_counts)]
        elif temperature == float("inf"):
            action = rng.choice(actions)
        else:
            # See paper appendix Data Generation
            dist = visit_counts ** (1 / temperature)
            dist = dist / sum(dist)
            action = rng.choice(actions, p=dist)
        return action

    @staticmethod
    def select_action(node, temperature):
        """self_play.py:222-245 (process-global numpy stream, like the reference)."""
        return SelfPlay._select_action(node, temperature, numpy.random.mtrand._rand)
