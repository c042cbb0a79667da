"""
Shared checks of RESIDENT rounds (config.device_games; include/mzx.h mzx_actor_set_resident, csrc/mzx_resident.h), run by
tests/test_resident_rounds.py on the serial build and by tests/test_gpu_resident_rounds.py on the product library.

The comparator is never the code under test alone: it is the native round loop on device draws with config.device_games
unset, on the same library -- the loop tests/test_device_draws.py holds to the Python loop.  "Same" means: games field for
field in the same order with the same finished_slots, the same draw_counter, identical searches / simulations stats, host
bank streams untouched, and at the end legal_actions() / to_play() / observation of every group's game object equal.
Every resident run also asserts THAT IT WAS RESIDENT (the assertions that fail where the flag is ignored): the shard says
so, the rounds committed on the device are the rounds played, and the host synchronisations are bounded by the chunks and
repairs, not by the rounds.  chunk = 3 throughout: calls straddle chunk ends and the log ring wraps.
"""
import copy
import ctypes

import numpy
import torch

from device_draws_cases import _same_games
from mzx import _lib, configs, games, models, search, self_play, synthetic

CHUNK = 3
FOREVER = 1 << 60


def _weights(backend, cfg, seed=21):
    return synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), seed)


def make_shard(backend, Game, cfg, weights, B, seed, resident, pipeline=True, **extra):
    c = copy.copy(cfg)
    c.native_rounds, c.self_play_pipeline, c.device_draws = True, pipeline, True
    if resident:
        c.device_games, c.device_games_chunk = True, CHUNK
    for k, v in extra.items():
        setattr(c, k, v)
    games.NativeBatchedGame.backend = backend
    return self_play.SelfPlay({"weights": weights}, Game, c, seed, num_games=B, _backend=backend)


def play(shard, calls):
    out, slots = [], []
    for temperature, kwargs in calls:
        got = shard.play_rounds(temperature, shard.config.temperature_threshold, **kwargs)
        assert len(got) == len(shard.finished_slots)
        out += got
        slots += shard.finished_slots
    return out, slots


def positions(shard):
    """What every group's game object says between calls: legal rows, side to move, observation."""
    out = []
    for g in shard._live["groups"]:
        game = g.game
        out.append((game.legal_actions(), numpy.asarray(game.to_play()), game._observation()))
    return out


def assert_was_resident(shard, B):
    live = shard._live
    assert live is not None and live.get("native") is not None and getattr(live["native"], "resident", False) is True
    assert "resident" in shard.stats, "the round loop kept no resident counters: config.device_games was ignored"
    st = shard.stats["resident"]
    rounds = shard.stats["searches"] // B
    assert shard.stats["searches"] == rounds * B
    assert st[0] == rounds * len(live["groups"]), (st, rounds)       # every group committed every round on the device
    assert st[3] <= 2 * st[1] + 3 * st[2], st                      # synchronisations: per chunk and repair, not per round
    assert st[5] > 0
    return st


def run(backend, Game, cfg, weights, B, seed, calls, resident, pipeline=True, **extra):
    shard = make_shard(backend, Game, cfg, weights, B, seed, resident, pipeline, **extra)
    before = [shard.bank.get_state(k) for k in range(B)]
    out, slots = play(shard, calls)
    result = dict(games=(out, slots), counter=shard.draw_counter, stats=dict(shard.stats), positions=positions(shard),
                  groups=len(shard._live["groups"]))
    for x, y in zip(before, [shard.bank.get_state(k) for k in range(B)]):      # no host stream was read or advanced
        assert x[2] == y[2] and (x[1] == y[1]).all()
    if resident:
        result["resident"] = assert_was_resident(shard, B)
    else:
        assert not getattr(shard._live["native"], "resident", False) and "resident" not in shard.stats
    shard.close_game()
    return result


def assert_same(a, b):
    _same_games(a["games"], b["games"])
    for x, y in zip(a["games"][0], b["games"][0]):
        for u, v in zip(x.observation_history, y.observation_history):
            assert numpy.asarray(u).dtype == numpy.asarray(v).dtype
    assert a["counter"] == b["counter"] > 0
    assert a["stats"]["searches"] == b["stats"]["searches"] and a["stats"]["simulations"] == b["stats"]["simulations"]
    assert a["groups"] == b["groups"]
    for (l1, t1, o1), (l2, t2, o2) in zip(a["positions"], b["positions"]):
        assert numpy.array_equal(l1, l2) and numpy.array_equal(t1, t2)
        assert o1.dtype == o2.dtype and numpy.array_equal(o1, o2)


def both(backend, Game, cfg, B, seed, calls, pipeline=True, weights=None, **extra):
    weights = _weights(backend, cfg) if weights is None else weights
    resident = run(backend, Game, cfg, weights, B, seed, calls, True, pipeline, **extra)
    host = run(backend, Game, cfg, weights, B, seed, calls, False, pipeline, **extra)
    assert_same(resident, host)
    return resident, host


# ---- the cases ----------------------------------------------------------------------------------------------------------

TICTACTOE_CALLS = [(1.0, dict(max_rounds=7, min_games=FOREVER)), (0.5, dict(max_rounds=4, min_games=FOREVER)),
                   (0.25, dict(max_rounds=9, min_games=FOREVER))]


def tictactoe_cfg():
    return configs.tictactoe(num_simulations=8, temperature_threshold=4)


def check_tictactoe(backend):
    """Wins and draws, restarts, the threshold gate, temperatures carried per game across calls, restricted legal sets."""
    resident, _ = both(backend, games.TicTacToeNative, tictactoe_cfg(), 5, 7, TICTACTOE_CALLS)
    out, slots = resident["games"]
    assert resident["groups"] == 2 and len(out) >= 8 and all(slots.count(s) >= 2 for s in range(5))
    assert len({len(g.action_history) for g in out}) > 1


def check_connect4(backend, B=4, calls=None):
    """Gravity, float64 planes, the legal-mask column of the log (full columns)."""
    cfg = configs.connect4(num_simulations=4, blocks=1, channels=8)
    calls = calls or [(1.0, dict(max_rounds=30, min_games=FOREVER)), (0.0, dict(max_rounds=30, min_games=FOREVER))]
    resident, _ = both(backend, games.Connect4Native, cfg, B, 3, calls)
    assert resident["groups"] == 2 and len(resident["games"][0]) >= B


def check_gomoku(backend):
    """The max_moves cut; 121 actions: two passes of the legal-row compaction."""
    cfg = configs.gomoku(num_simulations=3, blocks=1, channels=8, max_moves=12)
    calls = [(1.0, dict(max_rounds=14, min_games=FOREVER)), (0.5, dict(max_rounds=13, min_games=FOREVER))]
    resident, _ = both(backend, games.GomokuNative, cfg, 3, 5, calls, pipeline=False)
    out = resident["games"][0]
    assert len(out) == 6 and all(len(g.action_history) == 13 for g in out)


def check_synthetic(backend):
    """The whole-search route of a fully connected network, whole groups finishing in one round, two players."""
    cfg = configs.cartpole(num_simulations=7, max_moves=5, action_space=list(range(3)), observation_shape=(2, 1, 3),
                           players=list(range(2)))
    Native = games.make_native_synthetic_game(cfg.observation_shape, 3, 2)
    calls = [(1.0, dict(max_rounds=7, min_games=FOREVER)), (0.5, dict(max_rounds=6, min_games=FOREVER))]
    resident, _ = both(backend, Native, cfg, 12, 11, calls, weights=_weights(backend, cfg, 5))
    out, slots = resident["games"]
    assert len(out) == 24 and all(len(g.action_history) == 6 for g in out) and all(slots.count(s) == 2 for s in range(12))


def check_halt_and_repair(backend):
    """Equal priors everywhere on a 4-word tape: every search overflows, every round halts and is repaired."""
    old = search.TAPE_WORDS
    search.TAPE_WORDS = 4
    try:
        cfg = configs.cartpole(num_simulations=25, max_moves=4)
        Native = games.make_native_synthetic_game(cfg.observation_shape, len(cfg.action_space), 1)
        weights = {k: torch.zeros_like(v) if v.dtype.is_floating_point else v
                   for k, v in models.MuZeroNetwork(cfg, _backend=backend).state_dict().items()}
        calls = [(1.0, dict(max_rounds=5, min_games=FOREVER)), (0.5, dict(max_rounds=4, min_games=FOREVER))]
        resident, host = both(backend, Native, cfg, 5, 7, calls, weights=weights)
        assert resident["resident"][2] > 0 and resident["stats"]["native_phase_seconds"][4] > 0
        assert host["stats"]["native_phase_seconds"][4] > 0, "the comparator took the retry path too"
    finally:
        search.TAPE_WORDS = old


def check_min_games(backend):
    """min_games: whole chunks, enough games; the host loop given that many rounds plays the same games."""
    cfg, weights = tictactoe_cfg(), None
    weights = _weights(backend, cfg)
    resident = run(backend, games.TicTacToeNative, cfg, weights, 5, 7, [(1.0, dict(min_games=3))], True)
    rounds = resident["stats"]["searches"] // 5
    assert rounds % CHUNK == 0 and rounds > 0 and len(resident["games"][0]) >= 3
    host = run(backend, games.TicTacToeNative, cfg, weights, 5, 7, [(1.0, dict(max_rounds=rounds, min_games=FOREVER))], False)
    assert_same(resident, host)


def check_three_groups(backend):
    """Three groups: the finishing order is (round, group, slot)."""
    cfg = configs.tictactoe(num_simulations=8)
    calls = [(1.0, dict(max_rounds=8, min_games=FOREVER)), (0.5, dict(max_rounds=10, min_games=FOREVER))]
    resident, _ = both(backend, games.TicTacToeNative, cfg, 11, 7, calls, self_play_groups=3)
    assert resident["groups"] == 3 and len(resident["games"][0]) >= 11


def check_draw_counter(backend):
    """Saved, clobbered and restored between two calls -> the same games; also across the two loops."""
    cfg = tictactoe_cfg()
    weights = _weights(backend, cfg)
    whole = run(backend, games.TicTacToeNative, cfg, weights, 5, 7, TICTACTOE_CALLS, False)
    saved = {}
    for resident in (True, False):
        shard = make_shard(backend, games.TicTacToeNative, cfg, weights, 5, 7, resident)
        first = play(shard, TICTACTOE_CALLS[:1])
        saved[resident] = shard.draw_counter
        shard.draw_counter = saved[resident] + 1000
        assert shard.draw_counter == saved[resident] + 1000
        shard.draw_counter = saved[resident]
        rest = play(shard, TICTACTOE_CALLS[1:])
        if resident:
            assert_was_resident(shard, 5)
        shard.close_game()
        _same_games((first[0] + rest[0], first[1] + rest[1]), whole["games"])
    assert saved[True] == saved[False]
    # the value one loop saved restores the other: the counter means the same in both
    for resident in (True, False):
        shard = make_shard(backend, games.TicTacToeNative, cfg, weights, 5, 7, resident)
        first = play(shard, TICTACTOE_CALLS[:1])
        shard.draw_counter = 5
        shard.draw_counter = saved[not resident]
        rest = play(shard, TICTACTOE_CALLS[1:])
        assert shard.draw_counter == whole["counter"]
        shard.close_game()
        _same_games((first[0] + rest[0], first[1] + rest[1]), whole["games"])


def check_refusals(backend):
    """No silent fall-back: what the resident loop does not cover raises, naming the flag; the ABI refuses bad set-ups."""
    import pytest

    cfg = tictactoe_cfg()
    weights = _weights(backend, cfg)

    def refused(Game, config, **flags):
        c = copy.copy(config)
        c.device_games, c.device_games_chunk = True, CHUNK
        for k, v in flags.items():
            setattr(c, k, v)
        games.NativeBatchedGame.backend = backend
        w = weights if config is cfg else _weights(backend, c)
        shard = self_play.SelfPlay({"weights": w}, Game, c, 7, num_games=4, _backend=backend)
        with pytest.raises(NotImplementedError, match="device_games"):
            shard.play_rounds(1.0, None, max_rounds=2, min_games=FOREVER)
        shard.close_game()

    refused(games.TicTacToeNative, cfg, device_draws=False)
    refused(games.TicTacToeBatched, cfg, device_draws=True)                                   # no native_handle
    refused(games.TicTacToeNative, configs.tictactoe(num_simulations=8, stacked_observations=2), device_draws=True)
    refused(games.TicTacToeNative, cfg, device_draws=True, native_rounds=False)
    refused(games.TicTacToe, cfg, device_draws=True)                                          # the per-object path
    # the ABI
    lib = backend.lib
    plain = make_shard(backend, games.TicTacToeNative, cfg, weights, 4, 7, False, device_draws=False)
    handle = plain._native_shard(1.0).groups[0].handle
    assert lib.mzx_actor_set_resident(handle, CHUNK, 1 << 30) != 0 and b"device draws" in lib.mzx_last_error()
    out = (ctypes.c_int64 * 8)()
    assert lib.mzx_actor_resident_stats(handle, ctypes.byref(out)) != 0
    plain.close_game()
    drawn = make_shard(backend, games.TicTacToeNative, cfg, weights, 4, 7, False)
    native = drawn._native_shard(1.0)
    handle = native.groups[0].handle
    assert lib.mzx_actor_set_resident(None, CHUNK, 1 << 30) != 0
    assert lib.mzx_actor_set_resident(handle, 0, 1 << 30) != 0 and b"chunk_rounds" in lib.mzx_last_error()
    assert lib.mzx_actor_set_resident(handle, CHUNK, 1000) != 0
    message = lib.mzx_last_error()
    assert b"bytes" in message and b"max_log_bytes = 1000" in message
    # one group resident, the other not: the call is refused
    assert len(native.groups) == 2 and lib.mzx_actor_set_resident(handle, CHUNK, 1 << 30) == 0
    with pytest.raises(_lib.MzxError, match="all or none"):
        drawn.play_rounds(1.0, None, max_rounds=2, min_games=FOREVER)
    drawn.close_game()


def check_continuous_self_play(backend):
    """continuous_self_play on a resident shard: the overlapped hand-off (rounds() on a worker thread, collect(before) on the
    main thread, the same finished queue) delivers the games the in-turn hand-off delivers, in the same order with the same
    priorities -- and the rounds were resident."""
    from mzx import shared_storage
    from test_selfplay_refill import _same

    games.NativeBatchedGame.backend = backend

    def once(overlap):
        cfg = configs.tictactoe(num_simulations=5, training_steps=10, ratio=None, self_play_delay=0)
        cfg.PER, cfg.PER_alpha, cfg.td_steps = True, 0.5, 4
        cfg.self_play_overlap_handoff = overlap
        cfg.device_draws, cfg.device_games, cfg.device_games_chunk = True, True, CHUNK
        weights = _weights(backend, cfg, 4)
        storage = shared_storage.LocalStorage(weights=weights, training_step=0, terminate=False, num_played_games=0,
                                              num_played_steps=0)

        class Buffer:
            def __init__(self):
                self.games = []

            def save_game(self, game_history, shared_storage=None):
                assert game_history.priorities is not None
                self.games.append(game_history)
                if len(self.games) >= 20:
                    storage.set_info("terminate", True)

        buf = Buffer()
        actor = self_play.SelfPlay({"weights": weights}, games.TicTacToeNative, cfg, 1, num_games=6, _backend=backend)
        actor.continuous_self_play(storage, buf)
        assert_was_resident(actor, 6)
        actor.close_game()
        return buf.games

    overlapped, in_turn = once(True), once(False)
    n = min(len(overlapped), len(in_turn))
    assert n >= 20 and len(overlapped) >= len(in_turn)
    for a, b in zip(overlapped[:n], in_turn[:n]):
        _same(a, b, "overlapped hand-off")
        assert numpy.array_equal(a.priorities.view(numpy.int32), b.priorities.view(numpy.int32))
