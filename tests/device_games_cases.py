"""
Shared checks of the device-resident game twin (include/mzx.h mzx_game_device_*, csrc/mzx_games_device.h), run by
tests/test_device_games.py on the serial build and by tests/test_gpu_device_games.py on the product library.

The comparator is the host game object of the same library (mzx_game_*), which tests/test_native_games.py holds to the
Python classes: for the same actions the twin must give the same reward and done, the same observation BITS, the same legal
row and side to move at every step, leave masked-out games untouched where the host object does, and download into a host
object that then continues exactly as the comparator does.  No tolerance anywhere: the observation is an exact binary64
scaling rounded once to binary32 (synthetic) or holds -1 / 0 / 1 (boards); rewards are small integers in binary64.

B = 130 is no multiple of the wavefronts per workgroup (a partial last workgroup) and more than one workgroup; gomoku's
121 actions take two passes of the legal-row compaction, synthetic (1, 1, 130) with 70 actions is wider than a wavefront
in both the legal row and the observation (130 elements: no multiple of 64).
"""
import ctypes

import numpy

from mzx import games

B = 130
MOVES = 200

# name -> (factory of a game class, is a board game)
KINDS = {
    "tictactoe": (lambda: games.TicTacToeNative, True),
    "connect4": (lambda: games.Connect4Native, True),
    "gomoku": (lambda: games.GomokuNative, True),
    "synthetic_2x1x3_A3_p2": (lambda: games.make_native_synthetic_game((2, 1, 3), 3, 2), False),
    "synthetic_1x1x130_A70": (lambda: games.make_native_synthetic_game((1, 1, 130), 70, 1), False),
}


def _seeds():
    return [0, 1, 2, 7919, 2 ** 32 - 1, 12345678, 4000000000] + list(range(100, 100 + B - 7))


def host_position(game):
    """(observation float32 bits, legal rows, to_play) of a host game object, straight from the C entry points."""
    obs = numpy.empty((game.num_games,) + tuple(game.shape), numpy.float32)
    game.lib.check(game.lib.mzx_game_observe(game.native_handle, obs.ctypes.data))
    return obs.view(numpy.uint32), game.legal_actions(), numpy.asarray(game.to_play(), numpy.int64)


def device_position(state):
    obs, legal, to_play = state.position()
    return obs.cpu().numpy().view(numpy.uint32), legal.cpu().numpy(), to_play.cpu().numpy().astype(numpy.int64)


def assert_same_position(state, host, where):
    o1, l1, t1 = device_position(state)
    o2, l2, t2 = host_position(host)
    assert o1.shape == o2.shape and numpy.array_equal(o1, o2), ("observation bits", where)
    assert l1.dtype == numpy.int32 and numpy.array_equal(l1, l2), ("legal rows", where)
    assert numpy.array_equal(t1, t2), ("to_play", where)
    return o1, l2


def _random_legal(legal, rs):
    n = (legal >= 0).sum(1)
    assert (n > 0).all()
    return legal[numpy.arange(legal.shape[0]), rs.randint(0, 1 << 30, size=legal.shape[0]) % n].astype(numpy.int64)


def check_twin_equals_host(backend, name):
    make, board = KINDS[name]
    games.NativeBatchedGame.backend = backend
    cls = make()
    host, mirror = cls(_seeds()), cls(_seeds())
    rs = numpy.random.RandomState(17)
    host.reset(), mirror.reset()
    for _ in range(3):          # the twin starts from a position in the middle of the games, not from the first one
        a = _random_legal(host.legal_actions(), rs)
        host.step(a), mirror.step(a)
    state = mirror.device_state()
    finished = masked_rounds = 0
    for move in range(MOVES):
        before, legal = assert_same_position(state, host, move)
        actions = _random_legal(legal, rs)
        active = None
        if move % 3 == 2:       # every third move through the active mask
            active = (rs.randint(0, 4, size=B) > 0).astype(numpy.uint8)
            masked_rounds += 1
        _, r2, d2 = host.step(actions, active)
        r1, d1 = state.step(actions, active)
        r1, d1 = r1.cpu().numpy(), d1.cpu().numpy()
        assert r1.dtype == numpy.float64 and numpy.array_equal(r1.view(numpy.uint64), numpy.asarray(r2, numpy.float64).view(numpy.uint64)), move
        assert numpy.array_equal(d1.astype(bool), numpy.asarray(d2, bool)), move
        if active is not None and board:
            # untouched games stay untouched: same observation bits as before the move, reward 0, not done
            idle = active == 0
            after, _ = assert_same_position(state, host, (move, "after a masked move"))
            assert numpy.array_equal(after[idle], before[idle]) and not r1[idle].any() and not d1[idle].any(), move
            assert (after[~idle].reshape(int((~idle).sum()), -1) != before[~idle].reshape(int((~idle).sum()), -1)).any(1).all(), move
        over = numpy.nonzero(numpy.asarray(d2, bool))[0]
        if move % 11 == 10:     # restarts of games in progress too (the synthetic game never ends by itself)
            over = numpy.union1d(over, rs.choice(B, size=B // 7, replace=False))
        if over.size:
            finished += int(over.size)
            host.reset_games(over)
            state.reset(over.astype(numpy.int32))
    assert masked_rounds > 60
    if board:
        assert finished >= B    # wins, full boards and restarts: every slot ended at least once on average
    assert_same_position(state, host, "end")
    # download: the host object the twin came from is the comparator's equal again -- and continues as it does
    # (step counters and keys included, which no position shows)
    state.download()
    for extra in range(3):
        o1, l1, t1 = host_position(mirror)
        o2, l2, t2 = host_position(host)
        assert numpy.array_equal(o1, o2) and numpy.array_equal(l1, l2) and numpy.array_equal(t1, t2), extra
        a = _random_legal(l2, rs)
        _, ra, da = mirror.step(a)
        _, rb, db = host.step(a)
        assert numpy.array_equal(ra, rb) and numpy.array_equal(da, db), extra
        over = numpy.nonzero(numpy.asarray(db, bool))[0]
        if over.size:
            mirror.reset_games(over), host.reset_games(over)
    # the device state did not move with the host object; reset(None) restarts every game
    state.reset()
    host.reset()
    assert_same_position(state, host, "reset of every game")
    state.close(), host.close(), mirror.close()


def check_out_of_range_inputs_touch_nothing(backend):
    """An action outside the action space and a reset index outside the shard reach no memory and change no game."""
    games.NativeBatchedGame.backend = backend
    host = games.Connect4Native(list(range(9)))
    host.reset()
    state = host.device_state()
    actions = numpy.array([3, 7, -1, 2, 1 << 40, 0, 6, -(1 << 40), 5], numpy.int64)
    valid = (actions >= 0) & (actions < 7)
    before, _ = assert_same_position(state, host, "start")
    reward, done = state.step(actions)
    assert not reward.cpu().numpy().any() and not done.cpu().numpy().any()
    host.step(numpy.where(valid, actions, 0), valid.astype(numpy.uint8))
    after, _ = assert_same_position(state, host, "after the move")
    assert numpy.array_equal(after[~valid], before[~valid])
    state.reset(numpy.array([-1, 9, 1 << 30, 4], numpy.int32))
    host.reset_games([4])
    assert_same_position(state, host, "after the reset")
    state.close(), host.close()


def check_refusals(backend):
    lib = backend.lib
    games.NativeBatchedGame.backend = backend
    small, large, other = games.TicTacToeNative([0, 1]), games.TicTacToeNative([0, 1, 2]), games.Connect4Native([0, 1])
    h = ctypes.c_void_p()
    assert lib.mzx_game_device_create(None, ctypes.byref(h)) != 0
    assert lib.mzx_game_device_create(small.native_handle, None) != 0
    state = small.device_state()
    stream = backend.stream()
    assert lib.mzx_game_device_step(state.handle, None, None, None, None, stream) != 0
    assert lib.mzx_game_device_step(None, None, None, None, None, stream) != 0
    assert lib.mzx_game_device_position(None, None, None, None, stream) != 0
    assert lib.mzx_game_device_position(state.handle, None, None, None, stream) == 0       # nothing asked for
    assert lib.mzx_game_device_reset(state.handle, None, -1, stream) != 0
    assert lib.mzx_game_device_download(state.handle, None, stream) != 0
    for wrong in (large, other):    # another size, another kind
        assert lib.mzx_game_device_download(state.handle, wrong.native_handle, stream) != 0
        assert b"kind and size" in lib.mzx_last_error()
    assert lib.mzx_game_device_download(state.handle, small.native_handle, stream) == 0
    lib.mzx_game_device_destroy(None)
    state.close()
    for g in (small, large, other):
        g.close()
