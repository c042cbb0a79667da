"""
Reanalyse with fresh searches over the device-resident replay store: mzx_replay_search_inputs / mzx_replay_search_write
(csrc/mzx_replay.h), DeviceGameStore.reanalyse_search / download_targets, ReplayBuffer.sync_targets and
Reanalyse.reanalyse_store(search=True) (mzx/replay.py).  Here on the serial build of the same wave bodies (tests/hostcheck);
tests/test_gpu_reanalyse_search.py runs the check functions of this file on the device library.

Everything is compared bit for bit.  The two kernels against numpy restatements written here (the legal rows from the mask
bits, the tape from the Philox generator of tests/replay_sampler_cases.py, the quotients as numpy's int / int true
division).  The sweep against direct searches: every chunk's inputs are rebuilt on the host (store.stacked, the restated
legal rows and tape words, to_play of the histories) and searched with BatchedMCTS._launch at the same tree count --
mzx_search_run is deterministic for identical inputs at an identical tree count, and its agreement with the oracle is what
the parity suites hold, so it is not repeated here.

The weights are synthetic.fill_state_dict's (untied), chosen so that no search exhausts its tie-break tape: skipped == 0.
"""
import copy

import numpy
import pytest
import torch

import hostcheck
from mzx import configs, games, models, replay, self_play, synthetic
from mzx.search import TAPE_WORDS
from replay_sampler_cases import philox
from test_device_replay import CHECKPOINT
from test_reanalyse_sweep import SamplingStock, bits, history

LENGTHS = [0, 1, 3, 7, 12]
SEED = 0x9E3779B97F4A7C15          # both halves of the key are exercised
KEY = 0x52454153


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


def search_config(kind, **overrides):
    fields = dict(td_steps=4, num_unroll_steps=5, PER=True, PER_alpha=0.5, batch_size=16, replay_buffer_size=10 ** 6,
                  stacked_observations=2, seed=SEED & 0xFFFFFFFF)      # (numpy.random.seed takes 32 bits)
    fields.update(overrides)
    if kind == "fc":
        return configs.cartpole(**fields)
    if kind == "connect4":
        return configs.connect4(**fields)
    return configs.tictactoe(discount=0.997, **fields)


# ---------------------------------------------------------------------------------------------------- restatements

def mask_of(legal_lists, A):
    """uint32 [len][ceil(A / 32)]: bit a of a row set when action a is in the row's list."""
    rows = numpy.zeros((len(legal_lists), -(-A // 32)), numpy.uint32)
    for t, acts in enumerate(legal_lists):
        for a in acts:
            rows[t, a >> 5] |= numpy.uint32(1 << (a & 31))
    return rows


def restate_legal(mask_rows, n, A):
    """(legal [n][A] i32, flags [n] i32) of include/mzx.h: the set bits in increasing action order padded with -1; the
    identity without a mask, and -- flagged -- for a row without a bit."""
    legal, flags = numpy.full((n, A), -1, numpy.int32), numpy.zeros(n, numpy.int32)
    for i in range(n):
        acts = list(range(A)) if mask_rows is None else [a for a in range(A) if (int(mask_rows[i, a >> 5]) >> (a & 31)) & 1]
        if not acts:
            acts, flags[i] = list(range(A)), 1
        legal[i, :len(acts)] = acts
    return legal, flags


def restate_tape(seed, sweep, first, n, tape_words):
    tape = numpy.zeros((n, 4 * -(-tape_words // 4)), numpy.uint32)
    counter = numpy.zeros((n, 4), numpy.uint64)
    counter[:, 0] = first + numpy.arange(n)
    counter[:, 1], counter[:, 2] = sweep & 0xFFFFFFFF, sweep >> 32
    for b in range(tape.shape[1] // 4):
        counter[:, 3] = b
        tape[:, 4 * b:4 * b + 4] = philox(counter, (seed & 0xFFFFFFFF, (seed >> 32) ^ KEY))
    return numpy.ascontiguousarray(tape[:, :tape_words])


def flat_positions(store, ids):
    """[(game_id, position)] of the sweep's flat sequence."""
    return [(g, i) for g in ids for i in range(store.games[g][1])]


def sample_list(backend, store, flat):
    rows = numpy.array([store.games[g][0] for g, _ in flat], dtype=numpy.int64)
    pos = numpy.array([i for _, i in flat], dtype=numpy.int32)
    up = lambda a: torch.from_numpy(a).to(backend.device)
    return rows, pos, up(rows), up(pos)


# ---------------------------------------------------------------------------------------------------- stores

def with_legal(gh, A, seed, empty_at=None):
    """Random non-empty legal lists (increasing) for every position of a synthetic history; ``empty_at``: one empty list."""
    rs = numpy.random.RandomState(seed)
    gh.legal_actions = []
    for t in range(len(gh.root_values)):
        keep = numpy.nonzero(rs.randint(0, 2, size=A))[0].tolist() or [int(rs.randint(0, A))]
        gh.legal_actions.append([] if t == empty_at else keep)
    return gh


def synthetic_store(backend, cfg, masks, empty_row=False):
    """The five games of LENGTHS in a store (allocation order = LENGTHS order); returns (buffer, store)."""
    A = len(cfg.action_space)
    hist = [history(cfg, T, 700 + i) for i, T in enumerate(LENGTHS)]
    if masks:
        hist = [with_legal(g, A, 40 + i, empty_at=4 if empty_row and i == 3 else None) for i, g in enumerate(hist)]
    store = replay.DeviceGameStore(cfg, backend, sum(LENGTHS) + len(LENGTHS) + 3, legal_masks=masks)
    buffer = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=SamplingStock, device_store=store)
    for g in hist:
        buffer.save_game(g)
    assert [T for _, T in store.games.values()] == LENGTHS
    return buffer, store


def played(cfg, Game, seed, limit):
    """A game of mzx.games played with random legal moves for at most ``limit`` positions: its history, with the legal
    actions of every position and made-up search statistics."""
    rs = numpy.random.RandomState(seed)
    A = len(cfg.action_space)
    game, gh = Game(), self_play.GameHistory()
    gh.observation_history.append(game.reset())
    gh.action_history.append(0)
    gh.reward_history.append(0)
    gh.to_play_history.append(game.to_play())
    gh.legal_actions = []
    done = False
    while not done and len(gh.root_values) < limit:
        legal = game.legal_actions()
        gh.legal_actions.append(list(legal))
        visits = rs.randint(1, 20, size=len(legal))
        row = [0] * A
        for a, v in zip(legal, visits):
            row[a] = int(v) / int(visits.sum())
        gh.child_visits.append(row)
        gh.root_values.append(float(rs.standard_normal()))
        action = int(legal[int(rs.randint(0, len(legal)))])
        observation, reward, done = game.step(action)
        gh.action_history.append(action)
        gh.observation_history.append(observation)
        gh.reward_history.append(reward)
        gh.to_play_history.append(game.to_play())
    return gh


def played_store(backend, cfg, Game, limits, seed):
    hist = [played(cfg, Game, seed + i, limit) for i, limit in enumerate(limits)]
    rows = sum(len(g.root_values) + 1 for g in hist)
    store = replay.DeviceGameStore(cfg, backend, rows + 2, legal_masks=True)
    buffer = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=SamplingStock, device_store=store)
    for g in hist:
        buffer.save_game(g)
    return buffer, store


def engine_for(backend, cfg, trees, simulations, weights_seed=3):
    model = models.MuZeroNetwork(cfg, _backend=backend)
    model.set_weights(synthetic.fill_state_dict(model.state_dict(), weights_seed))
    return self_play.BatchedMCTS(cfg, model, trees, num_simulations=simulations)


# ---------------------------------------------------------------------------------------------------- 1. inputs kernel

INPUT_CASES = [("resnet", 9, True), ("fc", 2, False), ("fc", 70, True)]
WINDOWS = [(0, sum(LENGTHS)), (2, 7), (6, 14), (sum(LENGTHS) - 5, 5), (0, 0)]      # mid-game starts and ends


def check_inputs(backend, kind, A, masks):
    cfg = search_config(kind, action_space=list(range(A)))
    buffer, store = synthetic_store(backend, cfg, masks, empty_row=masks)
    lib = backend.lib
    flat = flat_positions(store, list(store.games))
    base, pos, d_base, d_pos = sample_list(backend, store, flat)
    to_play_column = store.to_play.cpu().numpy()
    mask_column = store.legal_mask.cpu().numpy().view(numpy.uint32) if masks else None
    if masks:
        assert store.mask_words == -(-A // 32)
        for g, gh in buffer.buffer.items():                       # the ingest: the histories' lists, all-ones padding
            b, T = store.games[g]
            assert numpy.array_equal(mask_column[b:b + T], mask_of(gh.legal_actions, A))
            assert (mask_column[b + T] == 0xFFFFFFFF).all()
        assert any(not row.any() for row in mask_column[base + pos])      # the all-zero row is among the samples
    sweep = (7 << 32) | 5
    for tape_words in (16, 6):
        for lo, n in WINDOWS:
            m = max(n, 1)
            out = dict(to_play=backend.zeros((m,), torch.int32), legal=backend.zeros((m, A), torch.int32),
                       tape=backend.zeros((m, tape_words), torch.int32), flags=backend.zeros((m,), torch.int32))
            lib.check(lib.mzx_replay_search_inputs(store.pool, backend.ptr(store.legal_mask), backend.ptr(d_base[lo:]),
                                                   backend.ptr(d_pos[lo:]), n, tape_words, SEED, sweep, lo, backend.ptr(out["to_play"]),
                                                   backend.ptr(out["legal"]), backend.ptr(out["tape"]), backend.ptr(out["flags"]),
                                                   backend.stream()))
            got = {k: v.cpu().numpy()[:n] for k, v in out.items()}
            rows = (base + pos)[lo:lo + n]
            legal, flags = restate_legal(None if mask_column is None else mask_column[rows], n, A)
            assert numpy.array_equal(got["to_play"], to_play_column[rows]), (kind, A, lo, n)
            assert numpy.array_equal(got["legal"], legal), (kind, A, lo, n)
            assert numpy.array_equal(got["flags"], flags), (kind, A, lo, n)
            assert numpy.array_equal(got["tape"].view(numpy.uint32), restate_tape(SEED, sweep, lo, n, tape_words)), (kind, A, lo, n)
            if masks and n == len(flat):
                assert flags.sum() == 1
    # the tape is apart from the sampler's stream (another key) and moves with the sweep counter and the seed
    t0 = restate_tape(SEED, 0, 0, 4, 8)
    assert not numpy.array_equal(t0, restate_tape(SEED, 1, 0, 4, 8)) and not numpy.array_equal(t0, restate_tape(SEED + 1, 0, 0, 4, 8))


@pytest.mark.parametrize("kind,A,masks", INPUT_CASES)
def test_search_inputs_bit_for_bit(backend, kind, A, masks):
    check_inputs(backend, kind, A, masks)


# ---------------------------------------------------------------------------------------------------- 2. write kernel

def check_write(backend, A):
    cfg = search_config("fc", action_space=list(range(A)))
    buffer, store = synthetic_store(backend, cfg, False)
    lib = backend.lib
    rs = numpy.random.RandomState(A)
    store.child_visits.copy_(torch.from_numpy(rs.standard_normal((store.rows, A)) - 9.0))      # sentinels
    store.root_values.copy_(torch.from_numpy(rs.standard_normal(store.rows) + 55.0))
    before = (store.child_visits.cpu().numpy().copy(), store.root_values.cpu().numpy().copy())
    others = {name: getattr(store, name).cpu().numpy().copy() for name in ("frames", "actions", "rewards", "to_play", "values")}
    flat = flat_positions(store, [1, 3, 4])                  # game 2 (and the empty game 0) stay out
    base, pos, d_base, d_pos = sample_list(backend, store, flat)
    n = len(flat)
    visits = rs.randint(0, 30, size=(n, A)).astype(numpy.int32)
    visits[:, 0] += (visits.sum(1) == 0)
    info = rs.randint(0, 50, size=(n, 4)).astype(numpy.int32)
    info[:, 1] = 0
    flags = numpy.zeros(n, numpy.int32)
    info[2, 1], info[9, 1], flags[5], flags[15] = 1, 2, 1, 1
    visits[12] = 0
    skipped = (info[:, 1] != 0) | (flags != 0) | (visits.sum(1) == 0)
    assert skipped.sum() == 5 and (visits.sum(1)[~skipped] >= 1).all()
    root_value = rs.standard_normal(n)
    up = lambda a: torch.from_numpy(a).to(backend.device)
    d = [up(visits), up(root_value), up(info), up(flags)]
    counter = backend.zeros((1,), torch.int32)
    lib.check(lib.mzx_replay_search_write(*(backend.ptr(t) for t in d), n, A, backend.ptr(d_base), backend.ptr(d_pos),
                                          backend.ptr(store.child_visits), backend.ptr(store.root_values), backend.ptr(counter),
                                          backend.stream()))
    got_visits, got_roots = store.child_visits.cpu().numpy(), store.root_values.cpu().numpy()
    rows = base + pos
    assert numpy.unique(rows).size == n
    want = visits[~skipped] / visits[~skipped].sum(1, keepdims=True)          # int / int true division in binary64
    assert want.dtype == numpy.float64
    assert numpy.array_equal(bits(got_visits[rows[~skipped]]), bits(want))
    assert numpy.array_equal(bits(got_roots[rows[~skipped]]), bits(root_value[~skipped]))
    untouched = numpy.ones(store.rows, bool)
    untouched[rows[~skipped]] = False                          # skipped samples, padding rows, the other games
    assert numpy.array_equal(bits(got_visits[untouched]), bits(before[0][untouched]))
    assert numpy.array_equal(bits(got_roots[untouched]), bits(before[1][untouched]))
    for b, T in store.games.values():
        assert untouched[b + T]
    assert int(counter.cpu().numpy()[0]) == int(skipped.sum())
    for name, column in others.items():
        assert numpy.array_equal(getattr(store, name).cpu().numpy(), column), name


@pytest.mark.parametrize("A", [9, 70])
def test_search_write_bit_for_bit(backend, A):
    check_write(backend, A)


# ---------------------------------------------------------------------------------------------------- 3. refusals

def check_refusals(backend):
    cfg = search_config("resnet")
    buffer, store = synthetic_store(backend, cfg, True)
    lib, ptr, A = backend.lib, backend.ptr, store.A
    flat = flat_positions(store, list(store.games))
    _, _, d_base, d_pos = sample_list(backend, store, flat)
    n = 4
    z = lambda shape, dtype=torch.int32: backend.zeros(shape, dtype)
    keep = [z((n,)), z((n, A)), z((n, 16)), z((n,))]             # (the outputs live as long as the calls)
    inputs = [ptr(d_base), ptr(d_pos), n, 16, SEED, 0, 0] + [ptr(t) for t in keep] + [None]

    def call_inputs(pool=store.pool, mask=store.legal_mask, **change):
        args = list(inputs)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.mzx_replay_search_inputs(pool, ptr(mask), *args)

    assert call_inputs() == 0 and call_inputs(mask=None) == 0
    assert lib.mzx_replay_search_inputs(None, None, *inputs) == -1 and b"mzx_replay_search_inputs" in lib.mzx_last_error()
    for k in (0, 1, 7, 8, 9, 10):                              # every required pointer
        assert call_inputs(**{f"a{k}": None}) == -1 and b"missing" in lib.mzx_last_error(), k
    assert call_inputs(a2=-1) == -1                            # num_samples < 0
    assert call_inputs(a3=0) == -1 and b"tape_words" in lib.mzx_last_error()
    assert call_inputs(a6=-1) == -1 and call_inputs(a6=2 ** 32 - 3) == -1      # the index leaves 32 bits
    assert call_inputs(a6=2 ** 32 - 4) == 0
    small = type(store.pool).from_buffer_copy(store.pool)
    small.action_space_size = 0
    assert call_inputs(pool=small) == -1 and b"action_space_size" in lib.mzx_last_error()
    small = type(store.pool).from_buffer_copy(store.pool)
    small.d_to_play = None
    assert call_inputs(pool=small) == -1
    assert call_inputs(a2=0) == 0

    keep += [z((n, A)), z((n,), torch.float64), z((n, 4)), z((n,)), z((1,))]
    write = [ptr(t) for t in keep[4:8]] + [n, A, ptr(d_base), ptr(d_pos), ptr(store.child_visits), ptr(store.root_values),
                                            ptr(keep[8]), None]
    before = (store.child_visits.cpu().numpy().copy(), store.root_values.cpu().numpy().copy())

    def call_write(**change):
        args = list(write)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.mzx_replay_search_write(*args)

    for k in (0, 1, 2, 3, 6, 7, 8, 9, 10):
        assert call_write(**{f"a{k}": None}) == -1 and b"missing" in lib.mzx_last_error(), k
    assert call_write(a4=-1) == -1 and call_write(a5=0) == -1 and b"mzx_replay_search_write" in lib.mzx_last_error()
    assert call_write(a4=0) == 0
    assert numpy.array_equal(store.child_visits.cpu().numpy(), before[0]) and numpy.array_equal(store.root_values.cpu().numpy(), before[1])


def test_refusals_before_any_launch(backend):
    check_refusals(backend)


# ---------------------------------------------------------------------------------------------------- 4. the sweep

def direct_targets(backend, buffer, store, engine, ids, chunk, sweep, tape_words=TAPE_WORDS):
    """The targets of a sweep from direct searches: per chunk the inputs rebuilt on the host and BatchedMCTS._launch at the
    chunk's tree count.  Returns {game_id: (child_visits [T][A], root_values [T])} and the number of flagged searches."""
    A = store.A
    flat = flat_positions(store, ids)
    stacked = {g: store.stacked(g) for g in ids if store.games[g][1]}
    mask_column = None if store.legal_mask is None else store.legal_mask.cpu().numpy().view(numpy.uint32)
    out = {g: (numpy.zeros((store.games[g][1], A)), numpy.zeros(store.games[g][1])) for g in ids}
    flagged = 0
    for lo in range(0, len(flat), chunk):
        part = flat[lo:lo + chunk]
        n = len(part)
        obs = torch.stack([stacked[g][i] for g, i in part]).reshape(n, -1).contiguous()
        rows = numpy.array([store.games[g][0] + i for g, i in part])
        legal, flags = restate_legal(None if mask_column is None else mask_column[rows], n, A)
        assert not flags.any()
        to_play = numpy.array([buffer.buffer[g].to_play_history[i] for g, i in part], dtype=numpy.int32)
        tape = restate_tape(store.config.seed, sweep, lo, n, tape_words)
        visits, root_values, _, info = engine._launch(n, obs, legal, to_play, None, tape, tape_words, None)
        flagged += int((info[:, 1] != 0).sum())
        assert (visits.sum(1) == engine.num_simulations).all()
        for k, (g, i) in enumerate(part):
            out[g][0][i] = visits[k] / visits[k].sum()
            out[g][1][i] = root_values[k]
    return out, flagged


def pool_targets(store):
    return {g: (v.copy(), r.copy()) for g, (v, r) in store.download_targets().items()}


def sweep_case(backend, kind):
    if kind == "fc":
        cfg = search_config("fc")
        buffer, store = synthetic_store(backend, cfg, False)
        return cfg, buffer, store, engine_for(backend, cfg, 4, 10), 4
    cfg = search_config("resnet")
    buffer, store = played_store(backend, cfg, games.TicTacToe, [9, 9, 0, 9, 4, 9], 60)
    return cfg, buffer, store, engine_for(backend, cfg, 8, 8), 5


def check_sweep(backend, cfg, buffer, store, engine, chunk):
    ids = list(store.games)
    total = sum(T for _, T in store.games.values())
    assert total % chunk and any(T % chunk for _, T in store.games.values())      # chunks straddle games, the last is partial
    before = {name: getattr(store, name).cpu().numpy().copy() for name in ("frames", "actions", "rewards", "to_play")}
    assert store.search_sweep_counter == 0
    report = store.reanalyse_search(engine, chunk_positions=chunk)
    assert report == {"positions": total, "skipped": 0, "chunks": -(-total // chunk)}, report
    assert store.search_sweep_counter == 1
    got = pool_targets(store)
    want, flagged = direct_targets(backend, buffer, store, engine, ids, chunk, 0)
    assert flagged == 0
    values = store.values.cpu().numpy()
    for g in ids:
        b, T = store.games[g]
        assert got[g][0].shape == (T, store.A) and got[g][1].shape == (T,)
        assert numpy.array_equal(bits(got[g][0]), bits(want[g][0])), g
        assert numpy.array_equal(bits(got[g][1]), bits(want[g][1])), g
        updated = copy.copy(buffer.buffer[g])
        updated.root_values, updated.reanalysed_predicted_root_values = want[g][1].tolist(), None
        assert numpy.array_equal(bits(values[b:b + T]), bits(replay.n_step_values(updated, cfg))), g
        if store.legal_mask is not None:      # an illegal action is no child: its target is 0
            for t, acts in enumerate(buffer.buffer[g].legal_actions):
                assert not got[g][0][t, [a for a in range(store.A) if a not in acts]].any()
    for name, column in before.items():
        assert numpy.array_equal(getattr(store, name).cpu().numpy(), column), name
    # the same counter again: the same bits
    store.search_sweep_counter = 0
    assert store.reanalyse_search(engine, chunk_positions=chunk)["skipped"] == 0
    again = pool_targets(store)
    for g in ids:
        assert numpy.array_equal(bits(again[g][0]), bits(got[g][0])) and numpy.array_equal(bits(again[g][1]), bits(got[g][1]))
    # the next counter: other tie-break words, the same shapes, distributions still
    assert store.search_sweep_counter == 1
    assert store.reanalyse_search(engine, chunk_positions=chunk)["skipped"] == 0 and store.search_sweep_counter == 2
    other = pool_targets(store)
    for g in ids:
        assert other[g][0].shape == got[g][0].shape and other[g][1].shape == got[g][1].shape
        # A quotients, each within half an ulp of 1: their sum is within A * 2^-53 of 1 before its own roundings
        assert numpy.allclose(other[g][0].sum(1), 1.0, rtol=0, atol=store.A * 2.0 ** -52)
        assert numpy.allclose(got[g][0].sum(1), 1.0, rtol=0, atol=store.A * 2.0 ** -52)
    return report


@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_sweep_equals_direct_searches(backend, kind):
    cfg, buffer, store, engine, chunk = sweep_case(backend, kind)
    check_sweep(backend, cfg, buffer, store, engine, chunk)


def check_selection_and_errors(backend):
    cfg = search_config("fc")
    buffer, store = synthetic_store(backend, cfg, False)
    engine = engine_for(backend, cfg, 4, 10)
    assert store.reanalyse_search(engine, []) == {"positions": 0, "skipped": 0, "chunks": 0}
    assert store.reanalyse_search(engine, [0]) == {"positions": 0, "skipped": 0, "chunks": 0}        # the game of T == 0
    with pytest.raises(KeyError):
        store.reanalyse_search(engine, [1, 99])
    with pytest.raises(ValueError):
        store.reanalyse_search(engine, chunk_positions=0)
    with pytest.raises(ValueError):                     # another action space
        store.reanalyse_search(engine_for(backend, search_config("fc", action_space=list(range(3))), 4, 10))
    with pytest.raises(ValueError):                     # another observation size
        store.reanalyse_search(engine_for(backend, search_config("fc", stacked_observations=0), 4, 10))
    assert store.search_sweep_counter == 0             # an empty or refused call consumes no counter value
    before = pool_targets(store)
    priorities = [gh.priorities.copy() for gh in buffer.buffer.values() if gh.priorities is not None]
    report = store.reanalyse_search(engine, [4, 2, 4], chunk_positions=1000, seed=12)      # chunk: capped by max_trees
    assert report == {"positions": 15, "skipped": 0, "chunks": 4}
    after = pool_targets(store)
    for g in store.games:
        same = numpy.array_equal(bits(after[g][0]), bits(before[g][0])) and numpy.array_equal(bits(after[g][1]), bits(before[g][1]))
        assert same == (g not in (4, 2) or store.games[g][1] == 0), g
    assert all(numpy.array_equal(p, gh.priorities) for p, gh in zip(priorities, [h for h in buffer.buffer.values() if h.priorities is not None]))
    assert store.search_sweep_counter == 1
    with pytest.raises(KeyError):
        store.download_targets([99])
    assert list(store.download_targets([3, 1])) == [3, 1]


def test_selection_and_errors(backend):
    check_selection_and_errors(backend)


# ---------------------------------------------------------------------------------------------------- 5. downstream

def check_downstream(backend, kind):
    cfg, buffer, store, engine, chunk = sweep_case(backend, kind)
    assert store.reanalyse_search(engine, chunk_positions=chunk)["skipped"] == 0
    visits = store.child_visits.cpu().numpy()
    U, A = cfg.num_unroll_steps, store.A
    for r in range(3):
        numpy.random.seed(70 + r)
        index_batch, tensors = buffer.get_batch()
        policy = tensors[4].cpu().numpy()
        assert policy.shape == (cfg.batch_size, U + 1, A)
        for i, (g, p) in enumerate(index_batch):
            b, T = store.games[g]
            for u in range(U + 1):
                want = visits[b + p + u] if p + u < T else numpy.full(A, 1 / A)
                assert numpy.array_equal(bits(policy[i, u]), bits(want)), (g, p, u)
    # the host histories take the device targets; a store built from them holds the same columns
    stale = {g: (copy.copy(gh.child_visits), copy.copy(gh.root_values)) for g, gh in buffer.buffer.items()}
    buffer.sync_targets()
    fresh = replay.DeviceGameStore(cfg, backend, store.rows, legal_masks=store.legal_mask is not None)
    fresh.add_many(list(buffer.buffer.items()))
    assert fresh.games == store.games
    for g, gh in buffer.buffer.items():
        T = len(gh.root_values)
        assert isinstance(gh.child_visits, list) and isinstance(gh.root_values, list) and gh.reanalysed_predicted_root_values is None
        assert all(isinstance(row, list) and len(row) == A for row in gh.child_visits) and all(isinstance(v, float) for v in gh.root_values)
        if T:
            assert gh.root_values != stale[g][1] and gh.child_visits != stale[g][0]
    for name in ("child_visits", "root_values", "values"):
        a, b = getattr(store, name).cpu().numpy(), getattr(fresh, name).cpu().numpy()
        for base, T in store.games.values():
            assert numpy.array_equal(bits(a[base:base + T]), bits(b[base:base + T])), name
    # a history whose length no longer matches the store's copy: refused before anything is written
    odd = next(g for g, gh in buffer.buffer.items() if len(gh.root_values) > 1)
    kept = buffer.buffer[odd].root_values
    buffer.buffer[odd].root_values = kept[:-1]
    first = next(iter(buffer.buffer))
    buffer.buffer[first].reanalysed_predicted_root_values = "untouched"
    with pytest.raises(ValueError):
        buffer.sync_targets()
    assert buffer.buffer[first].reanalysed_predicted_root_values == "untouched"
    buffer.buffer[odd].root_values, buffer.buffer[first].reanalysed_predicted_root_values = kept, None
    # the host-side batch of the synchronised histories: the same targets as the device's
    plain = replay.ReplayBuffer({"num_played_games": buffer.num_played_games, "num_played_steps": buffer.num_played_steps},
                                dict(buffer.buffer), cfg, stock=SamplingStock)
    numpy.random.seed(91)
    want = plain.get_batch()
    numpy.random.seed(91)
    got = buffer.get_batch()
    assert got[0] == want[0]
    assert numpy.array_equal(bits(got[1][4].cpu().numpy()), bits(numpy.asarray(want[1][4], dtype=numpy.float64)))
    assert numpy.array_equal(bits(got[1][2].cpu().numpy()), bits(numpy.asarray(want[1][2], dtype=numpy.float64)))


@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_batches_and_sync_after_a_sweep(backend, kind):
    check_downstream(backend, kind)


# ---------------------------------------------------------------------------------------------------- 6. the worker

def check_worker(backend):
    fields = dict(reanalyse_search_trees=4, reanalyse_search_simulations=10)

    def build(**overrides):
        cfg = search_config("fc", **fields, **overrides)
        buffer, store = synthetic_store(backend, cfg, False)
        weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 3)
        worker = replay.Reanalyse({"weights": weights, "num_reanalysed_games": 2}, cfg, _backend=backend, device_store=store)
        return cfg, buffer, store, worker

    cfg, buffer, store, worker = build(reanalyse_search=True)
    buffer._game_arrays(3, buffer.buffer[3])
    assert worker.reanalyse_store(buffer) == len(LENGTHS) and worker.num_reanalysed_games == 2 + len(LENGTHS)
    assert not buffer._arrays and store.search_sweep_counter == 1
    built = worker._search_engine
    assert built.max_trees == 4 and built.num_simulations == 10
    cfg2, buffer2, store2, _ = build()
    report = store2.reanalyse_search(engine_for(backend, cfg2, 4, 10))
    assert report["skipped"] == 0 and report["chunks"] == -(-sum(LENGTHS) // 4)
    for name in ("child_visits", "root_values", "values"):
        assert numpy.array_equal(bits(getattr(store, name).cpu().numpy()), bits(getattr(store2, name).cpu().numpy())), name
    assert worker.reanalyse_store(buffer, [4]) == 1 and worker._search_engine is built      # built once
    with pytest.raises(KeyError):
        worker.reanalyse_store(buffer, [99])
    # the argument wins over the configuration; without either the value sweep runs as before
    cfg3, buffer3, store3, worker3 = build()
    cfg4, buffer4, store4, worker4 = build(reanalyse_search=True)
    visits = store3.child_visits.cpu().numpy().copy()
    want = store2.__class__.reanalyse          # (the existing sweep, on a store of its own)
    cfg5, buffer5, store5, worker5 = build()
    swept = want(store5, worker5.model)
    assert worker3.reanalyse_store(buffer3) == len(LENGTHS) and worker4.reanalyse_store(buffer4, search=False) == len(LENGTHS)
    for s, b in ((store3, buffer3), (store4, buffer4)):
        assert s.search_sweep_counter == 0
        assert numpy.array_equal(bits(s.child_visits.cpu().numpy()), bits(visits))
        for name in ("root_values", "values"):
            assert numpy.array_equal(bits(getattr(s, name).cpu().numpy()), bits(getattr(store5, name).cpu().numpy())), name
        for g, gh in b.buffer.items():
            assert numpy.array_equal(bits(gh.reanalysed_predicted_root_values), bits(swept[g]))
    assert worker3._search_engine is None and worker3.reanalyse_store(buffer3, search=True) == len(LENGTHS)
    assert store3.search_sweep_counter == 1
    assert numpy.array_equal(bits(store3.child_visits.cpu().numpy()), bits(store.child_visits.cpu().numpy()))


def test_worker_searches_the_store(backend):
    check_worker(backend)


# ---------------------------------------------------------------------------------------------------- recording

def test_self_play_records_legal_actions(backend):
    """With config.reanalyse_search a played game carries the legal actions of every position, in the game's (increasing)
    order; the store turns them into its mask rows.  Without the flag the history has no such attribute."""
    for flag in (True, False):
        cfg = search_config("resnet", num_simulations=4, opponent="self", **({"reanalyse_search": True} if flag else {}))
        weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 2)
        actor = self_play.SelfPlay({"weights": weights}, games.TicTacToe, cfg, 5, _backend=backend)
        gh = actor.play_game(1.0, None, False, "self", 0)
        T = len(gh.root_values)
        if not flag:
            assert not hasattr(gh, "legal_actions")
            continue
        assert len(gh.legal_actions) == T and gh.legal_actions[0] == list(range(9))
        taken = []
        for t in range(T):
            assert gh.legal_actions[t] == [a for a in range(9) if a not in taken]
            taken.append(gh.action_history[t + 1])
        store = replay.DeviceGameStore(cfg, backend, T + 1, legal_masks=True)
        store.add(0, gh)
        assert numpy.array_equal(store.legal_mask.cpu().numpy().view(numpy.uint32)[:T], mask_of(gh.legal_actions, 9))


def shard_views(mask):
    from mzx.history import ShardGameHistory, _ShardRecord
    T, A = 3, 4
    rs = numpy.random.RandomState(2)
    obs = rs.standard_normal((2, T + 1, 1, 1, 4)).astype(numpy.float32)
    acts, rews, tps = rs.randint(0, A, size=(2, T + 1)), rs.standard_normal((2, T + 1)), numpy.zeros((2, T + 1), numpy.int32)
    vis = rs.randint(1, 9, size=(2, T, A))
    if mask is not None:
        vis = vis * mask
    totals = vis.sum(2)
    record = _ShardRecord(A, obs, acts, rews, tps, vis, rs.standard_normal((2, T)), totals, vis / totals[:, :, None],
                          numpy.array([mask is None] * 2), mask)
    return ShardGameHistory.make_many(record, 2, T)


def test_shard_views_expose_their_legal_mask(backend):
    """A history that views a shard record (batched and native round loops) offers the record's legal mask as
    ``legal_actions``; a record without a mask -- every action legal throughout -- leaves the attribute absent.  The lists
    survive pickling and copying (a checkpoint of the buffer, an object store), and a restored view enters a store built
    with legal_masks=True with the same mask rows as the live one."""
    import pickle
    mask = numpy.zeros((2, 3, 4), bool)
    mask[0, 0, [0, 3]] = mask[0, 1, [1]] = mask[0, 2, [0, 1, 2, 3]] = True
    mask[1] = True
    want = [[[0, 3], [1], [0, 1, 2, 3]], [[0, 1, 2, 3]] * 3]
    views = shard_views(mask)
    assert [v.legal_actions for v in views] == want
    assert "legal_actions" not in views[0].__dict__            # (a fresh view stays a two-entry object)
    restored = [pickle.loads(pickle.dumps(views[0])), copy.deepcopy(views[1])]
    assert all("_view" not in r.__dict__ for r in restored)
    assert [r.legal_actions for r in restored] == want
    cfg = search_config("fc", action_space=list(range(4)), stacked_observations=0, PER=False)
    rows = []
    for group in (shard_views(mask), restored):
        store = replay.DeviceGameStore(cfg, backend, 8, legal_masks=True)
        store.add_many(list(enumerate(group)))
        rows.append(store.legal_mask.cpu().numpy().view(numpy.uint32).copy())
    assert numpy.array_equal(rows[0], rows[1])
    assert numpy.array_equal(rows[0][:3], mask_of(want[0], 4)) and (rows[0][3] == 0xFFFFFFFF).all()
    # without a mask: no attribute, before and after a round trip (AttributeError, whatever the object still holds)
    plain = shard_views(None)
    assert getattr(plain[0], "legal_actions", None) is None
    assert getattr(pickle.loads(pickle.dumps(plain[0])), "legal_actions", None) is None
