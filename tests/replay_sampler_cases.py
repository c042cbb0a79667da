"""
Device-side prioritised sampling and priority feedback of the replay store (mzx_replay_sample,
mzx_replay_update_priorities, mzx_replay_sampler_refresh; csrc/mzx_replay.h): the numpy oracle of the draw as include/mzx.h
defines it, the Philox4x32-10 restatement behind it, and the check functions.  tests/test_replay_sampler.py runs them on
the serial build (tests/hostcheck), tests/test_gpu_replay_sampler.py on the device library.

Exact comparisons use priorities on a dyadic grid (multiples of 2^-12 below 2^8): every partial sum of up to 1000 of them
is exact in binary64 whatever the association, so the oracle's sequential sums, the serial build's and the device's
tile / chunk scans give the same bits, and with them the same targets, indices and weights.
"""
import copy
import ctypes

import numpy
import torch

from mzx import _lib, replay, trainer
from test_device_replay import CHECKPOINT, StandInStock
from test_reanalyse_sweep import history, sweep_config
import trainer_loss_cases

M32 = numpy.uint64(0xFFFFFFFF)
KAT = [  # Random123 known-answer vectors of philox4x32-10: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 700]      # around the chunk of 256 positions and the four-per-lane layout
SLOT_COUNTS = [1, 63, 64, 65, 256, 257, 1000]      # around the tile of 256 slots
BATCHES = [1, 7, 64, 130]


# ------------------------------------------------------------------------------------------------ the generator

def philox(counter, key):
    """Philox4x32-10 of counters [n, 4] under one key (k0, k1): uint32 [n, 4]."""
    c = [numpy.asarray(counter, dtype=numpy.uint64)[:, j] & M32 for j in range(4)]
    k0, k1 = numpy.uint64(key[0]), numpy.uint64(key[1])
    for _ in range(10):
        p0, p1 = numpy.uint64(0xD2511F53) * c[0], numpy.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> numpy.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> numpy.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + numpy.uint64(0x9E3779B9)) & M32, (k1 + numpy.uint64(0xBB67AE85)) & M32
    return numpy.stack(c, 1).astype(numpy.uint32)


def blocks(seed, call_counter, n, j):
    counter = numpy.zeros((n, 4), numpy.uint64)
    counter[:, 0] = numpy.arange(n)
    counter[:, 1], counter[:, 2], counter[:, 3] = call_counter & 0xFFFFFFFF, call_counter >> 32, j
    return philox(counter, (seed & 0xFFFFFFFF, seed >> 32)).astype(numpy.uint64)


def generator_uniforms(seed, call_counter, n):
    w = blocks(seed, call_counter, n, 0)
    u53 = lambda hi, lo: ((hi << numpy.uint64(21)) | (lo >> numpy.uint64(11))).astype(numpy.float64) * 2.0 ** -53
    return numpy.stack([u53(w[:, 0], w[:, 1]), u53(w[:, 2], w[:, 3])], 1)


def check_known_answers():
    for counter, key, want in KAT:
        assert [int(v) for v in philox([counter], key)[0]] == want


# ------------------------------------------------------------------------------------------------ the oracle

def clean(p):
    """A float32 priority as a binary64 weight: non-finite or non-positive counts as 0."""
    p = numpy.asarray(p, dtype=numpy.float32)
    with numpy.errstate(invalid="ignore"):
        return numpy.where(numpy.isfinite(p) & (p > 0), p, 0).astype(numpy.float64)


def first_above(weights, t):
    """Smallest index whose inclusive prefix exceeds t (strictly) and whose weight is positive; else the last positive."""
    c = numpy.cumsum(weights)
    hit = numpy.nonzero((c > t) & (weights > 0))[0]
    return int(hit[0]) if hit.size else int(numpy.nonzero(weights > 0)[0][-1])


def table_of(store):
    """Host copies of the sampler's state."""
    store._flush_slots()
    h = lambda t: t.cpu().numpy()
    return dict(game=h(store.slot_game), base=h(store.slot_base), len=h(store.slot_len), top=h(store.slot_priority),
                sum=h(store.slot_sum), priorities=h(store.priorities), owner=h(store.owner))


def slot_weights(table, per):
    """The game level's weights in slot order: game_priority with PER, 1 per game with a position otherwise (and when no
    priority is positive anywhere)."""
    live = (table["game"] >= 0) & (table["len"] > 0)
    w = numpy.where(live, clean(table["top"]), 0.0) if per else live.astype(numpy.float64)
    return w if w.sum() > 0 else live.astype(numpy.float64)


def oracle_sample(table, n, seed, call_counter, total_samples, per, U, action_space, uniforms=None, margins=None):
    """The draw of include/mzx.h in numpy: dict(base, len, pos, tape, game_id, weight).  ``margins`` (a list) receives the
    relative distance of every target from the nearest prefix boundary of its level."""
    u = generator_uniforms(seed, call_counter, n) if uniforms is None else numpy.asarray(uniforms, dtype=numpy.float64)
    w = slot_weights(table, per)
    S = numpy.cumsum(w)[-1]
    A = len(action_space)
    out = dict(base=numpy.zeros(n, numpy.int64), len=numpy.zeros(n, numpy.int32), pos=numpy.zeros(n, numpy.int32),
               tape=numpy.zeros((n, U + 1), numpy.int32), game_id=numpy.zeros(n, numpy.int64))
    raw = numpy.zeros(n, numpy.float64)
    words = numpy.concatenate([blocks(seed, call_counter, n, 1 + j) for j in range(U // 4 + 1)], 1)
    for i in range(n):
        t = u[i, 0] * S
        s = first_above(w, t)
        if margins is not None:
            margins.append(numpy.abs(numpy.cumsum(w) - t).min() / S)
        base, T = int(table["base"][s]), int(table["len"][s])
        p = clean(table["priorities"][base:base + T])
        P = numpy.cumsum(p)[-1]
        if per and P > 0:
            tp = u[i, 1] * P
            pos = first_above(p, tp)
            p_i = p[pos]
            if margins is not None:
                margins.append(numpy.abs(numpy.cumsum(p) - tp).min() / P)
        else:
            f = numpy.floor(u[i, 1] * T)
            pos = int(min(T - 1, f)) if f >= 0 else 0
            p_i, P = 1.0, float(T)
        out["base"][i], out["len"][i], out["pos"][i], out["game_id"][i] = base, T, pos, table["game"][s]
        raw[i] = 1.0 / ((numpy.float64(total_samples) * (w[s] / S)) * (p_i / P))
        for step in range(U + 1):
            if step >= T + 1 - pos:
                out["tape"][i, step] = action_space[int((int(words[i, step]) * A) >> 32)]
    out["weight"] = (raw / raw.max()).astype(numpy.float32) if per else None
    return out


def device_sample(store, n, seed, call_counter, total_samples, per, U, uniforms=None):
    base, length, pos, tape, game_id, weight = store.sample(n, seed, call_counter, total_samples, per, U, uniforms)
    h = lambda t: None if t is None else t.cpu().numpy()
    return dict(base=h(base), len=h(length), pos=h(pos), tape=h(tape), game_id=h(game_id), weight=h(weight))


def assert_bits(got, want, tag):
    for k, v in want.items():
        if v is None:
            assert got[k] is None, (tag, k)
        else:
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, (tag, k, got[k].dtype, v.dtype)
            assert numpy.array_equal(got[k].view(numpy.uint8), v.view(numpy.uint8)), (tag, k, got[k], v)


# ------------------------------------------------------------------------------------------------ stores

def sampler_config(per=True, kind="fc", **overrides):
    return sweep_config(kind, PER=per, seed=7, **overrides)


def game(cfg, T, seed, priorities=None):
    gh = history(cfg, T, seed)
    if priorities is not None:
        gh.priorities = numpy.asarray(priorities, dtype=numpy.float32)
        gh.game_priority = numpy.max(gh.priorities) if T else numpy.float32(0)
    return gh


def dyadic(rs, T):
    p = (rs.randint(0, 2 ** 20, size=T).astype(numpy.float64) * 2.0 ** -12).astype(numpy.float32)
    p[rs.random_sample(T) < 0.1] = 0
    return p


_STORES = {}


def dyadic_store(backend, slots, per):
    """A table of ``slots`` slots holding games of dyadic priorities: ids with gaps (empty slots in between), the lengths
    around the chunk size where there is room for them (each with a positive last priority, so that its last chunk can be
    aimed at), and among the short games some of T == 0 and some whose priorities are all 0."""
    key = (id(backend), slots, per)
    if key not in _STORES:
        cfg = sampler_config(per)
        rs = numpy.random.RandomState(slots)
        ids = [g for g in range(slots) if slots < 4 or g % 3 != 1]
        long_games = LENGTHS if slots >= 63 else LENGTHS[:1]
        items = []
        for n, g in enumerate(ids):
            T = long_games[n // 2] if n % 2 == 0 and n // 2 < len(long_games) else int(rs.randint(1, 10))
            short = n >= 2 * len(long_games)
            if short and n % 7 == 3:
                T = 0
            p = dyadic(rs, T)
            if short and n % 5 == 4:
                p[:] = 0
            if not short and n % 2 == 0:
                p[-1] = 0.5
            items.append((g + 5 * slots, game(cfg, T, 1000 * slots + g, p)))      # slot = id % slots = g
        store = replay.DeviceGameStore(cfg, backend, sum(len(gh.root_values) + 1 for _, gh in items) + 3, max_games=slots)
        store.add_many(items)
        _STORES[key] = (cfg, store, dict(items))
    return _STORES[key]


# ------------------------------------------------------------------------------------------------ checks

def check_bit_exact(backend, slots, per):
    cfg, store, games = dyadic_store(backend, slots, per)
    table = table_of(store)
    for g, gh in games.items():      # the state add_many left: priorities, padding row, slot columns
        s, T = g % slots, len(gh.root_values)
        assert table["game"][s] == g and table["len"][s] == T and (table["base"][s], T) == store.games[g]
        rows = table["priorities"][table["base"][s]:table["base"][s] + T + 1]
        want = gh.priorities if per else numpy.zeros(T, numpy.float32)
        assert numpy.array_equal(rows[:T], want) and rows[T] == 0
        assert table["top"][s] == (want.max() if T else 0) and table["sum"][s] == want.astype(numpy.float64).sum()
    assert (table["owner"] == -1).all()
    U, space, total = cfg.num_unroll_steps, list(cfg.action_space), int(table["len"][table["game"] >= 0].sum())
    first = None
    for n in BATCHES:
        want = oracle_sample(table, n, cfg.seed, 3, total, per, U, space)
        got = device_sample(store, n, cfg.seed, 3, total, per, U)
        assert_bits(got, want, (slots, per, n))
        assert_bits(device_sample(store, n, cfg.seed, 3, total, per, U), got, "same counter, same bits")
        live = (table["game"] >= 0) & (table["len"] > 0) & ((table["top"] > 0) | (not per))
        assert set(got["game_id"]) <= set(table["game"][live])
        assert ((got["pos"] >= 0) & (got["pos"] < got["len"])).all()
        if per:
            picked = table["priorities"][got["base"] + got["pos"]]
            assert (picked > 0).all() and got["weight"].max() == 1.0
        first = got
    # every length around the chunk size is resident with weight, and is drawn: samples aimed at each of those games -- at
    # its first position, at the edge and the middle of its last chunk of 256, and at its end
    wanted = LENGTHS if slots >= 63 else LENGTHS[:1]
    w = slot_weights(table, per)
    C, aimed, chunk_start = numpy.cumsum(w), [], []
    for T in wanted:
        s = next(g % slots for g, gh in games.items() if len(gh.root_values) == T and gh.priorities[-1] > 0)
        assert w[s] > 0 and (not per or table["sum"][s] > 0), T
        start = 256 * ((T - 1) // 256)
        p = clean(table["priorities"][table["base"][s]:table["base"][s] + T]) if per else numpy.ones(T)
        before = p[:start].sum()
        for u_pos in (0.0, before / p.sum() * (1 + 2.0 ** -50), (before + (p.sum() - before) / 2) / p.sum(), 1 - 2.0 ** -53):
            aimed.append(((C[s] - w[s] / 2) / C[-1], u_pos))
            chunk_start.append((table["game"][s], T, start if u_pos > 0 or start == 0 else 0))
    aimed = numpy.array(aimed)
    got = device_sample(store, len(aimed), cfg.seed, 5, total, per, U, uniforms=aimed)
    assert_bits(got, oracle_sample(table, len(aimed), cfg.seed, 5, total, per, U, space, uniforms=aimed), "aimed")
    for i, (g, T, start) in enumerate(chunk_start):
        assert got["game_id"][i] == g and got["len"][i] == T and start <= got["pos"][i] < T, (i, g, T, start, got["pos"][i])
        assert i % 4 != 3 or got["pos"][i] == T - 1
    other = device_sample(store, BATCHES[-1], cfg.seed, 4, total, per, U)
    assert_bits(other, oracle_sample(table, BATCHES[-1], cfg.seed, 4, total, per, U, space), "next counter")
    if slots > 1:
        assert not (numpy.array_equal(other["game_id"], first["game_id"]) and numpy.array_equal(other["pos"], first["pos"]))


def check_action_space(backend):
    """A permuted action space goes through d_action_space; short games make most steps absorbing."""
    cfg = sampler_config(True, action_space=[1, 0])
    store = replay.DeviceGameStore(cfg, backend, 40, max_games=8)
    store.add_many([(g, game(cfg, T, g, dyadic(numpy.random.RandomState(g), T) + 1)) for g, T in enumerate([1, 2, 3, 9])])
    table = table_of(store)
    for U in (0, 3, 4, 9):
        want = oracle_sample(table, 33, 11, 2 ** 40 + 5, 15, True, U, [1, 0])
        assert_bits(device_sample(store, 33, 11, 2 ** 40 + 5, 15, True, U), want, U)
        assert U == 0 or want["tape"].any()


def check_boundaries(backend):
    """S and P powers of two: targets land exactly on a prefix boundary, one step below, on 0 and at 1 - 2^-53; the
    strict rule C > t decides; zero-weight entries are never returned."""
    cfg = sampler_config(True)
    # slots: 0 weight 2, 1 zero priority, 2 empty, 3 weight 2, 4 T == 0, 5 weight 4 -> prefix 2 2 2 4 4 8, S = 8
    rows = {0: [2, 0, 1, 1], 1: [0, 0], 3: [0, 2, 0, 0.5, 1.5, 0], 4: [], 5: [4, 1, 0, 2, 1]}
    store = replay.DeviceGameStore(cfg, backend, 40, max_games=6)
    store.add_many([(g, game(cfg, len(p), g, p)) for g, p in rows.items()])
    table = table_of(store)
    eps, top = 2.0 ** -53, 1 - 2.0 ** -53
    cases = [  # (u_game, u_pos) -> (slot, position)
        ((0.0, 0.0), (0, 0)), ((0.25 - eps, 0.5 - eps), (0, 0)), ((0.25, 0.5), (3, 3)),       # P = 4: [2 2 3 4], [0 2 2 2.5 4 4]
        ((0.5 - eps, 0.5 - eps), (3, 1)), ((0.5, 0.5), (5, 1)), ((top, top), (5, 4)),          # P = 8: [4 5 5 7 8]
        ((0.5, 0.5 - eps), (5, 0)), ((0.5, 0.625), (5, 3)), ((0.5, 0.875), (5, 4)), ((0.25, 0.625 - eps), (3, 3)),
        ((0.25, 0.625), (3, 4)), ((0.0, 0.75), (0, 3)), ((0.0, 0.75 - eps), (0, 2)),
    ]
    u = numpy.array([c[0] for c in cases])
    got = device_sample(store, len(cases), 1, 0, 17, True, 2, uniforms=u)
    assert_bits(got, oracle_sample(table, len(cases), 1, 0, 17, True, 2, list(cfg.action_space), uniforms=u), "boundaries")
    assert [(int(g), int(p)) for g, p in zip(got["game_id"], got["pos"])] == [c[1] for c in cases]
    # PER off: three live games (slots 0, 1, 3, 5 have positions: four), positions floor(u * T)
    got = device_sample(store, 4, 1, 0, 17, False, 2, uniforms=numpy.array([[0.0, 0.0], [0.25, 0.5], [0.5 - eps, top], [top, top]]))
    assert [(int(g), int(p)) for g, p in zip(got["game_id"], got["pos"])] == [(0, 0), (1, 1), (1, 1), (5, 4)]
    assert got["weight"] is None


def check_general(backend, seed=2):
    """float32 priorities of fill_initial_priorities on random games: with every target of the oracle further than 2^-30
    (relative) from a prefix boundary -- association error over <= 1000 terms is below 2^-43 --, identical indices and
    weights within one float32 ulp."""
    cfg = sampler_config(True)
    rs = numpy.random.RandomState(seed)
    items = []
    for g in range(300):
        gh = game(cfg, int(rs.randint(1, 400)) if g % 9 == 0 else int(rs.randint(1, 30)), 50 + g)
        assert replay.fill_initial_priorities(gh, cfg)
        items.append((g, gh))
    store = replay.DeviceGameStore(cfg, backend, sum(len(gh.root_values) + 1 for _, gh in items), max_games=300)
    store.add_many(items)
    table, margins = table_of(store), []
    total = sum(len(gh.root_values) for _, gh in items)
    want = oracle_sample(table, 130, cfg.seed, 9, total, True, cfg.num_unroll_steps, list(cfg.action_space), margins=margins)
    assert min(margins) > 2.0 ** -30, "choose another seed: a target of the oracle lies on a prefix boundary"
    got = device_sample(store, 130, cfg.seed, 9, total, True, cfg.num_unroll_steps)
    weights = (got.pop("weight"), want.pop("weight"))
    assert_bits(got, want, "general")
    ulp = numpy.spacing(numpy.maximum(weights[0], weights[1]))
    assert (numpy.abs(weights[0] - weights[1]) <= ulp).all()
    for g, gh in items:
        s = g % 300
        assert table["top"][s] == gh.game_priority
        assert abs(table["sum"][s] - gh.priorities.astype(numpy.float64).sum()) <= 1e-12 * table["sum"][s]


DEGENERATE = ("all zero", "nan", "negative", "single live game")


def check_degenerate(backend, case):
    """Whatever the priorities hold, every index stays inside the table and its game, and a level without weight is drawn
    uniformly; no error is raised."""
    cfg = sampler_config(True)
    lengths = [5, 300, 0, 7]
    rows = [numpy.full(T, 0.5, numpy.float32) for T in lengths]
    if case == "all zero":
        rows = [numpy.zeros(T, numpy.float32) for T in lengths]
    elif case == "nan":
        rows[0][:] = numpy.nan
        rows[1][[0, 100, 299]] = numpy.nan
        rows[3][2] = numpy.inf              # an infinite game priority is no weight either
    elif case == "negative":
        rows[0][:] = -1
        rows[1][:299] = -2
        rows[3][:] = 0
    items = [(g, game(cfg, T, g, p)) for g, (T, p) in enumerate(zip(lengths, rows))]
    if case == "single live game":
        items = [(6, items[0][1]), (9, items[2][1])]
    store = replay.DeviceGameStore(cfg, backend, 330, max_games=5)
    store.add_many(items)
    table = table_of(store)
    got = device_sample(store, 200, cfg.seed, 1, 312, True, cfg.num_unroll_steps)
    want = oracle_sample(table, 200, cfg.seed, 1, 312, True, cfg.num_unroll_steps, list(cfg.action_space))
    weights = (got.pop("weight"), want.pop("weight"))
    assert_bits(got, want, case)
    assert numpy.allclose(weights[0], weights[1], rtol=1e-6)
    lens = dict((g, len(gh.root_values)) for g, gh in items)
    assert all(lens[int(g)] > 0 and 0 <= p < lens[int(g)] for g, p in zip(got["game_id"], got["pos"]))
    drawn = set(int(g) for g in got["game_id"])
    if case == "all zero":
        assert drawn == {0, 1, 3} and len(set(got["pos"][got["game_id"] == 1])) > 20 and (weights[0] > 0).all()
    elif case == "nan":
        assert drawn == {1} and not set(got["pos"]) & {0, 100, 299} and len(set(got["pos"])) > 20
    elif case == "negative":
        assert drawn == {1} and (got["pos"] == 299).all()
    else:
        assert drawn == {6}


def check_distribution(backend):
    """5 games of lengths 1 .. 9, 50 calls of 4096 samples: every (game, position) frequency within 5 standard deviations
    sqrt(p (1 - p) / N) of its exact probability."""
    cfg = sampler_config(True)
    rs = numpy.random.RandomState(4)
    lengths = [1, 3, 5, 7, 9]
    items = [(g, game(cfg, T, g, rs.random_sample(T).astype(numpy.float32) + 0.05)) for g, T in enumerate(lengths)]
    store = replay.DeviceGameStore(cfg, backend, 40, max_games=5)
    store.add_many(items)
    for per in (True, False):
        counts = numpy.zeros((5, 9))
        for call in range(50):
            got = device_sample(store, 4096, 21, call, 25, per, 0)
            numpy.add.at(counts, (got["game_id"], got["pos"]), 1)
        N = 50 * 4096
        tops = numpy.array([gh.game_priority for _, gh in items], dtype=numpy.float64)
        for g, gh in items:
            T = lengths[g]
            p64 = gh.priorities.astype(numpy.float64)
            exact = (tops[g] / tops.sum()) * (p64 / p64.sum()) if per else numpy.full(T, 1 / (5 * T))
            assert (counts[g, T:] == 0).all()
            assert (numpy.abs(counts[g, :T] / N - exact) <= 5 * numpy.sqrt(exact * (1 - exact) / N)).all(), (per, g)


def restated_update_priorities(buffer, priorities, index_info):
    """update_priorities of the stock buffer (replay_buffer.py:205-228) in this suite's words; the serial suite checks it
    against the unmodified method (the reference tree does not travel to the device suite)."""
    oldest = next(iter(buffer))
    for row, (game_id, pos) in zip(priorities, index_info):
        if game_id >= oldest:
            target = buffer[game_id].priorities
            end = min(pos + len(row), len(target))
            target[pos:end] = row[:end - pos]
            buffer[game_id].game_priority = numpy.max(target)


def scatter_case(cfg, steps):
    """Games 8 .. 15 in a table of 8 slots (ids 0 .. 7 have left: id 3 is stale, its slot holds 11) and an index with
    duplicates, overlapping windows, windows past T, pos = T - 1, the stale id and an id below the oldest game."""
    rs = numpy.random.RandomState(steps)
    lengths = [9, 1, 12, 6, 20, 3, 7, 5]
    games = {8 + k: game(cfg, T, 70 + k, rs.random_sample(T).astype(numpy.float32) + 0.1) for k, T in enumerate(lengths)}
    index = [[8, 2], [8, 2], [8, 4], [10, 11], [12, 0], [12, 3], [12, 1], [3, 0], [0, 1], [9, 0], [13, 2], [11, 5], [8, 8],
             [12, 19], [8, 0], [14, 3], [12, 3]]
    new = (rs.random_sample((len(index), steps)) * 4).astype(numpy.float32)
    return games, index, new


def check_scatter(backend, steps, stock_update=restated_update_priorities):
    cfg = sampler_config(True)
    games, index, new = scatter_case(cfg, steps)
    theirs = copy.deepcopy(games)
    store = replay.DeviceGameStore(cfg, backend, sum(len(g.root_values) + 1 for g in games.values()) + 2, max_games=8)
    store.add_many(list(games.items()))
    before = table_of(store)
    stock_update(theirs, new, index)
    ids, pos = numpy.array([g for g, _ in index], numpy.int64), numpy.array([p for _, p in index], numpy.int32)
    for again in range(2):
        store.update_priorities(new if again else torch.from_numpy(new).to(backend.device), ids, pos)
        after = table_of(store)
        touched = numpy.zeros(store.rows, bool)
        for g, gh in theirs.items():
            got, top = store.priorities_of(g)
            assert numpy.array_equal(got.view(numpy.uint32), gh.priorities.view(numpy.uint32)), (g, got, gh.priorities)
            assert numpy.float32(top).tobytes() == numpy.float32(gh.game_priority).tobytes()
            want_sum = gh.priorities.astype(numpy.float64).sum()
            assert abs(after["sum"][g % 8] - want_sum) <= 1e-12 * want_sum
            if g in ids:
                touched[store.games[g][0]:store.games[g][0] + len(gh.root_values)] = True
        assert (after["owner"] == -1).all()
        assert numpy.array_equal(after["priorities"][~touched], before["priorities"][~touched])
        assert any(not numpy.array_equal(theirs[g].priorities, games[g].priorities) for g in (8, 10, 12))
        for k in ("game", "base", "len"):
            assert numpy.array_equal(after[k], before[k])


def check_upkeep(backend):
    """Slots follow add_many, drop, the stock eviction and the capacity bound in positions; a collision on an occupied
    slot raises StoreFull and leaves the store unchanged; without max_games nothing is allocated."""
    cfg = sampler_config(True, replay_buffer_size=5)
    plain = replay.DeviceGameStore(cfg, backend, 30)
    assert plain.sampler is None and plain.max_games is None
    assert not any(hasattr(plain, name) for name in ("priorities", "owner", "slot_game", "slot_sum"))
    for call in (lambda: plain.sample(1, 0, 0, 1, True), lambda: plain.priorities_of(0),
                 lambda: replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock, device_store=plain, device_sampler=True),
                 lambda: replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock, device_sampler=True)):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError("a store without max_games has no sampler")
    store = replay.DeviceGameStore(cfg, backend, 60, max_games=5)      # fewer rows than five of these games need
    fresh = table_of(store)
    assert (fresh["game"] == -1).all() and (fresh["owner"] == -1).all() and not fresh["priorities"].any()
    assert not fresh["top"].any() and not fresh["sum"].any() and not fresh["len"].any()
    buffer = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=StandInStock, device_store=store, device_sampler=True)
    rs = numpy.random.RandomState(8)
    for k in range(14):
        gh = game(cfg, int(rs.randint(0, 25)), 300 + k)
        replay.fill_initial_priorities(gh, cfg)
        buffer.save_game(gh)
        table = table_of(store)
        assert set(store.games) == set(buffer.buffer) and len(buffer.buffer) <= 5
        for s in range(5):
            resident = [g for g in store.games if g % 5 == s]
            if not resident:
                assert table["game"][s] == -1
                continue
            (g,) = resident
            base, T = store.games[g]
            assert (table["game"][s], table["base"][s], table["len"][s]) == (g, base, T)
            want = buffer.buffer[g].priorities if T else numpy.zeros(0, numpy.float32)
            assert numpy.array_equal(table["priorities"][base:base + T], want) and table["priorities"][base + T] == 0
            assert table["top"][s] == (want.max() if T else 0)
        if any(T for _, T in store.games.values()):
            got = device_sample(store, 16, 1, k, buffer.total_samples, True, 2)
            assert set(got["game_id"]) <= set(store.games)
    newest = max(store.games)
    state = (dict(store.games), store._head, dict(store._slot_owner), table_of(store))
    for items in ([(newest + 5, game(cfg, 2, 1, [1, 1]))], [(newest + 1, game(cfg, 1, 1, [1])), (newest + 6, game(cfg, 1, 2, [1]))]):
        if (newest + 1) % 5 in store._slot_owner and len(items) == 2:
            store.drop(store._slot_owner[(newest + 1) % 5])
            state = (dict(store.games), store._head, dict(store._slot_owner), table_of(store))
        try:
            store.add_many(items)
        except replay.StoreFull:
            pass
        else:
            raise AssertionError("a collision on an occupied slot must raise StoreFull")
        after = table_of(store)
        assert (dict(store.games), store._head, dict(store._slot_owner)) == state[:3]
        assert all(numpy.array_equal(after[k], state[3][k]) for k in after)
    gone = next(iter(store.games))
    store.drop(gone)
    assert table_of(store)["game"][gone % 5] == -1
    values_before = store.priorities.clone()
    survivor = next(g for g in store.games if store.games[g][1])
    store.update(survivor, buffer.buffer[survivor])                         # reanalyse leaves priorities alone
    assert torch.equal(store.priorities, values_before)


class FeedbackStock(StandInStock):
    """The stand-in stock buffer with the priority feedback; games without a position are never drawn by its host path."""

    def update_priorities(self, priorities, index_info):
        restated_update_priorities(self.buffer, priorities, index_info)

    def sample_n_games(self, n_games, force_uniform=False):
        keep = self.buffer
        self.buffer = {g: h for g, h in keep.items() if len(h.root_values)}
        try:
            return super().sample_n_games(n_games, force_uniform)
        finally:
            self.buffer = keep


def check_end_to_end(backend, kind, per):
    cfg = sampler_config(per, kind, batch_size=24)
    cfg.value_loss_weight = 0.25
    rs = numpy.random.RandomState(3)
    lengths = [int(T) for T in rs.randint(1, 20, size=12)] + [0]
    games = [game(cfg, T, 500 + k) for k, T in enumerate(lengths)]
    store = replay.DeviceGameStore(cfg, backend, sum(lengths) + len(lengths), max_games=16)
    ours = replay.ReplayBuffer(dict(CHECKPOINT), {}, cfg, stock=FeedbackStock, device_store=store, device_sampler=True)
    theirs = FeedbackStock(dict(CHECKPOINT), {}, cfg)
    for gh in games:
        ours.save_game(gh)
        theirs.save_game(copy.deepcopy(gh))
    U, total = cfg.num_unroll_steps, ours.total_samples
    # get_batch == the gather of the downloaded draws
    base, length, pos, tape, game_id, weight = store.sample(cfg.batch_size, cfg.seed, 0, total, per, U)
    index_batch, tensors = ours.get_batch()
    assert isinstance(index_batch, replay.DeviceIndexBatch) and len(index_batch) == cfg.batch_size
    assert index_batch.tolist() == [[int(g), int(p)] for g, p in zip(game_id.cpu(), pos.cpu())] == list(index_batch)
    assert index_batch[3] == index_batch.tolist()[3]
    obs, (value, reward, policy, action, scale) = store.batch([g for g, _ in index_batch], [p for _, p in index_batch],
                                                              tape.cpu().numpy(), U)
    for got, want in zip(tensors, (obs, action, value, reward, policy, weight, scale)):
        assert (got is None and want is None and not per) or torch.equal(got, want)
    bare = store.gather(base, length, pos)                 # no tape: the absorbing steps take action 0
    zero = store.batch([g for g, _ in index_batch], [p for _, p in index_batch], None, U)
    assert torch.equal(bare[0], zero[0]) and all(torch.equal(a, b) for a, b in zip(bare[1], zero[1]))
    # two training steps against update_weights + the stock update_priorities on the same draws
    torch.manual_seed(5)
    width = int(numpy.prod(store.sample_shape))
    model = trainer_loss_cases.TinyModel(width, 8, cfg.support_size, len(cfg.action_space)).to(backend.device)
    twin = trainer_loss_cases.TinyModel(width, 8, cfg.support_size, len(cfg.action_space)).to(backend.device)
    twin.load_state_dict(model.state_dict())
    opt, opt_twin = torch.optim.SGD(model.parameters(), lr=0.05), torch.optim.SGD(twin.parameters(), lr=0.05)
    for step in (1, 2):
        base, length, pos, tape, game_id, weight = store.sample(cfg.batch_size, cfg.seed, step, total, per, U)
        obs, (value, reward, policy, action, scale) = store.gather(base, length, pos, tape, U)
        want = trainer.update_weights(twin, opt_twin, (obs, action, value, reward, policy, weight, scale), cfg, backend=backend)
        if per:
            theirs.update_priorities(want[0], [[int(g), int(p)] for g, p in zip(game_id.cpu(), pos.cpu())])
        packed = trainer.train_step(model, opt, ours, cfg, backend=backend)
        assert torch.is_tensor(packed) and packed.shape == (4,) and packed.device.type == backend.device.type
        assert numpy.array_equal(packed.cpu().numpy(), numpy.array(want[1:], numpy.float32))
        for a, b in zip(model.parameters(), twin.parameters()):
            assert torch.equal(a, b)
    changed = False
    for g, gh in theirs.buffer.items():
        got, top = store.priorities_of(g)
        if per and len(gh.root_values):
            assert numpy.array_equal(got.view(numpy.uint32), gh.priorities.view(numpy.uint32)), g
            assert numpy.float32(top).tobytes() == numpy.float32(gh.game_priority).tobytes()
            changed = changed or not numpy.array_equal(got, ours.buffer[g].priorities)
        else:
            assert not got.any() and top == 0
    assert changed == per                  # the host histories went stale ...
    ours.sync_priorities()                 # ... until they are written back
    for g, gh in ours.buffer.items():
        if per and len(gh.root_values):
            got, top = store.priorities_of(g)
            assert numpy.array_equal(gh.priorities, got) and gh.game_priority == top and gh.priorities.flags.writeable
    # a host index keeps the stock method
    if per:
        host_index = [[g, 0] for g in list(ours.buffer)[:2] if len(ours.buffer[g].root_values)]
        ours.update_priorities(numpy.full((len(host_index), 3), 9, numpy.float32), host_index)
        assert all(ours.buffer[g].priorities[0] == 9 for g, _ in host_index)
        assert all(store.priorities_of(g)[0][0] != 9 for g, _ in host_index)


def check_abi_refusals(backend):
    """Null sampler, n < 0, steps < 1, missing outputs / columns / workspace: MZX_ERR_INVALID with a message, nothing
    launched (the outputs keep their fill)."""
    lib = backend.lib
    cfg = sampler_config(True)
    store = replay.DeviceGameStore(cfg, backend, 20, max_games=4)
    store.add_many([(0, game(cfg, 3, 1, [1, 2, 3]))])
    store._flush_slots()
    n, U = 4, 2
    out = dict(d_base=torch.full((n,), 77, dtype=torch.int64), d_len=torch.full((n,), 77, dtype=torch.int32),
               d_pos=torch.full((n,), 77, dtype=torch.int32), d_absorbing_actions=torch.full((n, U + 1), 77, dtype=torch.int32),
               d_game_id=torch.full((n,), 77, dtype=torch.int64), d_weight=torch.full((n,), 77, dtype=torch.float32))
    out = {k: v.to(backend.device) for k, v in out.items()}
    raw = backend.zeros((n,), torch.float64)

    def sampler(**fields):
        s = _lib.ReplaySampler.from_buffer_copy(store.sampler)
        s.d_raw, s.raw_capacity = raw.data_ptr(), n
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    def io(**fields):
        x = _lib.ReplaySampleIO()
        x.seed, x.call_counter, x.total_samples, x.num_samples, x.per, x.num_unroll_steps, x.num_actions = 1, 0, 3, n, 1, U, store.A
        for k, v in out.items():
            setattr(x, k, v.data_ptr())
        for k, v in fields.items():
            setattr(x, k, v)
        return x

    def refused(rc, word):
        assert rc == -1 and word in lib.mzx_last_error().decode(), (rc, lib.mzx_last_error())       # MZX_ERR_INVALID
        assert all((v == 77).all() for v in out.values())

    stream, ref = backend.stream(), ctypes.byref
    refused(lib.mzx_replay_sample(None, ref(io()), stream), "null sampler")
    refused(lib.mzx_replay_sample(ref(sampler()), None, stream), "null io")
    refused(lib.mzx_replay_sample(ref(sampler()), ref(io(num_samples=-1)), stream), "num_samples")
    refused(lib.mzx_replay_sample(ref(sampler()), ref(io(num_actions=0)), stream), "num_actions")
    for field in out:
        refused(lib.mzx_replay_sample(ref(sampler()), ref(io(**{field: None})), stream), "missing output")
    refused(lib.mzx_replay_sample(ref(sampler(d_slot_sum=None)), ref(io()), stream), "missing sampler column")
    refused(lib.mzx_replay_sample(ref(sampler(slots=0)), ref(io()), stream), "positive")
    refused(lib.mzx_replay_sample(ref(sampler(raw_capacity=n - 1)), ref(io()), stream), "workspace")
    refused(lib.mzx_replay_sample(ref(sampler(d_tile_prefix=None)), ref(io()), stream), "workspace")
    new, ids, pos = backend.zeros((n, 2), torch.float32), backend.zeros((n,), torch.int64), backend.zeros((n,), torch.int32)
    before = table_of(store)
    ptr = backend.ptr
    refused(lib.mzx_replay_update_priorities(None, ptr(new), ptr(ids), ptr(pos), n, 2, stream), "null sampler")
    refused(lib.mzx_replay_update_priorities(ref(sampler()), ptr(new), ptr(ids), ptr(pos), -1, 2, stream), "negative")
    refused(lib.mzx_replay_update_priorities(ref(sampler()), ptr(new), ptr(ids), ptr(pos), n, 0, stream), "steps")
    refused(lib.mzx_replay_update_priorities(ref(sampler()), None, ptr(ids), ptr(pos), n, 2, stream), "missing buffer")
    refused(lib.mzx_replay_update_priorities(ref(sampler(d_owner=None)), ptr(new), ptr(ids), ptr(pos), n, 2, stream), "column")
    slots = backend.zeros((1,), torch.int32)
    refused(lib.mzx_replay_sampler_refresh(None, ptr(slots), 1, stream), "null sampler")
    refused(lib.mzx_replay_sampler_refresh(ref(sampler()), ptr(slots), -1, stream), "negative")
    refused(lib.mzx_replay_sampler_refresh(ref(sampler()), None, 1, stream), "missing slot list")
    after = table_of(store)
    assert all(numpy.array_equal(after[k], before[k]) for k in after)
    # the accepted call after all that: PER off needs neither d_weight nor the raw workspace; n == 0 is a no-op
    assert lib.mzx_replay_sample(ref(sampler(d_raw=None, raw_capacity=0)), ref(io(per=0, d_weight=None)), stream) == 0
    assert (out["d_game_id"] == 0).all() and (out["d_weight"] == 77).all()
    assert lib.mzx_replay_sample(ref(sampler()), ref(io(num_samples=0)), stream) == 0
    # weights are never NaN: 0 for every sample when total_samples <= 0, and when no game is live (game_id -1, T 0)
    assert lib.mzx_replay_sample(ref(sampler()), ref(io(total_samples=0)), stream) == 0
    assert (out["d_weight"] == 0).all() and (out["d_game_id"] == 0).all()
    empty = replay.DeviceGameStore(cfg, backend, 20, max_games=4)
    s = _lib.ReplaySampler.from_buffer_copy(empty.sampler)
    s.d_raw, s.raw_capacity = raw.data_ptr(), n
    assert lib.mzx_replay_sample(ref(s), ref(io()), stream) == 0
    assert (out["d_weight"] == 0).all() and (out["d_game_id"] == -1).all() and (out["d_len"] == 0).all()
    assert (out["d_base"] == 0).all() and (out["d_pos"] == 0).all()
    # a refresh of an empty slot writes 0 / 0; one listed out of range is passed over
    listed = torch.tensor([1, 9, -1], dtype=torch.int32).to(backend.device)
    assert lib.mzx_replay_sampler_refresh(ref(sampler()), ptr(listed), 3, stream) == 0
    assert all(numpy.array_equal(table_of(store)[k], before[k]) for k in before)
