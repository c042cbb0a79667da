"""
Self-play draws on the device (mzx_selfplay_draws, mzx_selfplay_select_device, mzx_selfplay_move_device;
csrc/mzx_draws.h): the numpy / math restatement of the definition and the check functions.  tests/test_device_draws.py
runs them on the serial build (tests/hostcheck: same libm as Python's math, so the noise is bit-exact there),
tests/test_gpu_device_draws.py on the device library (tape and action choice bit-exact, noise within 1e-12).

The restatement records the relative margin of every comparison the gamma sampler makes: a last-bit difference of a device
log / pow could only flip an accept / reject decision whose margin is of that order, and the grid is asserted to stay
above MARGIN_FLOOR -- so no row may be excused on the device.
"""
import ctypes
import functools
import math

import numpy
import torch

from mzx import _lib, draws

M32 = 0xFFFFFFFF
KEY_XOR = 0x53454C46
NOISE, TAPE, ACTION = 0, 1, 2
SEED = 0x1234_5678_9ABC_DEF0
BIG_COUNTER = (1 << 32) + 17

BATCHES = [1, 5, 70]                       # either side of the four wavefronts of a workgroup
ACTIONS = [1, 2, 7, 63, 64, 65, 130]
ALPHAS = [0.1, 0.3, 1.0, 2.5]              # shape < 1, shape < 1, exponential, Marsaglia-Tsang
TAPES = [1, 4, 5, 16, 33]
MARGIN_FLOOR = 1e-9
NOISE_GPU_RTOL = 1e-12
INF = float("inf")

KAT = [  # Random123 known-answer vectors of philox4x32-10: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


# ------------------------------------------------------------------------------------------------ the restatement

def philox(c, k):
    """Philox4x32-10 of one counter (4 ints) under one key (2 ints), in Python integers."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def block(seed, stream, counter, purpose, index):
    return philox([stream & M32, counter & M32, (counter >> 32) & M32, (purpose << 30) | index],
                  [seed & M32, ((seed >> 32) & M32) ^ KEY_XOR])


def u53(hi, lo):
    return float((hi << 21) | (lo >> 11)) * 2.0 ** -53


def tape_row(seed, stream, counter, words):
    out = []
    for b in range((words + 3) // 4):
        out += block(seed, stream, counter, TAPE, b)
    return numpy.array(out[:words], dtype=numpy.uint32)


def action_uniform(seed, stream, counter):
    w = block(seed, stream, counter, ACTION, 0)
    return u53(w[0], w[1])


class Margins:
    def __init__(self):
        self.smallest, self.count = INF, 0

    def note(self, a, b):
        self.count += 1
        scale = max(abs(a), abs(b))
        self.smallest = min(self.smallest, abs(a - b) / scale if scale > 0 else INF)


class ChildStream:
    """The uniforms of root child j: two per block, blocks (j << 14) | 0, 1, ...; and numpy's legacy gamma over them."""

    def __init__(self, seed, stream, counter, child, margins):
        self.args, self.child, self.blocks, self.pending, self.gauss, self.m = (seed, stream, counter), child, 0, None, None, margins

    def next(self):
        if self.pending is not None:
            u, self.pending = self.pending, None
            return u
        w = block(*self.args, NOISE, (self.child << 14) | (self.blocks & 0x3FFF))
        self.blocks += 1
        self.pending = u53(w[2], w[3])
        return u53(w[0], w[1])

    def exponential(self):
        return -math.log(1.0 - self.next())

    def gauss_polar(self):
        if self.gauss is not None:
            g, self.gauss = self.gauss, None
            return g
        while True:
            x1 = 2.0 * self.next() - 1.0
            x2 = 2.0 * self.next() - 1.0
            r2 = x1 * x1 + x2 * x2
            self.m.note(r2, 1.0)
            if not (r2 >= 1.0 or r2 == 0.0):
                break
        f = math.sqrt(-2.0 * math.log(r2) / r2)
        self.gauss = f * x1
        return f * x2

    def gamma(self, shape):
        m = self.m
        if shape == 1.0:
            return self.exponential()
        if shape == 0.0:
            return 0.0
        if shape < 1.0:
            while True:
                U = self.next()
                V = self.exponential()
                m.note(U, 1.0 - shape)
                if U <= 1.0 - shape:
                    X = math.pow(U, 1.0 / shape)
                    m.note(X, V)
                    if X <= V:
                        return X
                else:
                    Y = -math.log((1 - U) / shape)
                    X = math.pow(1.0 - shape + shape * Y, 1.0 / shape)
                    m.note(X, V + Y)
                    if X <= V + Y:
                        return X
        b = shape - 1.0 / 3.0
        c = 1.0 / math.sqrt(9 * b)
        while True:
            while True:
                X = self.gauss_polar()
                V = 1.0 + c * X
                m.note(c * X, -1.0)
                if not V <= 0.0:
                    break
            V = V * V * V
            U = self.next()
            bound = 1.0 - 0.0331 * (X * X) * (X * X)
            m.note(U, bound)
            if U < bound:
                return b * V
            lhs, rhs = math.log(U), 0.5 * X * X + b * (1.0 - V + math.log(V))
            m.note(lhs, rhs)
            if lhs < rhs:
                return b * V


def noise_row(seed, stream, counter, n, A, alpha, margins):
    g = [ChildStream(seed, stream, counter, j, margins).gamma(alpha) for j in range(n)]
    total = 0.0
    for v in g:
        total = total + v
    row = numpy.zeros(A, numpy.float64)
    if total > 0.0 and math.isfinite(total):
        row[:n] = [v / total for v in g]
    else:
        row[:n] = 1.0 / n
    return row


def choose(u, legal_row, visit_row, T, table, table_temperatures):
    """The action of one game: legal_row padded with -1, visit_row by action."""
    legal = [int(a) for a in legal_row if a >= 0]
    n = len(legal)
    c = [int(visit_row[a]) for a in legal]
    if T == 0:
        return legal[c.index(max(c))]
    if T == INF:
        return legal[min(n - 1, int(math.floor(u * n)))]
    row = [i for i, t in enumerate(table_temperatures) if t == T][-1]
    w = [float(table[row][v]) for v in c]
    total = 0.0
    for v in w:
        total = total + v
    t = u * total
    acc, last = 0.0, 0
    for j, v in enumerate(w):
        acc = acc + v
        if acc > t:
            return legal[j]
        if v > 0.0:
            last = j
    return legal[max([j for j, v in enumerate(w) if v > 0.0] or [0])]


# ------------------------------------------------------------------------------------------------ the grid

def legal_rows(B, A):
    """n = 1 + (7k + 3) % A legal actions per row, in decreasing action order, padded with -1."""
    legal = numpy.full((B, A), -1, numpy.int32)
    for k in range(B):
        n = 1 + (7 * k + 3) % A
        legal[k, :n] = numpy.arange(n)[::-1]
    return legal


def grid_case(bi, ai):
    B, A = BATCHES[bi], ACTIONS[ai]
    explicit = (ai + bi) % 2 == 0
    streams = (numpy.arange(B, dtype=numpy.int32)[::-1] * 3 + 11).copy() if explicit else None
    return dict(B=B, A=A, alpha=ALPHAS[(ai + bi) % 4], tape_words=TAPES[(ai + 2 * bi) % 5], streams=streams,
                first_stream=0 if explicit else 1000 + ai, counter=BIG_COUNTER + ai if (ai + bi) % 3 else 5 + bi,
                seed=SEED + 977 * ai + bi, legal=legal_rows(B, A))


def stream_ids(case):
    return case["streams"] if case["streams"] is not None else case["first_stream"] + numpy.arange(case["B"])


@functools.lru_cache(maxsize=None)
def grid_reference(bi, ai):
    """(noise [B][A], tape [B][W], smallest margin, comparisons) of one grid case, computed once per process."""
    c = grid_case(bi, ai)
    m = Margins()
    ids = stream_ids(c)
    noise = numpy.stack([noise_row(c["seed"], int(ids[k]), c["counter"], int((c["legal"][k] >= 0).sum()), c["A"], c["alpha"], m)
                         for k in range(c["B"])])
    tape = numpy.stack([tape_row(c["seed"], int(ids[k]), c["counter"], c["tape_words"]) for k in range(c["B"])])
    noise.setflags(write=False)
    tape.setflags(write=False)
    return noise, tape, m.smallest, m.count


def lib_draws(backend, c, noise=True, **over):
    c = dict(c, **over)
    t_noise, t_tape = draws.root_draws(backend, c["seed"], c["counter"], c["B"], c["A"], c["tape_words"], alpha=c["alpha"],
                                       legal=c.get("legal"), n=c.get("n"), streams=c["streams"], first_stream=c["first_stream"],
                                       noise=noise)
    return (None if t_noise is None else t_noise.cpu().numpy()), t_tape.cpu().numpy().view(numpy.uint32)


def bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


# ------------------------------------------------------------------------------------------------ checks

def check_known_answers():
    for counter, key, want in KAT:
        assert philox(counter, key) == want
    # the layout of this path: key (seed lo, seed hi ^ "SELF"), counter (stream, counter lo, counter hi, purpose << 30 | index)
    stream, counter = 0x243F6A88, (0x13198A2E << 32) | 0x85A308D3
    seed = (0x299F31D0 ^ KEY_XOR) << 32 | 0xA4093822
    assert block(seed, stream, counter, 0, 0x03707344) == KAT[2][2]


def check_library_words(backend):
    """The library's tape words ARE the Philox blocks of the layout (known answer through the entry point)."""
    seed = (0x299F31D0 ^ KEY_XOR) << 32 | 0xA4093822
    counter = (0x13198A2E << 32) | 0x85A308D3
    # purpose 1 (tape): index b -> counter word 3 = 0x40000000 | b
    _, tape = lib_draws(backend, dict(seed=seed, counter=counter, B=1, A=1, tape_words=8, alpha=0.3, streams=None,
                                      first_stream=0x243F6A88), noise=False)
    want = philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x40000000], [0xA4093822, 0x299F31D0]) + \
        philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x40000001], [0xA4093822, 0x299F31D0])
    assert [int(v) for v in tape[0]] == want


def check_margins(ai):
    """The guard of the device comparison: no accept / reject decision of the grid sits within MARGIN_FLOOR of its boundary."""
    smallest, count = INF, 0
    for bi in range(len(BATCHES)):
        _, _, m, n = grid_reference(bi, ai)
        smallest, count = min(smallest, m), count + n
    print(f"A={ACTIONS[ai]}: smallest relative margin {smallest:.3e} over {count} comparisons")
    assert smallest >= MARGIN_FLOOR, (ACTIONS[ai], smallest)
    return smallest, count


def check_grid(backend, ai, exact_noise):
    """Tape bit for bit; noise bit for bit (serial build) or within NOISE_GPU_RTOL (device); row properties."""
    worst = 0.0
    for bi in range(len(BATCHES)):
        c = grid_case(bi, ai)
        want_noise, want_tape, margin, _ = grid_reference(bi, ai)
        assert margin >= MARGIN_FLOOR
        noise, tape = lib_draws(backend, c)
        assert numpy.array_equal(tape, want_tape), (c["B"], c["A"])
        n = (c["legal"] >= 0).sum(1)
        past = numpy.arange(c["A"])[None, :] >= n[:, None]
        assert numpy.array_equal(bits(noise)[past], numpy.zeros(int(past.sum()), numpy.int64))      # exactly +0.0
        assert (noise[~past] > 0).all()
        assert (noise[n == 1, 0] == 1.0).all()
        sums = numpy.array([math.fsum(r) for r in noise])
        assert (numpy.abs(sums - 1.0) <= 4 * 2.0 ** -52).all(), numpy.abs(sums - 1.0).max()
        if exact_noise:
            assert numpy.array_equal(bits(noise), bits(want_noise)), (c["B"], c["A"], c["alpha"])
        else:
            rel = numpy.abs(noise - want_noise)[~past] / want_noise[~past]
            worst = max(worst, float(rel.max()))
            assert (rel <= NOISE_GPU_RTOL).all(), (c["B"], c["A"], c["alpha"], float(rel.max()))
        # the same draws without noise, and with n given explicitly instead of legal rows
        _, tape2 = lib_draws(backend, c, noise=False)
        assert numpy.array_equal(tape2, want_tape)
        noise3, _ = lib_draws(backend, c, legal=None, n=n.astype(numpy.int32))
        assert numpy.array_equal(bits(noise3), bits(noise))
    if not exact_noise:
        print(f"A={ACTIONS[ai]}: largest relative noise difference {worst:.3e} (gate {NOISE_GPU_RTOL:.0e})")
    return worst


def check_tape_prefix(backend):
    c = dict(grid_case(1, 2), tape_words=16)
    _, short = lib_draws(backend, c, noise=False)
    _, long_ = lib_draws(backend, c, noise=False, tape_words=128)
    assert long_.shape == (c["B"], 128) and numpy.array_equal(long_[:, :16], short)
    ids = stream_ids(c)
    assert numpy.array_equal(long_[3], tape_row(c["seed"], int(ids[3]), c["counter"], 128))


def check_determinism(backend):
    """(seed, stream, counter) alone decide a row: any batch, any order; each of the three matters; purposes are apart."""
    A, W, alpha = 7, 16, 0.3
    legal = numpy.tile(numpy.arange(A, dtype=numpy.int32), (70, 1))
    streams = numpy.arange(70, dtype=numpy.int32)
    base = dict(seed=SEED, counter=BIG_COUNTER, B=70, A=A, tape_words=W, alpha=alpha, streams=streams, first_stream=0, legal=legal)
    noise, tape = lib_draws(backend, base)
    perm = numpy.random.RandomState(3).permutation(70).astype(numpy.int32)
    noise_p, tape_p = lib_draws(backend, base, streams=perm)
    assert numpy.array_equal(bits(noise_p), bits(noise[perm])) and numpy.array_equal(tape_p, tape[perm])
    few = numpy.array([69, 0, 33], numpy.int32)
    noise_f, tape_f = lib_draws(backend, base, B=3, streams=few, legal=legal[:3])
    assert numpy.array_equal(bits(noise_f), bits(noise[few])) and numpy.array_equal(tape_f, tape[few])
    noise_1, tape_1 = lib_draws(backend, base, B=1, streams=None, first_stream=42, legal=legal[:1])
    assert numpy.array_equal(bits(noise_1[0]), bits(noise[42])) and numpy.array_equal(tape_1[0], tape[42])
    for change in (dict(seed=SEED + 1), dict(seed=SEED + (1 << 32)), dict(counter=BIG_COUNTER + 1),
                   dict(counter=BIG_COUNTER + (1 << 32)), dict(streams=streams + 70)):
        noise_c, tape_c = lib_draws(backend, base, **change)
        assert not (bits(noise_c) == bits(noise)).all(1).any(), change
        assert not (tape_c == tape).all(1).any(), change
    assert len({tuple(r) for r in tape.tolist()}) == 70 and len({tuple(r) for r in bits(noise).tolist()}) == 70
    # purposes do not collide: the words behind child 0's first uniforms are not the tape's first block
    for k in (0, 42):
        first_noise = block(SEED, k, BIG_COUNTER, NOISE, 0)
        assert [int(v) for v in tape[k, :4]] == block(SEED, k, BIG_COUNTER, TAPE, 0) != first_noise
        assert block(SEED, k, BIG_COUNTER, ACTION, 0) not in (first_noise, [int(v) for v in tape[k, :4]])


def select_case(B, A, seed):
    rs = numpy.random.RandomState(seed)
    legal = numpy.full((B, A), -1, numpy.int32)
    visits = numpy.zeros((B, A), numpy.int32)
    for k in range(B):
        n = 1 + (7 * k + 3) % A
        acts = rs.permutation(A)[:n]
        legal[k, :n] = acts
        visits[k, acts] = rs.randint(0, 40, size=n)
        if k % 5 == 1:                       # all-zero counts but one
            visits[k] = 0
            visits[k, acts[n // 2]] = 9
        if k % 5 == 2 and n > 1:             # ties for the maximum
            visits[k, acts] = 3
            visits[k, acts[[0, n - 1]]] = 17
        if k % 5 == 3:                       # nothing visited at all
            visits[k] = 0
    temps = numpy.array([0.0, INF, 1.0, 0.5, 0.25])[(numpy.arange(B) * 3 + seed) % 5]
    return legal, visits, temps


def check_select(backend, ai):
    A = ACTIONS[ai]
    for bi, B in enumerate(BATCHES):
        legal, visits, temps = select_case(B, A, 10 * ai + bi)
        table, tt = draws.power_table(temps, 41)
        explicit = (ai + bi) % 2 == 1
        streams = (numpy.arange(B, dtype=numpy.int32)[::-1] * 5 + 2).copy() if explicit else None
        first = 0 if explicit else 300
        ids = streams if explicit else first + numpy.arange(B)
        counter = BIG_COUNTER * 3 + bi
        got = draws.select(backend, SEED, counter, legal, visits, temps, table, tt, streams=streams, first_stream=first).cpu().numpy()
        want = [choose(action_uniform(SEED, int(ids[k]), counter), legal[k], visits[k], temps[k], table, tt) for k in range(B)]
        assert got.dtype == numpy.int64 and got.tolist() == want, (B, A)
        for k in range(B):
            assert got[k] in legal[k]


def check_select_boundaries(backend):
    """Crafted uniforms: a target equal to a prefix (strict >), a target no prefix exceeds (last positive weight), the ends
    of the uniform branch, zero weights around the chosen one."""
    table, tt = draws.power_table([1.0], 20)
    legal = numpy.array([[3, 1, 0, 2, -1]] * 8, numpy.int32)
    visits = numpy.zeros((8, 5), numpy.int32)
    visits[:, [3, 1, 0, 2]] = [2, 4, 2, 0]           # weights in legal order 2, 4, 2, 0: prefixes 2, 6, 8, 8
    visits[6] = 0                                     # no positive weight anywhere
    temps = numpy.array([1.0, 1.0, 1.0, 1.0, INF, INF, 1.0, 1.0])
    u = numpy.array([0.25, numpy.nextafter(0.25, 0), 0.75, 1.0, 1.0, numpy.nextafter(0.25, 0), 0.5, 0.0])
    got = draws.select(backend, 1, 1, legal, visits, temps, table, tt, uniforms=u).cpu().numpy().tolist()
    #        t = 2 -> prefix 6; just below -> prefix 2; t = 6 -> prefix 8; t = 8: none -> last positive (index 2)
    assert got == [1, 3, 0, 0, 2, 3, 3, 3], got
    assert got == [choose(u[k], legal[k], visits[k], temps[k], table, tt) for k in range(8)]
    # the largest uniform the generator can give, 1 - 2^-53: t stays below the total (u * total < total in binary64 for
    # every u < 1), so the last positive weight is reached through its prefix, trailing zero weights are never chosen
    u1 = numpy.full(3, 1.0 - 2.0 ** -53)
    counts = numpy.array([[1, 3, 0, 0, 0]] * 3, numpy.int32)
    table3, tt3 = draws.power_table([0.25], 4)
    legal2 = numpy.array([[0, 1, 2, -1, -1], [1, 0, 2, 3, 4], [2, 1, 0, -1, -1]], numpy.int32)
    got = draws.select(backend, 1, 1, legal2, counts, numpy.full(3, 0.25), table3, tt3, uniforms=u1).cpu().numpy().tolist()
    assert got == [1, 0, 0], got


def check_distribution(backend):
    """20 000 Dirichlet(0.3 x 7) rows: every coordinate is Beta(alpha, 6 alpha); mean and second moment within 5 standard
    errors, the errors from the exact Beta moments."""
    N, n, alpha = 20000, 7, 0.3
    legal = numpy.tile(numpy.arange(n, dtype=numpy.int32), (N, 1))
    noise, _ = lib_draws(backend, dict(seed=SEED + 5, counter=9, B=N, A=n, tape_words=1, alpha=alpha, streams=None,
                                       first_stream=0, legal=legal))
    a, s = alpha, n * alpha

    def moment(k):          # E[X^k] of Beta(a, s - a) = prod (a + i) / (s + i)
        return math.prod((a + i) / (s + i) for i in range(k))

    m1, m2, m4 = moment(1), moment(2), moment(4)
    se1, se2 = math.sqrt((m2 - m1 * m1) / N), math.sqrt((m4 - m2 * m2) / N)
    assert abs(m1 - 1.0 / n) < 1e-15
    mean, second = noise.mean(0), (noise * noise).mean(0)
    print("mean deviations / se:", numpy.round((mean - m1) / se1, 2), " second moment:", numpy.round((second - m2) / se2, 2))
    assert (numpy.abs(mean - m1) <= 5 * se1).all() and (numpy.abs(second - m2) <= 5 * se2).all()


def check_refusals(backend):
    lib = backend.lib
    ok = dict(seed=1, counter=1, B=2, A=3, tape_words=4, alpha=0.3, streams=None, first_stream=0,
              legal=numpy.array([[0, 1, 2], [1, -1, -1]], numpy.int32))
    lib_draws(backend, ok)
    for bad, text in ((dict(tape_words=0), "tape_words"), (dict(tape_words=-3), "tape_words"),
                      (dict(A=draws.MAX_ACTIONS + 1, legal=numpy.zeros((2, draws.MAX_ACTIONS + 1), numpy.int32)), "at most"),
                      (dict(legal=None), "d_legal_actions or d_n"), (dict(alpha=0.0), "dirichlet_alpha")):
        try:
            lib_draws(backend, ok, **bad)
        except _lib.MzxError as e:
            assert text in str(e), (bad, str(e))
        else:
            raise AssertionError(f"accepted {bad}")
    tape = backend.zeros((2, 4), torch.int32)
    d = _lib.Draws(seed=1, counter=1, num_games=2, action_space_size=3, tape_words=4, dirichlet_alpha=0.3)
    assert lib.mzx_selfplay_draws(ctypes.byref(d), backend.stream()) == -1 and b"d_tape" in lib.mzx_last_error()
    assert lib.mzx_selfplay_draws(None, backend.stream()) == -1
    d.d_tape = backend.ptr(tape)
    assert lib.mzx_selfplay_draws(ctypes.byref(d), backend.stream()) == 0          # no noise asked for: no row count needed
    d.num_games = 0
    assert lib.mzx_selfplay_draws(ctypes.byref(d), backend.stream()) == -1
    d.num_games = 2
    s = _lib.DrawsSelect()
    assert lib.mzx_selfplay_select_device(ctypes.byref(d), ctypes.byref(s), backend.stream()) == -1
    assert b"required" in lib.mzx_last_error()
    assert lib.mzx_selfplay_select_device(ctypes.byref(d), None, backend.stream()) == -1
    legal, visits = backend.zeros((2, 3), torch.int32), backend.zeros((2, 3), torch.int32)
    temps, action = backend.zeros((2,), torch.float64), backend.zeros((2,), torch.int64)
    s.d_legal_actions, s.d_visit_counts, s.d_temperature = backend.ptr(legal), backend.ptr(visits), backend.ptr(temps)
    assert lib.mzx_selfplay_select_device(ctypes.byref(d), ctypes.byref(s), backend.stream()) == -1      # d_action missing
    s.d_action = backend.ptr(action)
    s.num_temperatures = 1
    assert lib.mzx_selfplay_select_device(ctypes.byref(d), ctypes.byref(s), backend.stream()) == -1
    assert b"power table" in lib.mzx_last_error()
    s.num_temperatures = 0
    assert lib.mzx_selfplay_select_device(ctypes.byref(d), ctypes.byref(s), backend.stream()) == 0


# ------------------------------------------------------------------------------------------------ fused move, engine, self-play

def _net(backend, kind, **extra):
    from mzx import configs, models, synthetic

    if kind == "fc":          # CartPole-class fully connected network, 2 actions
        cfg = configs.cartpole(num_simulations=10, **extra)
    else:                     # tic-tac-toe-class residual network, 9 actions
        cfg = configs.tictactoe(num_simulations=8, **extra)
    model = models.MuZeroNetwork(cfg, _backend=backend)
    model.set_weights(synthetic.fill_state_dict(model.state_dict(), 9))
    model.eval()
    return cfg, model


def _move_inputs(cfg, B, seed):
    from mzx import synthetic

    A = len(cfg.action_space)
    obs = numpy.ascontiguousarray(numpy.asarray(synthetic.observations(B, cfg.observation_shape, seed=seed), numpy.float32))
    rs = numpy.random.RandomState(seed)
    legal = numpy.full((B, A), -1, numpy.int32)
    for k in range(B):
        n = A if A == 2 else 1 + (7 * k + 3) % A          # restricted legal sets where the game has them
        legal[k, :n] = numpy.sort(rs.permutation(A)[:n])
    to_play = (numpy.arange(B) % len(cfg.players)).astype(numpy.int32)
    return obs, legal, to_play


def check_composition(backend, kind):
    """One fused move (mzx_selfplay_move_device) against mzx_selfplay_draws, mzx_search_run on those arrays and
    mzx_selfplay_select_device: visits, root values, info and actions bit for bit.  Shard of 5."""
    from mzx import search

    B = 5
    cfg, model = _net(backend, kind)
    A = len(cfg.action_space)
    obs, legal, to_play = _move_inputs(cfg, B, 4)
    temps = numpy.array([1.0, 0.0, 0.5, INF, 0.25])
    streams = numpy.array([9, 2, 40, 41, 7], numpy.int32)
    for counter, ids in ((3, streams), (BIG_COUNTER, None)):
        engine = search.BatchedMCTS(cfg, model, B, device_draws=True)
        engine.draw_seed = SEED
        fused = engine.run(obs, legal, to_play, True, None, streams=ids, counter=counter, temperature=temps)
        # the separate calls, on a second engine (its own arena and handle)
        other = search.BatchedMCTS(cfg, model, B)
        noise, tape = draws.root_draws(backend, SEED, counter, B, A, search.TAPE_WORDS, alpha=cfg.root_dirichlet_alpha, legal=legal,
                                       streams=ids, noise=True)
        io, out, keep = other.make_io(B, obs.reshape(B, -1), legal, to_play, noise, tape)
        arena = other.arena(B)
        backend.lib.check(backend.lib.mzx_search_run(other.handle(B), ctypes.byref(io), backend.ptr(arena), arena.numel(), backend.stream()))
        visits = out["visits"].cpu().numpy()
        table, tt = draws.power_table(temps, other.num_nodes + 1)
        actions = draws.select(backend, SEED, counter, legal, visits, temps, table, tt, streams=ids).cpu().numpy()
        assert numpy.array_equal(fused.visit_counts, visits) and visits.sum() == B * cfg.num_simulations
        assert numpy.array_equal(bits(fused.root_values), bits(out["root_value"].cpu().numpy()))
        assert numpy.array_equal(bits(fused.root_predicted_values), bits(out["predicted"].cpu().numpy()))
        info = out["info"].cpu().numpy()
        assert numpy.array_equal(fused.max_tree_depth, info[:, 0]) and numpy.array_equal(fused.tape_used, info[:, 2])
        assert numpy.array_equal(fused.flags, info[:, 1]) and numpy.array_equal(fused.sum_depth, info[:, 3])
        assert fused.actions.dtype == numpy.int64 and numpy.array_equal(fused.actions, actions)
        for k in range(B):
            assert fused.actions[k] in legal[k]
        # ... and the restatement of the draws behind them
        who = ids if ids is not None else numpy.arange(B)
        want_tape = numpy.stack([tape_row(SEED, int(who[k]), counter, search.TAPE_WORDS) for k in range(B)])
        assert numpy.array_equal(tape.cpu().numpy().view(numpy.uint32), want_tape)
        assert engine.draw_counter == 0          # an explicit counter leaves the engine's own alone
    # the engine's own counter: used, then incremented
    a = engine.run(obs, legal, to_play, True, None, temperature=1.0)
    b = engine.run(obs, legal, to_play, True, None, temperature=1.0)
    again = engine.run(obs, legal, to_play, True, None, counter=0, temperature=1.0)
    assert engine.draw_counter == 2
    assert numpy.array_equal(a.visit_counts, again.visit_counts) and numpy.array_equal(a.actions, again.actions)
    assert not numpy.array_equal(bits(a.root_values), bits(b.root_values))


def check_engine_continued(backend):
    """continue_search and run_from_trees with rngs=None against the same calls fed the restated noise and tape."""
    from mzx import search

    B = 4
    cfg, model = _net(backend, "fc")
    A = len(cfg.action_space)
    obs, legal, to_play = _move_inputs(cfg, B, 6)
    streams = numpy.array([5, 1, 30, 8], numpy.int32)

    class Fed:
        """A RandomState stand-in whose dirichlet / randint hand out the restated draws of one (stream, counter)."""

        def __init__(self, stream, counter, alpha):
            self.stream, self.counter, self.alpha = stream, counter, alpha

        def dirichlet(self, alphas):
            n = len(alphas)
            return noise_row(SEED, self.stream, self.counter, n, n, self.alpha, Margins())

        def randint(self, lo, hi, size, dtype):
            return tape_row(SEED, self.stream, self.counter, size)

        def get_state(self):
            return None

        def set_state(self, state):
            pass

    def engines():
        out = []
        for flag in (True, False):
            e = search.BatchedMCTS(cfg, model, B, max_carried_nodes=40, device_draws=flag)
            e.draw_seed = SEED
            rngs = [numpy.random.RandomState(70 + i) for i in range(B)]
            first = e.run(obs, legal, to_play, True, rngs)
            out.append((e, first))
        return out

    (dev, first_d), (host, first_h) = engines()
    assert numpy.array_equal(first_d.visit_counts, first_h.visit_counts)
    picks = first_d.visit_counts.argmax(1).astype(numpy.int32)
    picks[1] = -1
    counter = BIG_COUNTER + 3
    got = dev.continue_search(picks, to_play, True, None, streams=streams, counter=counter)
    want = host.continue_search(picks, to_play, True, [Fed(int(s), counter, cfg.root_dirichlet_alpha) for s in streams])
    for name in ("visit_counts", "max_tree_depth", "tape_used", "sum_depth"):
        assert numpy.array_equal(getattr(got, name), getattr(want, name)), name
    assert numpy.array_equal(bits(got.root_values), bits(want.root_values))
    assert got.visit_counts.sum() > first_d.visit_counts.sum() - B * cfg.num_simulations
    # the default streams and the engine's own counter
    dev.draw_counter = 11
    got2 = dev.continue_search([-1] * B, to_play, True)
    want2 = host.continue_search([-1] * B, to_play, True, [Fed(i, 11, cfg.root_dirichlet_alpha) for i in range(B)])
    assert dev.draw_counter == 12
    assert numpy.array_equal(got2.visit_counts, want2.visit_counts) and numpy.array_equal(bits(got2.root_values), bits(want2.root_values))
    # run_from_trees: graphs exported by a per-operator engine, searched again both ways
    trees = []
    for flag in (True, False):
        e = search.BatchedMCTS(cfg, model, B, mode=0, max_carried_nodes=40, device_draws=flag)
        e.draw_seed = SEED
        res = e.run(obs, legal, to_play, True, [numpy.random.RandomState(70 + i) for i in range(B)])
        t = e.export_trees(B)
        roots = [e.node_graph(B, i, res.legal_actions[i], _trees=t) for i in range(B)]
        trees.append((e, roots))
    (dev, roots_d), (host, roots_h) = trees
    got3 = dev.run_from_trees(roots_d, to_play, True, None, streams=streams, counter=5)
    want3 = host.run_from_trees(roots_h, to_play, True, [Fed(int(s), 5, cfg.root_dirichlet_alpha) for s in streams])
    assert numpy.array_equal(got3.visit_counts, want3.visit_counts) and numpy.array_equal(bits(got3.root_values), bits(want3.root_values))
    assert [r.visit_count for r in roots_d] == [r.visit_count for r in roots_h]
    try:
        host.continue_search([-1] * B, to_play, True, None)
    except ValueError as e:
        assert "device draws" in str(e)
    else:
        raise AssertionError("rngs=None accepted without device draws")


def _shard(backend, Game, cfg, weights, B, seed, native, pipeline):
    import copy

    from mzx import self_play

    c = copy.copy(cfg)
    c.native_rounds, c.self_play_pipeline, c.device_draws = native, pipeline, True
    return self_play.SelfPlay({"weights": weights}, Game, c, seed, num_games=B, _backend=backend)


def _play(shard, calls):
    out, slots = [], []
    for temperature, kwargs in calls:
        out += shard.play_rounds(temperature, shard.config.temperature_threshold, **kwargs)
        slots += shard.finished_slots
    return out, slots


def _same_games(a, b):
    from test_selfplay_refill import _same

    (ga, sa), (gb, sb) = a, b
    assert sa == sb and len(ga) == len(gb) and len(ga) > 0
    for k, (x, y) in enumerate(zip(ga, gb)):
        _same(x, y, (k, sa[k]))


def check_selfplay_rounds(backend, zero_weights=False):
    """play_rounds of a native tic-tac-toe shard (5 slots, 2 slot groups, slots restart) with the flag on: the library's
    round loop against the Python loop, game for game and field for field; successive games of a slot differ; a saved and
    restored draw_counter continues the same games.  ``zero_weights``: TAPE_WORDS lowered to 4 on a network with equal priors
    -- every search exhausts its tape and takes the retry path, in both loops."""
    from mzx import configs, games, models, search, synthetic

    if zero_weights:
        old = search.TAPE_WORDS
        search.TAPE_WORDS = 4
        try:
            return _selfplay_rounds(backend, True)
        finally:
            search.TAPE_WORDS = old
    return _selfplay_rounds(backend, False)


def _selfplay_rounds(backend, zero_weights):
    from mzx import configs, games, models, synthetic

    games.NativeBatchedGame.backend = backend
    if zero_weights:
        cfg = configs.cartpole(num_simulations=25, max_moves=4)
        Native = games.make_native_synthetic_game(cfg.observation_shape, len(cfg.action_space), 1)
        Python = Native
        weights = {k: torch.zeros_like(v) if v.dtype.is_floating_point else v
                   for k, v in models.MuZeroNetwork(cfg, _backend=backend).state_dict().items()}
        calls = [(1.0, {}), (0.5, {})]
    else:
        cfg = configs.tictactoe(num_simulations=8, temperature_threshold=4)
        Native, Python = games.NATIVE["tictactoe"], games.BATCHED["tictactoe"]
        weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 21)
        calls = [(1.0, dict(min_games=3)), (0.5, dict(max_rounds=4, min_games=1 << 60)), (0.25, dict(min_games=14))]
    B, seed = 5, 7
    runs = {}
    for name, Game, native in (("native", Native, True), ("python", Native, False)) + (() if zero_weights else (("plain", Python, False),)):
        shard = _shard(backend, Game, cfg, weights, B, seed, native, True)
        before = [shard.bank.get_state(k) for k in range(B)]
        runs[name] = _play(shard, calls)
        assert len(shard._live["groups"]) == 2 and bool(shard._live.get("native")) == native
        runs[name + "_counter"] = shard.draw_counter
        for x, y in zip(before, [shard.bank.get_state(k) for k in range(B)]):      # no host stream was read or advanced
            assert x[2] == y[2] and (x[1] == y[1]).all()
        if zero_weights and native:
            assert shard.stats["native_phase_seconds"][4] > 0, "the retry callback ran"
        if zero_weights and not native:
            assert sum(g.engine.tape_retries for g in shard._live["groups"]) > 0, "the Python loop searched trees again"
        shard.close_game()
    _same_games(runs["native"], runs["python"])
    if not zero_weights:
        _same_games(runs["native"], runs["plain"])
    assert runs["native_counter"] == runs["python_counter"] > 0
    out, slots = runs["native"]
    if zero_weights:
        return
    # the two games a slot plays in succession differ (the counter goes on; a slot is no fixed sequence)
    for s in set(slots):
        mine = [g for g, who in zip(out, slots) if who == s]
        assert len(mine) >= 2, "every slot restarts in this run"
        assert (list(mine[0].action_history) != list(mine[1].action_history)
                or [list(v) for v in mine[0].child_visits] != [list(v) for v in mine[1].child_visits])
    # draw_counter: saved, clobbered, restored between two calls -> the same games; left clobbered -> other games
    for native in (True, False):
        shard = _shard(backend, Native, cfg, weights, B, seed, native, True)
        first = _play(shard, calls[:1])
        saved = shard.draw_counter
        shard.draw_counter = saved + 1000
        assert shard.draw_counter == saved + 1000
        shard.draw_counter = saved
        rest = _play(shard, calls[1:])
        shard.close_game()
        _same_games((first[0] + rest[0], first[1] + rest[1]), runs["native"])
        shard = _shard(backend, Native, cfg, weights, B, seed, native, True)
        _play(shard, calls[:1])
        shard.draw_counter = saved + 1000
        other = _play(shard, calls[1:])
        shard.close_game()
        theirs = runs["native"][0][len(first[0]):]
        assert any(list(x.action_history) != list(y.action_history) for x, y in zip(other[0], theirs))
    # a start counter set before the first round is the first search's
    shard = _shard(backend, Native, cfg, weights, B, seed, True, True)
    shard.draw_counter = BIG_COUNTER
    _play(shard, calls[:1])
    assert shard.draw_counter > BIG_COUNTER
    shard.close_game()


def check_actor_seed(backend):
    """The actor's seed keys the draws: two shards that differ only in it (same configuration, same config.seed, a
    deterministic game) play different games, the same seed plays the same games again, in the library's loop and in the
    Python loop; ranks of a job (seed, seed + games) share no game either."""
    from mzx import configs, games, models, synthetic

    games.NativeBatchedGame.backend = backend
    cfg = configs.tictactoe(num_simulations=8)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 21)
    B, calls = 5, [(1.0, dict(min_games=10))]

    def play(seed, native):
        shard = _shard(backend, games.NATIVE["tictactoe"], cfg, weights, B, seed, native, True)
        assert shard.draw_seed == seed
        out = _play(shard, calls)
        assert all(g.engine.draw_seed == seed for g in shard._live["groups"])
        shard.close_game()
        return out

    moves = lambda run: [tuple(g.action_history) for g in run[0]]
    a, again, python = play(7, True), play(7, True), play(7, False)
    _same_games(a, again)
    _same_games(a, python)
    for other_seed in (8, 7 + B, 1007):
        b = play(other_seed, True)
        _same_games(b, play(other_seed, False))
        assert moves(a) != moves(b), other_seed
        assert sum(x == y for x, y in zip(moves(a), moves(b))) < len(moves(a)) // 2, "mostly other games"
    # the engine on its own: draw_seed is part of the key
    from mzx import search

    cfg2, model = _net(backend, "fc")
    obs, legal, to_play = _move_inputs(cfg2, 4, 2)
    res = []
    for seed in (3, 3, 4):
        engine = search.BatchedMCTS(cfg2, model, 4, device_draws=True)
        assert engine.draw_seed == int(cfg2.seed)
        engine.draw_seed = seed
        res.append(engine.run(obs, legal, to_play, True, None, temperature=1.0))
    assert numpy.array_equal(bits(res[0].root_values), bits(res[1].root_values))
    assert not numpy.array_equal(bits(res[0].root_values), bits(res[2].root_values))


def check_selfplay_lockstep(backend):
    """play_games (lock-step, thinning batch) with the flag on: deterministic, and no stream of the bank moves."""
    from mzx import configs, games, models, synthetic

    cfg = configs.tictactoe(num_simulations=8)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg, _backend=backend).state_dict(), 21)
    outs = []
    for _ in range(2):
        shard = _shard(backend, games.BATCHED["tictactoe"], cfg, weights, 5, 7, False, False)
        before = [shard.bank.get_state(s) for s in range(5)]
        outs.append(shard.play_games(1.0, None, False, "self", 0))
        after = [shard.bank.get_state(s) for s in range(5)]
        for x, y in zip(before, after):
            assert x[2] == y[2] and (x[1] == y[1]).all()
        assert shard.draw_counter == max(len(g.action_history) - 1 for g in outs[-1])
        shard.close_game()
    _same_games((outs[0], list(range(5))), (outs[1], list(range(5))))


def check_move_refusals(backend):
    """The fused move's own refusals, and the SelfPlay paths that keep numpy streams."""
    from mzx import configs, models, search, self_play, synthetic

    cfg, model = _net(backend, "fc")
    B, A = 3, len(cfg.action_space)
    obs, legal, to_play = _move_inputs(cfg, B, 1)
    engine = search.BatchedMCTS(cfg, model, B, device_draws=True)
    engine.run(obs, legal, to_play, True, None, temperature=1.0)
    lib = backend.lib
    st = engine._staging(B, search.TAPE_WORDS, obs.size // B, True, device_draws=True)
    mv = st["move"]
    d = _lib.Draws(seed=1, counter=1, num_games=B, action_space_size=A, tape_words=search.TAPE_WORDS, dirichlet_alpha=0.25)
    n_legal = numpy.zeros(B, numpy.int32)
    arena = engine.arena(B)

    def call(move, draws_):
        return lib.mzx_selfplay_move_device(engine.handle(B), ctypes.byref(move), ctypes.byref(draws_), None, n_legal.ctypes.data,
                                            backend.ptr(arena), arena.numel(), backend.stream())

    assert call(mv, d) == 0
    saved = mv.io.d_noise
    mv.io.d_noise = None                      # add_exploration_noise with d_noise NULL
    assert call(mv, d) == -1 and b"d_noise" in lib.mzx_last_error()
    mv.io.d_noise = saved
    mv.add_exploration_noise = 0              # ... and noise given without it
    assert call(mv, d) == -1 and b"d_noise" in lib.mzx_last_error()
    mv.add_exploration_noise = 1
    d.tape_words = 0
    assert call(mv, d) == -1
    d.tape_words = search.TAPE_WORDS
    saved = mv.io.d_visit_counts
    mv.io.d_visit_counts = None               # null outputs
    assert call(mv, d) == -1
    mv.io.d_visit_counts = saved
    bad = legal.copy()
    bad[1] = -1
    try:
        engine.run(obs, bad, to_play, True, None)
    except AssertionError as e:
        assert "should not be an empty array" in str(e)
    else:
        raise AssertionError("an empty legal row was accepted")
    try:
        engine.run(obs, legal, to_play, True, [numpy.random.RandomState(1)] * B, temperature=1.0)
    except ValueError as e:
        assert "device draws" in str(e)
    else:
        raise AssertionError("temperature= accepted on host streams")
    # SelfPlay: the per-object paths keep numpy streams and refuse the flag
    import copy

    c = copy.copy(cfg)
    c.device_draws = True
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(c, _backend=backend).state_dict(), 2)
    Game = synthetic.make_synthetic_game(c.observation_shape, A, 1)
    for num_games, calls in ((1, [lambda sp: sp.play_game(1.0, None, False, "self", 0)]),
                             (3, [lambda sp: sp.play_games(1.0, None, False, "self", 0), lambda sp: sp.play_rounds(1.0, None),
                                  lambda sp: sp.play_games(1.0, None, False, "random", 0)])):
        sp = self_play.SelfPlay({"weights": weights}, Game, c, 3, num_games=num_games, _backend=backend)
        for fn in calls:
            try:
                fn(sp)
            except NotImplementedError as e:
                assert "device_draws" in str(e)
            else:
                raise AssertionError("a numpy-stream path ran with config.device_draws")
        sp.close_game()
