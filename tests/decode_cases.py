"""
Shared by the support-decode tests (tests/test_decode_edges.py on the serial build, tests/test_gpu_decode_edges.py on the
device): logit rows for support_to_scalar -- soft-max over 2 * support + 1 bins, expectation, inverse value transform
sign(x) * (((sqrt(1 + 0.004 (|x| + 1.001)) - 1) / 0.002)^2 - 1) -- and the two references they are held to.

  * exact_rows: rows whose mass sits on 1, 2 or 4 equally weighted bins, every other bin far below.  The soft-max is then
    exactly 1 / n per bin (exp gives 1 and 0, the sum is a power of two, whose reciprocal is exact), and the expectation x
    is an exact multiple of 1/4 in float32 in ANY summation order.  Only the transform's IEEE operations remain, so every
    decode must give restate(x) bit for bit: the float32 op-by-op restatement of support_inverse_transform
    (csrc/mzx_tree.h) in numpy.  x = 0 gives sign(0) * (tiny negative) = -0.0.
  * dense_rows: six families of rows with mass everywhere (or on two unequal bins), held to a tolerance.  The gate is
    computed from the reference side only: 4 x max(e_ref, e_transform), where e_ref is the error of the plain-torch
    float32 expression (trainer_loss_cases.torch_support_to_scalar) against binary64 on the same rows and e_transform the
    restatement's own error against binary64 on the support's exact rows, both relative to max(1, |truth|).  4 is the
    yardstick factor of fc_train_cases / trainer_loss_cases.  No sign is asserted on a dense row:
    near x = 0 the transform returns a tiny value whose sign is decided by the last bit of the expectation.
  * edge_rows: at most ten rows per support for the whole-search kernels, whose heads are made to return them.

Everything is rebuilt from seeds (numpy.random.RandomState, float32 only).
"""
import functools

import numpy
import torch

import trainer_loss_cases

SUPPORTS = (0, 1, 7, 8, 10, 15, 16, 31, 32, 300)
OFF_LEVELS = (-200.0, -1e30)      # exp(off - level) underflows to 0 in float32 for every level in [-30, 30]
ROW_CAP = 1500                    # exact rows per support, both copies together (about)
FOUR_BIN_ROWS = 128
DENSE_ROWS = 256
YARDSTICK_FACTOR = 4
FAMILIES = ("n3", "n20", "equal", "adjacent", "mirror", "nearzero")

f32 = numpy.float32


def bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view({4: numpy.uint32, 8: numpy.uint64}[a.dtype.itemsize])


def restate(x):
    """support_inverse_transform (csrc/mzx_tree.h) op by op in float32: |x| + 1, + 0.001, 0.004 *, 1 +, sqrt, - 1,
    / 0.002, t * t - 1, sign(x) *.  numpy rounds every operation of a float32 array to float32."""
    x = numpy.asarray(x, f32)
    t = numpy.abs(x) + f32(1.0)
    t = t + f32(0.001)
    t = f32(0.004) * t
    t = f32(1.0) + t
    t = numpy.sqrt(t)
    t = (t - f32(1.0)) / f32(0.002)
    t = t * t - f32(1.0)
    out = numpy.sign(x) * t
    assert out.dtype == f32
    return out


def transform64(x):
    x = numpy.asarray(x, numpy.float64)
    return numpy.sign(x) * (((numpy.sqrt(1 + 0.004 * (numpy.abs(x) + 1.001)) - 1) / 0.002) ** 2 - 1)


def truth(rows, S):
    """binary64 soft-max, expectation and transform of float32 rows [n, 2 S + 1] -> float64 [n]."""
    z = numpy.asarray(rows, numpy.float64)
    assert z.ndim == 2 and z.shape[1] == 2 * S + 1
    e = numpy.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    return transform64((p * numpy.arange(-S, S + 1, dtype=numpy.float64)).sum(1))


def _den(t):
    return numpy.maximum(1.0, numpy.abs(t))


def rel_error(got, want):
    """max |got - want| / max(1, |want|), `want` in binary64."""
    got = numpy.asarray(got, numpy.float64).reshape(-1)
    assert got.shape == want.shape
    return float(numpy.max(numpy.abs(got - want) / _den(want))) if got.size else 0.0


# ---------------------------------------------------------------------------------------------------------- exact rows

def _on_sets(S, seed):
    """[(bins, x)]: the bins that carry the mass of a row and its exact expectation."""
    F = 2 * S + 1
    rs = numpy.random.RandomState(seed)
    sets = [((i,), float(i - S)) for i in range(F)]                                  # every one-hot row
    sets += [((i, i + 1), i - S + 0.5) for i in range(F - 1)]                        # every adjacent pair: the half grid
    for k in sorted(set([1, 2, S // 2, S - 1, S]) & set(range(1, S + 1))):           # x = 0 by a symmetric pair ...
        sets.append(((S - k, S + k), 0.0))
    sets += [((S,), 0.0)] * 3                                                        # ... and by the centre bin
    if F >= 4:
        for _ in range(FOUR_BIN_ROWS):
            b = tuple(sorted(rs.choice(F, size=4, replace=False).tolist()))
            sets.append((b, sum(i - S for i in b) / 4.0))
        sets.append(((S - 2, S, S + 1, S + 2), 0.25))
    return sets


@functools.lru_cache(maxsize=None)
def _exact(S, seed):
    F = 2 * S + 1
    sets = _on_sets(S, seed)
    rs = numpy.random.RandomState(seed + 1)
    keep = numpy.arange(len(sets))
    half = ROW_CAP // 2
    if len(sets) > half:      # the first and last one-hot, +-0.5, +-1 and every x = 0 row stay; the rest is a seeded sample
        must = [i for i, (b, x) in enumerate(sets) if x == 0.0 or abs(x) in (0.5, 1.0) or (len(b) == 1 and abs(x) == S)]
        rest = numpy.setdiff1d(keep, must)
        keep = numpy.sort(numpy.concatenate([must, rs.choice(rest, size=half - len(must), replace=False)]).astype(numpy.int64))
    level = rs.uniform(-30.0, 30.0, size=len(sets)).astype(f32)
    rows, xs = [], []
    for off in OFF_LEVELS:
        block = numpy.full((len(keep), F), f32(off), f32)
        for r, k in enumerate(keep):
            block[r, list(sets[k][0])] = level[k]
        rows.append(block)
        xs.append(numpy.asarray([sets[k][1] for k in keep], f32))
    rows, xs = numpy.concatenate(rows), numpy.concatenate(xs)
    assert (xs * 4 == numpy.round(xs * 4)).all() and (numpy.abs(xs) <= S).all()
    rows.setflags(write=False), xs.setflags(write=False)
    return rows, xs


def exact_rows(S, seed=0):
    """(rows float32 [n, 2 S + 1], x float32 [n]): the first n / 2 rows have their off bins at -200, the second half is the
    same set with the off bins at -1e30.  Computed once per process and left unchanged (read-only arrays)."""
    return _exact(S, 7000 + seed)


def finite_half(S, seed=0):
    """The copy of exact_rows with the off bins at -200 (a cross entropy of such a row stays finite)."""
    rows, xs = exact_rows(S, seed)
    return rows[: len(rows) // 2], xs[: len(xs) // 2]


# ---------------------------------------------------------------------------------------------------------- dense rows

@functools.lru_cache(maxsize=None)
def _dense(S, seed):
    F, n = 2 * S + 1, DENSE_ROWS
    rs = numpy.random.RandomState(seed)
    out = {}
    out["n3"] = (rs.standard_normal((n, F)) * 3).astype(f32)
    out["n20"] = (rs.standard_normal((n, F)) * 20).astype(f32)
    out["equal"] = numpy.repeat(rs.uniform(-30, 30, size=(n, 1)).astype(f32), F, 1)
    half = (rs.standard_normal((n, S + 1)) * 3).astype(f32)
    out["mirror"] = numpy.concatenate([half, half[:, :S][:, ::-1]], 1)
    if F >= 2:
        adj = numpy.full((n, F), f32(OFF_LEVELS[0]), f32)
        near = adj.copy()
        first = rs.randint(0, F - 1, size=n)
        first[:4] = (0, F - 2, max(S - 1, 0), min(S, F - 2))          # both ends of the support, either side of zero
        gap = rs.uniform(-20.0, 0.0, size=n).astype(f32)
        side = rs.randint(0, 2, size=n)
        for r in range(n):
            adj[r, first[r] + side[r]] = 0.0
            adj[r, first[r] + 1 - side[r]] = gap[r]
        out["adjacent"] = adj
        level = rs.uniform(-18.0, -6.0, size=n).astype(f32)
        where = S + 2 * rs.randint(0, 2, size=n) - 1
        near[:, S] = 0.0
        near[numpy.arange(n), where] = level
        out["nearzero"] = near
    for a in out.values():
        assert a.dtype == f32 and a.shape == (n, F)
        a.setflags(write=False)
    return out


def dense_rows(S, seed=0):
    """{family: float32 [256, 2 S + 1]}; a support of one bin has no two-bin family.  Read-only, computed once."""
    return _dense(S, 9000 + seed)


def dense_block(S, seed=0):
    """All dense rows of a support as one array (one launch), with the slice of every family."""
    fam = dense_rows(S, seed)
    names = [f for f in FAMILIES if f in fam]
    rows = numpy.concatenate([fam[f] for f in names])
    return rows, {f: slice(i * DENSE_ROWS, (i + 1) * DENSE_ROWS) for i, f in enumerate(names)}


# ---------------------------------------------------------------------------------------------------------- edge rows

@functools.lru_cache(maxsize=None)
def _edges(S):
    F = 2 * S + 1
    rs = numpy.random.RandomState(4100 + S)
    rows, xs, names = [], [], []

    def on(name, bins, level=0.0):
        row = numpy.full(F, f32(OFF_LEVELS[0]), f32)
        row[[b + S for b in bins]] = f32(level)
        rows.append(row), xs.append(f32(sum(bins) / len(bins))), names.append(name)

    seen = set()
    for name, b, level in (("one-hot -S", -S, 3.0), ("one-hot -1", -1, -7.5), ("one-hot 0", 0, 11.0), ("one-hot +1", 1, 0.0),
                           ("one-hot +S", S, -30.0)):
        if abs(b) <= S and b not in seen:      # (supports 0 and 1: -S and -1, +1 and +S fall together)
            seen.add(b)
            on(name, [b], level)
    if S >= 1:
        on("pair +0.5", [0, 1], 2.0)
        on("pair -0.5", [-1, 0], -4.0)
    if S >= 2:
        on("four bins 0.25", [-2, 0, 1, 2], 5.0)
    for name, scale in (("N(0,3)", 3), ("N(0,20)", 20)):
        rows.append((rs.standard_normal(F) * scale).astype(f32)), xs.append(None), names.append(name)
    rows = numpy.stack(rows)
    rows.setflags(write=False)
    return rows, tuple(xs), tuple(names)


def edge_rows(S):
    """(rows float32 [n <= 10, 2 S + 1], x: the exact expectation of a row or None for a dense row, names); ten rows from
    support 2 on, five at support 1 and three at support 0, whose bins do not hold more."""
    return _edges(S)


# ---------------------------------------------------------------------------------------------------------- the gate

def torch_decode(rows, S):
    """The plain-torch float32 expression, as the oracle evaluates it: the error yardstick (NOT a bit reference: torch's
    vectorised path rounds one step differently on some rows, see test_decode_edges.test_reference_meets_the_gate)."""
    return trainer_loss_cases.torch_support_to_scalar(torch.from_numpy(numpy.array(rows)), S).numpy().reshape(-1)


@functools.lru_cache(maxsize=None)
def e_transform(S):
    """The restatement's own error on the support's exact rows: max |restate(x) - truth| / den."""
    rows, xs = exact_rows(S)
    return rel_error(restate(xs), truth(rows, S))


@functools.lru_cache(maxsize=None)
def _yardstick(S):
    rows, where = dense_block(S)
    want = truth(rows, S)
    ref = torch_decode(rows, S)
    return {f: rel_error(ref[s], want[s]) for f, s in where.items()}


def yardstick(S):
    """{family: e_ref = max |torch float32 - truth| / den} on dense_rows(S)."""
    return dict(_yardstick(S))


def gate(S, family):
    return YARDSTICK_FACTOR * max(_yardstick(S)[family], e_transform(S))


def check_dense(got, S, label, report=print):
    """`got`: a decode of dense_block(S)[0].  Finite everywhere, and per family within the gate; every figure is printed
    before it is asserted.  Returns the worst (error, gate, family)."""
    rows, where = dense_block(S)
    want = truth(rows, S)
    got = numpy.asarray(got).reshape(-1)
    assert numpy.isfinite(got).all(), label
    worst, failures = (0.0, 0.0, None), []
    for f, s in where.items():
        err, g = rel_error(got[s], want[s]), gate(S, f)
        report(f"decode_edges {label} support {S} {f}: error {err:.3e} e_ref {_yardstick(S)[f]:.3e} "
               f"e_transform {e_transform(S):.3e} gate {g:.3e}")
        if not err <= g:
            failures.append((f, err, g))
        if worst[2] is None or err - g > worst[0] - worst[1]:
            worst = (err, g, f)
    assert not failures, (label, S, failures)
    return worst


def check_exact(got, S, label, report=print):
    """`got`: a decode of exact_rows(S)[0].  restate(x) bit for bit, hence -0.0 wherever x = 0."""
    rows, xs = exact_rows(S)
    got = numpy.asarray(got, f32).reshape(-1)
    want = restate(xs)
    assert numpy.isfinite(got).all(), label
    differ = numpy.flatnonzero(bits(got) != bits(want))
    report(f"decode_edges {label} support {S} exact: {len(xs)} rows, {numpy.unique(xs).size} distinct x, "
           f"{differ.size} differ from the restatement in bits")
    assert differ.size == 0, (label, S, [(float(xs[i]), float(got[i]), float(want[i])) for i in differ[:8]])
    zero = xs == 0
    assert zero.any() and (bits(got[zero]) == 0x80000000).all(), (label, S, "x = 0 must decode to -0.0")


# ---------------------------------------------------------------------------------------------------------- the entries

def _up(be, a):
    return torch.from_numpy(numpy.array(a)).to(be.device)      # (a copy: the shared rows are read-only)


def decode(be, rows, S):
    """mzx_support_to_scalar of float32 rows -> float32 [n]: one launch."""
    logits = _up(be, rows)
    out = be.empty((logits.shape[0],), torch.float32)
    be.lib.check(be.lib.mzx_support_to_scalar(be.ptr(logits), logits.shape[0], S, be.ptr(out), be.stream()))
    return out.cpu().numpy()


def replay_decode(be, rows, S):
    """mzx_replay_reanalyse_write (the replay / reanalyse value decode) of the rows, sample n written to pool row n:
    (float32 [n], the float64 pool column [n])."""
    n = len(rows)
    logits = _up(be, rows)
    base, pos = _up(be, numpy.arange(n, dtype=numpy.int64)), _up(be, numpy.zeros(n, numpy.int32))
    out = be.zeros((n,), torch.float32)
    column = _up(be, numpy.full(n, numpy.nan, numpy.float64))
    be.lib.check(be.lib.mzx_replay_reanalyse_write(be.ptr(logits), n, S, be.ptr(base), be.ptr(pos), be.ptr(out), be.ptr(column),
                                                   be.stream()))
    return out.cpu().numpy(), column.cpu().numpy()


def trainer_priorities(be, rows, S, steps=3):
    """mzx_trainer_loss with PER_alpha = 1 and value targets of 0, the rows as the value logits of a steps x B batch (the
    last step padded with row 0): the priorities [n] in the order of the rows, and the four losses."""
    n, F = rows.shape
    B = -(-n // steps)
    value = numpy.concatenate([rows, numpy.repeat(rows[:1], steps * B - n, 0)]).reshape(steps, B, F)
    A = 2
    x = dict(value=value, reward=numpy.zeros_like(value), policy=numpy.zeros((steps, B, A), f32),
             target_value=numpy.zeros((B, steps), f32), target_reward=numpy.zeros((B, steps), f32),
             target_policy=numpy.full((B, steps, A), f32(0.5), f32), gradient_scale=numpy.ones((B, steps), f32), weight=None)
    case = dict(B=B, steps=steps, S=S, A=A, vlw=0.25, alpha=1.0)
    got = trainer_loss_cases.run_abi(be, case, x, grads=False)
    losses = numpy.asarray([got[k] for k in ("loss", "value_loss", "reward_loss", "policy_loss")])
    return numpy.ascontiguousarray(got["priorities"].T).reshape(-1)[:n], losses


def check_entries(be, S, report=print):
    """Part 2 of one support on a backend: mzx_support_to_scalar against the two references, then the replay decode and the
    trainer's priorities against mzx_support_to_scalar, bit for bit on every row.  One launch per entry and block of rows."""
    exact, xs = exact_rows(S)
    dense, _ = dense_block(S)
    got_exact, got_dense = decode(be, exact, S), decode(be, dense, S)
    check_exact(got_exact, S, "mzx_support_to_scalar", report)
    worst = check_dense(got_dense, S, "mzx_support_to_scalar", report)
    every = numpy.concatenate([exact, dense])
    want = numpy.concatenate([got_exact, got_dense])
    out, column = replay_decode(be, every, S)
    assert numpy.array_equal(bits(out), bits(want)), ("replay decode", S, numpy.flatnonzero(bits(out) != bits(want))[:8])
    assert numpy.array_equal(bits(column), bits(want.astype(numpy.float64))), ("replay decode, pool column", S)
    finite, _ = finite_half(S)
    rows = numpy.concatenate([finite, dense])
    pred = numpy.concatenate([got_exact[: len(finite)], got_dense])
    prio, losses = trainer_priorities(be, rows, S)
    assert numpy.isfinite(losses).all() and numpy.isfinite(prio).all(), ("trainer loss", S, losses)
    assert numpy.array_equal(bits(prio), bits(numpy.abs(pred))), ("priorities", S, numpy.flatnonzero(bits(prio) != bits(numpy.abs(pred)))[:8])
    report(f"decode_edges entries support {S}: {len(every)} rows through mzx_support_to_scalar and the replay decode, "
           f"{len(rows)} through mzx_trainer_loss | worst dense error {worst[0]:.3e} ({worst[2]}) against its gate {worst[1]:.3e}")
    return worst


# ---------------------------------------------------------------------------------------------------------- searches

SEARCH_TREES, SEARCH_SIMULATIONS = 4, 3


def heads_network(make, support, k, backend=None, net_mode=None, actions=None):
    """(config, network): `make()`'s network at `support` with one player and three simulations, every tensor zero, the
    value head returning edge row k and the reward head edge row (k + 3) % rows at every node."""
    import tree_edge_cases
    from mzx import models

    cfg = make()
    cfg.support_size = support
    if actions is not None:
        cfg.action_space = list(range(actions))
    cfg.players = [0]
    cfg.num_simulations = SEARCH_SIMULATIONS
    rows, _, _ = edge_rows(support)
    net = models.MuZeroNetwork(cfg) if backend is None else models.MuZeroNetwork(cfg, _backend=backend)
    A = len(cfg.action_space)
    net.set_weights(tree_edge_cases.network_weights(net, "heads", A, heads=(rows[k], rows[(k + 3) % len(rows)])))
    if net_mode is not None:
        net.set_mode(net_mode)
    return cfg, net


def check_search(be, make, support, mode, tuning, route, want_kernel, net_mode=None, actions=None, backend_arg=False,
                 report=print):
    """One search per edge row of `support` on a route: the kernel that ran, by name (`want_kernel`: a predicate), and every
    decoded number a search exports -- root predicted values, rewards of every node but the root, the value of every node
    visited once, the root's reward -0.0 -- with the bits of mzx_support_to_scalar, and of restate(x) on the exact rows."""
    import tree_edge_cases
    from mzx import self_play, synthetic

    rows, xs, names = edge_rows(support)
    decoded = decode(be, rows, support)
    assert numpy.isfinite(decoded).all()
    B, S = SEARCH_TREES, SEARCH_SIMULATIONS
    worst, kernel = 0.0, None
    want = truth(rows, support)
    for k in range(len(rows)):
        kr = (k + 3) % len(rows)
        cfg, net = heads_network(make, support, k, backend=be if backend_arg else None, net_mode=net_mode, actions=actions)
        A = len(cfg.action_space)
        obs = synthetic.observations(B, net.input_shape, seed=6)
        legal = tree_edge_cases.ragged_legal(A, B, 7)
        with be.lib.tuning(**tuning):
            engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
            res = engine.run(list(obs), legal, [0] * B, False, [numpy.random.RandomState(500 + i) for i in range(B)])
            kernel = engine.kernel_name(B)
            trees = engine.export_trees(B)
        label = (route, support, names[k], names[kr], kernel)
        assert want_kernel(kernel), label
        assert (res.flags == 0).all() and (res.visit_counts.sum(1) == S).all(), label
        v64, r64 = numpy.float64(decoded[k]), numpy.float64(decoded[kr])
        for b in range(B):
            n = int(trees["n_nodes"][b])
            assert n == S + 1, label
            assert bits(res.root_predicted_values[b: b + 1])[0] == bits(v64.reshape(1))[0], label + ("root value", b)
            assert numpy.array_equal(bits(trees["reward"][b, 1:n]), numpy.repeat(bits(r64.reshape(1)), n - 1)), label + ("reward", b)
            once = numpy.flatnonzero(trees["visit"][b, :n] == 1)
            once = once[once > 0]
            assert once.size, label
            # (0.0 + v: the value itself, but for v = -0.0, whose sum is +0.0 -- equality of numbers, which for every
            # other v is equality of bits)
            assert (trees["value_sum"][b, once] == v64).all(), label + ("leaf", b)
            assert bits(trees["reward"][b, :1])[0] == 0x8000000000000000, label + ("root reward must be -0.0", b)
        for i, got in ((k, decoded[k]), (kr, decoded[kr])):
            if xs[i] is not None:
                assert bits(numpy.asarray([got], f32))[0] == bits(restate([xs[i]]))[0], label + ("restatement", names[i])
            worst = max(worst, rel_error([got], want[i: i + 1]))
    g = YARDSTICK_FACTOR * max(rel_error(torch_decode(rows, support), want), e_transform(support))
    report(f"decode_edges search {route}: support {support} actions {A} kernel {kernel.split(' between ')[-1]} | {len(rows)} searches x {B} trees x "
           f"{S} simulations, every decoded number with the bits of mzx_support_to_scalar | worst error {worst:.3e} gate {g:.3e}")
    assert worst <= g, (route, support, worst, g)
    return kernel
