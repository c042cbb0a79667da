"""
The write side of a simulation of fc2_search_kernel without exec masks ("Branch-free writes"):
back-propagation in which EVERY lane of a row stores a whole node record, its parent's {q, n, child} and the refreshed
prior scores of its node -- lanes at and beyond the leaf the leaf's own values again, the root lane and the lanes without
an inner node into a dead slot row in front of the tree's slots (only the MinMaxStats atomics keep their guard: duplicate
lanes on one address are served one after the other; 16-lane records have no dead row and keep the root lane's guard too);
a value chain whose steps 6 .. 1 run unguarded; the walk's last path entry and the leaf's child slots stored by the whole row; SmallNetCartpole's hidden state stored by sixteen lanes into eight floats
plus the next node's (or, for the last node, a dead tail behind the tree's hidden states).

The yardstick is the per-operator path (mode 0: one thread per tree, none of the above): every array of export_trees (node
and slot records, MinMaxStats, node counts) and every result, bit for bit, on both engines of the kernel (SmallNetCartpole,
mode 3; the same network on LdsNet, mode 7) at 1, 3, 5 and 17 trees -- a lone row, a partial wave, a wave plus a row, a
workgroup plus a row.  From three trees on a slab has neighbours (a dead-row or hidden-tail store that strays lands in the next
tree), at seventeen there is a second workgroup.  Every search here fills its node capacity: the last simulation expands
node NN - 1, and flags == 0 is asserted.

The weight cases and their preconditions are those of tests/test_gpu_fc2_lean_loop.py, run again here on purpose: they are
the cases that reach the new write side, and that file's yardstick cache is shared, so the per-operator searches run once.
They are values and rewards of both signs with one and two players, all-zero weights that tie at every level and back up
q = 0 from duplicate lanes, and a chain of at least 33 plies (three 16-level chunks, the loop's copy of the write side, the
hand-over behind its scalar branch, rows with no lane in the upper chunk).  New here: roots with ONE legal action (a slot row whose second slot is -inf and has to stay -inf through the
unconditional refresh), and the four- and sixteen-lane record instantiations at five trees.
"""
import numpy
import pytest
import torch

import test_gpu_continue_shapes as shapes
import test_gpu_fc2_lean_loop as lean
from mzx import _lib, configs, self_play, synthetic

pytestmark = pytest.mark.gpu

RESULT_KEYS = lean.RESULT_KEYS
_bits = lean._bits
_single = {}    # (players, B) -> inputs and the per-operator path's result, computed once and never changed


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _assert_equal(want, want_trees, res, trees, skip=()):
    for key in RESULT_KEYS:
        if key not in skip:
            assert numpy.array_equal(_bits(getattr(want, key)), _bits(getattr(res, key))), key
    assert set(trees) == set(want_trees)
    for key, w in want_trees.items():
        assert numpy.array_equal(_bits(trees[key]), _bits(w)), key
    assert (res.flags == 0).all()


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [3, 7], ids=["small", "lds"])
@pytest.mark.parametrize("case", sorted(lean.CASES))
def test_weight_cases(backend, case, mode, B):
    """One and two players, both signs / all ties / a chain of 33 plies and more (preconditions asserted by the yardstick)."""
    cfg, net, obs, legal, to_play, want, want_trees = lean._yardstick(case, B)
    res, trees, kernel = lean._search(cfg, net, mode, B, obs, legal, to_play)
    assert "fc2_search_kernel" in kernel, kernel
    _assert_equal(want, want_trees, res, trees)
    assert (trees["n_nodes"] == cfg.num_simulations + 1).all()
    assert (res.visit_counts.sum(1) == cfg.num_simulations).all()


def _single_action_yardstick(players, B):
    key = (len(players), B)
    if key not in _single:
        S = 16
        cfg = configs.cartpole(players=players, num_simulations=S)
        net = lean._weights(cfg, "signs")
        A = len(cfg.action_space)
        # every second tree (tree 0 included, so also at B = 1) has ONE legal action, alternately action 1 and action 0
        legal = [[(i // 2 + 1) % A] if i % 2 == 0 else list(cfg.action_space) for i in range(B)]
        to_play = [int(i % len(players)) for i in range(B)]
        obs = synthetic.observations(B, net.input_shape, seed=B + 7)
        res, trees, _ = lean._search(cfg, net, 0, B, obs, legal, to_play)
        assert (trees["n_nodes"] == S + 1).all() and (res.flags == 0).all()
        for i in range(0, B, 2):       # the precondition: a one-slot root that took every visit through its only action
            only = legal[i][0]
            assert res.visit_counts[i][only] == S and res.visit_counts[i].sum() == S
            assert sorted(trees["child"][i, 0]) == [-1, 1]
            assert res.max_tree_depth[i] >= 2
        _single[key] = (cfg, net, obs, legal, to_play, res, trees)
    return _single[key]


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [3, 7], ids=["small", "lds"])
@pytest.mark.parametrize("players", [[0], [0, 1]], ids=["one-player", "two-players"])
def test_single_action_roots(backend, players, mode, B):
    """nslots < AW at the root: its second slot's cached prior score is -inf and stays -inf through sixteen refreshes."""
    cfg, net, obs, legal, to_play, want, want_trees = _single_action_yardstick(players, B)
    res, trees, kernel = lean._search(cfg, net, mode, B, obs, legal, to_play)
    assert "fc2_search_kernel" in kernel, kernel
    _assert_equal(want, want_trees, res, trees)


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [3, 7], ids=["small", "lds"])
@pytest.mark.parametrize("players", [[0], [0, 1]], ids=["one-player", "two-players"])
def test_given_roots(backend, players, mode, B):
    """OVERRIDE: the caller's hidden states, priors and rewards (both signs and zero) replace initial_inference; one tree
    (tree 3, or tree 0 where there are fewer than four) has a single legal action."""
    S = 16
    one = 3 if B > 3 else 0
    cfg = configs.cartpole(players=players, num_simulations=S)
    net = lean._weights(cfg, "signs")
    rewards = [[0.75, -1.5, 0.0][i % 3] for i in range(B)]
    outs = []
    for m in (0, mode):
        roots = []
        state = numpy.random.RandomState(11)
        for i in range(B):
            root = self_play.Node(0)
            hidden = torch.as_tensor(state.rand(1, net.hidden_size).astype(numpy.float32))
            logits = torch.as_tensor(state.randn(1, len(cfg.action_space)).astype(numpy.float32))
            root.expand(cfg.action_space if i != one else [1], i % len(players), rewards[i], logits, hidden)
            roots.append(root)
        engine = self_play.BatchedMCTS(cfg, net, B, mode=m)
        res = engine.run_from_roots(roots, [i % len(players) for i in range(B)], True,
                                    [numpy.random.RandomState(500 + i) for i in range(B)])
        outs.append((res, engine.export_trees(B), engine.kernel_name(B)))
    (r0, t0, _), (r1, t1, kernel) = outs
    assert "fc2_search_kernel" in kernel, kernel
    _assert_equal(r0, t0, r1, t1, skip=("root_predicted_values",))      # (none: the roots were given)
    assert r0.visit_counts[one, 1] == S and sorted(t0["child"][one, 0]) == [-1, 1]
    assert (t0["n_nodes"] == S + 1).all() and (r1.visit_counts.sum(1) == S).all()
    assert (t0["reward"][:, 0] == numpy.array(rewards)).all()


def _continued(engine, cfg, net, B, rounds, seed, to_play, check):
    """A fresh search and `rounds` continuations (result, trees, kernel, route per round).  The pick of tree i in round r is
    test_gpu_continue_shapes' pick of round r + 1: a lone tree moves to its most visited child, then to its least visited
    expanded one; from three trees on every round also searches an old root again."""
    obs = synthetic.observations(B, net.input_shape, seed=seed)
    rngs = [numpy.random.RandomState(seed + i) for i in range(B)]
    legal = [list(cfg.action_space)] * B
    P = len(cfg.players)
    tp = numpy.array(to_play, numpy.int64)
    out = []

    def note(res):
        kernel, route = engine.kernel_name(B), shapes.whole._route(engine, B)
        check(kernel, route)
        assert (res.flags == 0).all(), res.flags
        out.append((res, engine.export_trees(B), kernel, route))

    res = engine.run(list(obs), legal, list(tp), True, rngs)
    note(res)
    for r in range(rounds):
        acts = [shapes._pick(res, i, r + 1) for i in range(B)]
        assert any(a >= 0 for a in acts) and (B < 3 or any(a < 0 for a in acts))
        tp = numpy.array([(tp[i] + 1) % P if a >= 0 else tp[i] for i, a in enumerate(acts)])
        res = engine.continue_search(acts, list(tp), True, rngs)
        note(res)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [None, 7], ids=["small", "lds"])
def test_continued_search(backend, mode, B):
    """A fresh search and two continuations on a handle with spare capacity, two players: leaf indices beyond S + 1, the
    hidden states exported and imported around the dead tail, fc2_from_arena leaving the dead slot row alone."""
    S = 12
    cfg = configs.cartpole(players=[0, 1], num_simulations=S)
    net = lean._weights(cfg, "signs")
    to_play = [i % 2 for i in range(B)]
    outs = {}
    for m, check in ((mode, shapes._is(shapes.FC2, 4)), (0, shapes._is(shapes.PER_OPERATOR, 0))):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=m, max_carried_nodes=3 * S)
        outs[m] = _continued(engine, cfg, net, B, 2, 31, to_play, check)
    for r, (x, y) in enumerate(zip(outs[mode], outs[0])):
        shapes.whole._assert_same(x, y, ("continued", "round", r))
    assert len(outs[0]) == 3 and outs[0][-1][1]["n_nodes"].max() > S + 1


#        name: config factory
WIDE = {
    "four-actions": configs.lunarlander,        # A = 4: the AW = 4 instantiation
    "six-actions": shapes._lds16(6),            # 4 < A <= 16: the AW = 16 instantiation (generic walk and refresh)
}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wider_records(backend, name):
    """Fully connected configurations with four and with more than four actions at five trees, ragged legal sets with a
    single-action root (tree 0), a fresh search and one continuation against the per-operator path."""
    B, S = 5, 12
    cfg = WIDE[name](num_simulations=S)
    A, P = len(cfg.action_space), len(cfg.players)
    assert (A == 4) if name == "four-actions" else (4 < A <= 16)
    net = shapes.whole._net(cfg, 11)
    legal = shapes.ragged_legal(A, B, 23)
    assert len(legal[0]) == 1 and len({len(a) for a in legal}) > 1
    to_play = [i % P for i in range(B)]
    outs = {}
    for m, check in ((None, shapes._is(shapes.FC2, 4)), (0, shapes._is(shapes.PER_OPERATOR, 0))):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=m, max_carried_nodes=3 * S)
        outs[m] = shapes._chain(engine, cfg, net, B, 1, 31, legal, to_play, check)
    shapes._assert_same(outs[None], outs[0], name)
    first = outs[0][0][0]
    assert first.visit_counts[0][legal[0][0]] == S and first.visit_counts[0].sum() == S
