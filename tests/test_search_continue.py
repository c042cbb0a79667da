"""
Continued searches -- MCTS.run(..., override_root_with=node) on a node that already carries visits and expanded
descendants (/root/reference/self_play.py:260-361) -- on the CPU:
  * the oracle helper (tests/continue_oracle.py) against the live reference (``reference``-marked);
  * the serial test double of the C ABI (tests/hostcheck: tree_advance_kernel's per-lane pieces, the continued root
    preparation, the lock-step simulations) against the helper, bit for bit, chained and with a = -1;
  * the refusals: capacity, to_play, a route that leaves no hidden states, searches without spare capacity;
  * BatchedMCTS.continue_search against run_from_trees on the host-flattened node_graph: identical trees.
GPU twin: tests/test_gpu_search_continue.py.
"""
import ctypes

import numpy
import pytest
import torch

import continue_oracle as co
import hostcheck
from mzx import _lib, configs, models, self_play, synthetic
from oracle import mcts_oracle as mo
from oracle import net_oracle, ref_shim


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


# ---------------------------------------------------------------- the helper against the live reference

def _ref_graph_equal(a, tree, n=0):
    """Reference Node `a` against node n of an oracle Tree: statistics bit for bit, children in order, recursively."""
    assert a.visit_count == tree.visit[n] and a.to_play == tree.to_play[n]
    assert a.value_sum == tree.value_sum[n] and a.reward == tree.reward[n]
    assert list(a.children) == list(tree.actions[n])
    count = 1
    for s, (action, ch) in enumerate(a.children.items()):
        assert ch.prior == tree.prior[n][s], (n, action)
        c = tree.child[n][s]
        assert ch.expanded() == (c >= 0)
        if c >= 0:
            count += _ref_graph_equal(ch, tree, c)
    return count


@pytest.mark.reference
@pytest.mark.parametrize("game", ["cartpole", "tictactoe"])
@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("which", ["child", "root"])
def test_helper_equals_live_reference(game, noise, which):
    ref_models, ref_self_play = ref_shim.load()
    cfg = configs.BY_NAME[game](num_simulations=25)
    torch.manual_seed(0)
    ref = ref_models.MuZeroNetwork(cfg)
    ref.set_weights(synthetic.fill_state_dict(ref.state_dict(), 31))
    ref.eval()
    net = models.MuZeroNetwork(cfg, _backend=hostcheck.backend())
    obs = synthetic.observations(1, net.input_shape, seed=3)[0]
    legal = list(cfg.action_space)[2:] if game == "tictactoe" else list(cfg.action_space)
    numpy.random.seed(11)
    with torch.no_grad():
        root, _ = ref_self_play.MCTS(cfg).run(ref, obs, legal, 0, True)
        best = max(root.children, key=lambda a: root.children[a].visit_count)
        node = root.children[best] if which == "child" else root
        searched, info = ref_self_play.MCTS(cfg).run(ref, None, legal, node.to_play, noise, override_root_with=node)
    assert searched is node and info["root_predicted_value"] is None
    rng = numpy.random.RandomState(11)
    ev = net_oracle.NetworkEvaluator(ref, cfg.support_size)
    tree = mo.run_search(cfg, ev, obs, legal, 0, True, rng)
    tree = co.carry(tree, cfg, best if which == "child" else -1)
    co.continue_search(cfg, ev, tree, tree.to_play[0], noise, rng)
    assert info["max_tree_depth"] == tree.max_depth
    assert _ref_graph_equal(node, tree) == len(tree.visit)
    assert numpy.array_equal(numpy.random.get_state()[1], rng.get_state()[1])
    assert numpy.random.get_state()[2] == rng.get_state()[2]


# ---------------------------------------------------------------- the serial ABI against the helper

def _carry_case(backend, game, B, S, rounds, noise, ties=False, legal_cut=0, pick=None, seed=0):
    cfg = configs.BY_NAME[game](num_simulations=S)
    A = len(cfg.action_space)
    legal = [list(cfg.action_space)[legal_cut:] for _ in range(B)]
    cap = (rounds + 1) * S + 1 + 1
    ls = co.LockstepCarry(backend, cfg, B, S, cap)
    count = (rounds + 1) * S + 1
    dev_rngs = [numpy.random.RandomState(seed + 100 + i) for i in range(B)]
    ora_rngs = [numpy.random.RandomState(seed + 100 + i) for i in range(B)]
    dev_ev = [co.ReplayValues(seed + i, count, A, ties) for i in range(B)]
    ora_ev = [co.ReplayValues(seed + i, count, A, ties) for i in range(B)]
    trees = [mo.run_search(cfg, ora_ev[i], None, legal[i], 0, noise, ora_rngs[i]) for i in range(B)]
    got = ls.fresh(legal, numpy.zeros(B, numpy.int32), noise, dev_rngs, dev_ev)
    for i in range(B):
        co.assert_tree_equal(got, i, trees[i], A)
    pick = pick or (lambda r, i, t: -1 if (r + i) % 3 == 2 else max(
        (a for s, a in enumerate(t.actions[0]) if t.child[0][s] >= 0), key=lambda a: t.visit[t.child[0][t.actions[0].index(a)]]))
    for r in range(rounds):
        acts = [pick(r, i, trees[i]) for i in range(B)]
        trees = [co.carry(trees[i], cfg, acts[i]) for i in range(B)]
        assert ls.advance(acts) == 0, backend.lib.mzx_last_error()
        for i in range(B):
            co.continue_search(cfg, ora_ev[i], trees[i], trees[i].to_play[0], noise, ora_rngs[i])
        got = ls.cont([len(t.actions[0]) for t in trees], numpy.array([t.to_play[0] for t in trees], numpy.int32), noise,
                      dev_rngs, dev_ev)
        for i in range(B):
            co.assert_tree_equal(got, i, trees[i], A)
            assert got["predicted"][i] != got["predicted"][i]      # NaN: root_predicted_value is None
            assert numpy.array_equal(dev_rngs[i].get_state()[1], ora_rngs[i].get_state()[1])
    ls.close()
    return trees


@pytest.mark.parametrize("game,noise,ties,cut", [("cartpole", True, False, 0), ("tictactoe", True, False, 3),
                                                 ("connect4", False, True, 0), ("tictactoe", False, True, 0)])
def test_hostcheck_chained_continuations_equal_helper(backend, game, noise, ties, cut):
    trees = _carry_case(backend, game, 6, 12, 3, noise, ties, cut)
    assert all(len(t.visit) > 12 for t in trees)


def test_hostcheck_root_again_keeps_legal_children(backend):
    """a = -1 every round: the root keeps its own (legal) children, its visits accumulate."""
    trees = _carry_case(backend, "tictactoe", 4, 10, 2, True, legal_cut=4, pick=lambda r, i, t: -1)
    for t in trees:
        assert len(t.actions[0]) == 5 and t.visit[0] == 30 and len(t.visit) == 31


def test_hostcheck_refusals(backend):
    cfg = configs.BY_NAME["tictactoe"](num_simulations=8)
    B, A = 3, len(cfg.action_space)
    legal = [list(cfg.action_space)] * B
    ls = co.LockstepCarry(backend, cfg, B, 8, 8 + 1 + 8)      # room for 8 carried nodes
    ev = [co.ReplayValues(i, 40, A) for i in range(B)]
    rngs = [numpy.random.RandomState(i) for i in range(B)]
    lib = backend.lib
    # continuing before anything was carried
    with pytest.raises(_lib.MzxError, match="no carried trees"):
        ls.cont([A] * B, numpy.zeros(B, numpy.int32), False, rngs, ev)
    ls.fresh(legal, numpy.zeros(B, numpy.int32), False, rngs, ev)
    # the old root carries 9 nodes: 9 + 8 + 1 > 17
    assert ls.advance([-1] * B) == 0
    with pytest.raises(_lib.MzxError, match="node slots"):
        ls.cont([A] * B, numpy.zeros(B, numpy.int32), False, rngs, ev)
    # a child: fewer nodes, but to_play must be the carried root's (player 1 after the root's move)
    d = ls.dump(ls.arenas[0])
    acts = [int(numpy.nonzero(d["child"][i, 0] > 0)[0][0]) for i in range(B)]
    ls.arenas.reverse()        # back to the fresh trees (the advance above did not touch them)
    assert ls.advance(acts) != 0            # the handle's last call left its trees in the other arena
    assert b"d_src_arena" in lib.mzx_last_error()
    ls.close()

    ls = co.LockstepCarry(backend, cfg, B, 8, 8 + 1 + 8)
    ls.fresh(legal, numpy.zeros(B, numpy.int32), False, rngs, ev)
    d = ls.dump(ls.arenas[0])
    acts = [int(numpy.nonzero(d["child"][i, 0] > 0)[0][0]) for i in range(B)]
    assert ls.advance(acts) == 0
    with pytest.raises(_lib.MzxError, match="to_play"):
        ls.cont([A] * B, numpy.zeros(B, numpy.int32), False, rngs, ev)
    got = ls.cont([A] * B, numpy.ones(B, numpy.int32), False, rngs, ev)
    assert (got["info"][:, 1] == 0).all() and (got["visits"].sum(1) > 8).all()
    # the same arena twice
    t = ls.dev(numpy.zeros(B, numpy.int32), torch.int32)
    assert lib.mzx_search_advance(ls.handle, backend.ptr(t), backend.ptr(ls.arenas[0]), backend.ptr(ls.arenas[0]), None) != 0
    ls.close()


def _engine(backend, game, S, carried, mode=0, seed=7):
    cfg = configs.BY_NAME[game](num_simulations=S)
    net = models.MuZeroNetwork(cfg, _backend=backend)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), seed))
    return cfg, net, self_play.BatchedMCTS(cfg, net, 4, mode=mode, max_carried_nodes=carried)


def test_hostcheck_without_capacity_or_hidden_states_refuses(backend):
    cfg, net, engine = _engine(backend, "cartpole", 6, 0)
    obs = synthetic.observations(4, net.input_shape, seed=1)
    engine.run(list(obs), [list(cfg.action_space)] * 4, [0] * 4, False, [numpy.random.RandomState(i) for i in range(4)])
    with pytest.raises(ValueError, match="max_carried_nodes"):
        engine.continue_search([0] * 4, [0] * 4, False, [numpy.random.RandomState(i) for i in range(4)])
    # a lock-step search on a handle WITH a network leaves no hidden states: advance refuses and says why
    cfg, net, engine = _engine(backend, "cartpole", 6, 20)
    h = engine.handle(4)
    lib = backend.lib
    arena = engine.arena(4)
    legal = torch.zeros((4, 2), dtype=torch.int32)
    legal[:, 1] = 1
    tp = torch.zeros(4, dtype=torch.int32)
    pri = torch.full((4, 2), 0.5, dtype=torch.float64)
    io = _lib.SearchIO(None, backend.ptr(legal), backend.ptr(tp), None, None, None, None, None, None)
    lib.check(lib.mzx_search_lockstep_begin(h, ctypes.byref(io), backend.ptr(pri), None, backend.ptr(arena), arena.numel(), None))
    other = torch.zeros_like(arena)
    acts = torch.full((4,), -1, dtype=torch.int32)
    assert lib.mzx_search_advance(h, backend.ptr(acts), backend.ptr(arena), backend.ptr(other), None) == -1
    assert b"hidden state" in lib.mzx_last_error()


@pytest.mark.parametrize("game", ["cartpole", "tictactoe"])
def test_hostcheck_continue_search_equals_run_from_trees(backend, game):
    """tree_advance_kernel's carry against the host flattening of node_graph (run_from_trees): the same trees."""
    S, B = 10, 4
    out = []
    for path in ("advance", "load"):
        cfg, net, engine = _engine(backend, game, S, 3 * S)
        obs = synthetic.observations(B, net.input_shape, seed=2)
        legal = [list(cfg.action_space)] * B
        rngs = [numpy.random.RandomState(50 + i) for i in range(B)]
        res = engine.run(list(obs), legal, [0] * B, True, rngs)
        acts = [int(numpy.argmax(res.visit_counts[i])) if i % 2 == 0 else -1 for i in range(B)]
        tp = [(1 if len(cfg.players) == 2 else 0) if a >= 0 else 0 for a in acts]
        if path == "advance":
            res2 = engine.continue_search(acts, tp, True, rngs)
        else:
            roots = [engine.node_graph(B, i, legal[i]) for i in range(B)]
            roots = [r.children[a] if a >= 0 else r for r, a in zip(roots, acts)]
            res2 = engine.run_from_trees(roots, tp, True, rngs)
            for i, r in enumerate(roots):   # searched in place: the given objects carry the new statistics
                assert r.visit_count == (res.visit_counts[i][acts[i]] if acts[i] >= 0 else S) + S
        assert res2.root_predicted_values == [None] * B
        out.append((res2, engine.export_trees(B), [r.get_state()[2] for r in rngs]))
    (ra, ta, sa), (rb, tb, sb) = out
    assert numpy.array_equal(ra.visit_counts, rb.visit_counts) and numpy.array_equal(ra.root_values, rb.root_values)
    for k in ("max_tree_depth", "flags", "tape_used", "sum_depth"):
        assert numpy.array_equal(getattr(ra, k), getattr(rb, k)), k
    assert sa == sb
    for k in ta:
        if k == "child" or k == "prior":
            continue
        assert numpy.array_equal(ta[k], tb[k]), k
    for i in range(B):        # slots past a node's children are padding
        n = int(ta["n_nodes"][i])
        assert numpy.array_equal(ta["child"][i, :n], tb["child"][i, :n])
        assert numpy.array_equal(ta["prior"][i, 1:n], tb["prior"][i, 1:n])
