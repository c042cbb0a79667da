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

def _config(game, S):
    """A named game (configs.BY_NAME) or a factory of a config that takes num_simulations."""
    return configs.BY_NAME[game](num_simulations=S) if isinstance(game, str) else game(num_simulations=S)


def wide32(**kw):
    """32 actions on a 4 x 8 board, two players: several child slots per lane in the device kernels."""
    return configs.connect4(observation_shape=(3, 4, 8), action_space=list(range(32)), **kw)


def ragged_legal(A, B, seed):
    """Per-tree legal sets as tests/test_gpu_tower_search.py draws them; tree 0 keeps a single action."""
    rs = numpy.random.RandomState(seed)
    legal = [sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for _ in range(B)]
    legal[0] = legal[0][:1]
    return legal


def _expanded(t):
    """(node index, visits, action) of the expanded children of the root of oracle tree t."""
    return [(c, t.visit[c], a) for a, c in zip(t.actions[0], t.child[0]) if c >= 0]


def pick_alternating(r, i, t):
    """The old root again and an expanded child in the same shard and round: the trees alternate between them in pairs (trees
    0, 1, 4, 5, ... start with the root: root again on its restricted legal set, then a child, then that child again as a
    root), so that with tree i starting as player i % P both players meet both kinds; the child is the most visited one
    or, for odd i, the least visited expanded one."""
    if (r + i // 2) % 2 == 0:
        return -1
    seen = [(v, a) for _, v, a in _expanded(t)]
    return (max(seen) if i % 2 == 0 else min(seen, key=lambda x: (x[0], -x[1])))[1]


def pick_late_child(r, i, t):
    """The old root for three rounds, then its expanded child with the largest node index (the youngest subtree)."""
    return -1 if r < 3 else max(_expanded(t))[2]


def _carry_case(backend, game, B, S, rounds, noise, ties=False, legal_cut=0, pick=None, seed=0, ragged=False,
                mixed_to_play=False, log=None):
    """ragged: per-tree legal sets (ragged_legal); mixed_to_play: tree i starts with player i % P; log: a list that gets,
    per round, the chosen actions, the old node index of every new root and the node counts carried (oracle trees)."""
    cfg = _config(game, S)
    A, P = len(cfg.action_space), len(cfg.players)
    legal = ragged_legal(A, B, seed + 7) if ragged else [list(cfg.action_space)[legal_cut:] for _ in range(B)]
    tp0 = [i % P if mixed_to_play else 0 for i in range(B)]
    cap = (rounds + 1) * S + 1 + 1
    ls = co.LockstepCarry(backend, cfg, B, S, cap)
    count = (rounds + 1) * S + 1
    dev_rngs = [numpy.random.RandomState(seed + 100 + i) for i in range(B)]
    ora_rngs = [numpy.random.RandomState(seed + 100 + i) for i in range(B)]
    dev_ev = [co.ReplayValues(seed + i, count, A, ties) for i in range(B)]
    ora_ev = [co.ReplayValues(seed + i, count, A, ties) for i in range(B)]
    trees = [mo.run_search(cfg, ora_ev[i], None, legal[i], tp0[i], noise, ora_rngs[i]) for i in range(B)]
    got = ls.fresh(legal, numpy.array(tp0, numpy.int32), noise, dev_rngs, dev_ev)
    for i in range(B):
        co.assert_tree_equal(got, i, trees[i], A)
    pick = pick or (lambda r, i, t: -1 if (r + i) % 3 == 2 else max(
        (a for s, a in enumerate(t.actions[0]) if t.child[0][s] >= 0), key=lambda a: t.visit[t.child[0][t.actions[0].index(a)]]))
    for r in range(rounds):
        acts = [pick(r, i, trees[i]) for i in range(B)]
        chosen = [0 if a < 0 else t.child[0][t.actions[0].index(a)] for a, t in zip(acts, trees)]
        trees = [co.carry(trees[i], cfg, acts[i]) for i in range(B)]
        if log is not None:
            log.append(dict(acts=acts, chosen=chosen, carried=[len(t.visit) for t in trees], legal_n=[len(a) for a in legal],
                            root_n=[len(t.actions[0]) for t in trees], to_play=[t.to_play[0] for t in trees]))
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


def assert_root_shapes(log, A, P, B):
    """What a ragged, alternating chain has to contain to be worth its name (read off the oracle trees)."""
    first = log[0]
    assert len(set(first["legal_n"])) > 1                                                     # ragged sets
    assert any(n == 1 and a < 0 for n, a in zip(first["root_n"], first["acts"]))              # a single-action root, again
    assert all(any(a < 0 for a in r["acts"]) and any(a >= 0 for a in r["acts"]) for r in log)     # both kinds, every round
    # root again on a restricted root, then its child (a full root), then that root again
    assert any(log[0]["acts"][i] < 0 and log[0]["root_n"][i] < A and log[1]["acts"][i] >= 0 and log[2]["acts"][i] < 0
               for i in range(B))


CHAINS = [("cartpole", True, False), ("lunarlander", True, False), ("tictactoe", True, True), (wide32, False, True),
          ("gomoku", True, False)]


@pytest.mark.parametrize("game,noise,ties", CHAINS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_hostcheck_ragged_roots_mixed_players_equal_helper(backend, game, noise, ties):
    """Ragged legal sets (a single-action root among them), tree i starting with player i % P, and a pick that searches
    the old root again in some trees and moves to an expanded child in others, in the same shard and round: the slot ->
    action map of a restricted root survives a = -1, is replaced by the whole action space under a child, and the noise
    covers exactly the root's own slots.  Action spaces 2, 4, 9, 32 and 121."""
    B, S = 8, 10
    cfg = _config(game, S)
    log = []
    trees = _carry_case(backend, game, B, S, 3, noise, ties, pick=pick_alternating, seed=5, ragged=True, mixed_to_play=True,
                        log=log)
    assert_root_shapes(log, len(cfg.action_space), len(cfg.players), B)
    P = len(cfg.players)
    for r in log:      # both players at roots searched again and at new roots, in every round
        assert len({p for p, a in zip(r["to_play"], r["acts"]) if a < 0}) == P, r
        assert len({p for p, a in zip(r["to_play"], r["acts"]) if a >= 0}) == P, r


LATE = [(wide32, True), ("gomoku", False)]


@pytest.mark.parametrize("game,ties", LATE, ids=lambda v: getattr(v, "__name__", str(v)))
def test_hostcheck_carry_starts_past_the_first_chunk(backend, game, ties):
    """A new root whose old node index is >= 64: tree_advance_kernel's membership loop starts at `c & ~63`, past chunk 0,
    and the trees that keep their root carry more than 64 nodes (two chunks).  3 S + 1 nodes never reach 64 at S <= 20, so
    this chain alone has a fourth round: three times the old root (21, 41, 61, 81 nodes), then its youngest expanded child."""
    log = []
    _carry_case(backend, game, 6, 20, 4, True, ties, pick=lambda r, i, t: -1 if i % 2 else pick_late_child(r, i, t), seed=9,
                ragged=True, mixed_to_play=True, log=log)
    assert max(log[3]["chosen"]) >= 64, log[3]["chosen"]
    assert max(log[3]["carried"]) > 64


def _bad_carry_actions(d, legal, A):
    """Per tree of a fresh dump: (action, kind) with kind 0 = a legal action whose child was never expanded, 1 = an action
    outside the root's legal set, 2 = an expanded child -- each kind in every third tree."""
    out = []
    for i, acts in enumerate(legal):
        child = d["child"][i, 0]
        never = [a for s, a in enumerate(acts) if child[s] < 0]
        illegal = [a for a in range(A) if a not in acts]
        valid = [a for s, a in enumerate(acts) if child[s] > 0]
        kind = i % 3
        assert never and illegal and valid, (i, acts)
        out.append(((never[-1], illegal[0], valid[-1])[kind], kind))
    return out


def bad_carry_lockstep(backend, game, B, S, seed=0):
    """TF_BAD_CARRY through the C ABI: mzx_search_advance with actions that name no expanded child (the library's host
    guard lives in BatchedMCTS.continue_search, not here).  carry_root reports them, the old root is kept, carry_meta sets
    flag 4, ContinueRootOp preserves it, the simulations run on the old root and mzx_search_finish reports it: info word 1
    is 4 exactly on those trees, which equal what a = -1 yields under the oracle helper; the valid trees equal the helper."""
    cfg = _config(game, S)
    A, P = len(cfg.action_space), len(cfg.players)
    rs = numpy.random.RandomState(seed + 3)
    legal = [sorted(rs.choice(A, size=rs.randint(S + 1, A), replace=False).tolist()) for _ in range(B)]     # S < |legal| < A
    tp0 = [i % P for i in range(B)]
    ls = co.LockstepCarry(backend, cfg, B, S, 2 * S + 2)
    dev_rngs = [numpy.random.RandomState(seed + 40 + i) for i in range(B)]
    ora_rngs = [numpy.random.RandomState(seed + 40 + i) for i in range(B)]
    dev_ev = [co.ReplayValues(seed + i, 2 * S + 1, A) for i in range(B)]
    ora_ev = [co.ReplayValues(seed + i, 2 * S + 1, A) for i in range(B)]
    trees = [mo.run_search(cfg, ora_ev[i], None, legal[i], tp0[i], True, ora_rngs[i]) for i in range(B)]
    got = ls.fresh(legal, numpy.array(tp0, numpy.int32), True, dev_rngs, dev_ev)
    picks = _bad_carry_actions(got, legal, A)
    assert {k for _, k in picks} == {0, 1, 2}
    assert ls.advance([a for a, _ in picks]) == 0, backend.lib.mzx_last_error()
    trees = [co.carry(trees[i], cfg, a if kind == 2 else -1) for i, (a, kind) in enumerate(picks)]
    for i in range(B):
        co.continue_search(cfg, ora_ev[i], trees[i], trees[i].to_play[0], True, ora_rngs[i])
    got = ls.cont([len(t.actions[0]) for t in trees], numpy.array([t.to_play[0] for t in trees], numpy.int32), True,
                  dev_rngs, dev_ev)
    want = numpy.array([0 if kind == 2 else 4 for _, kind in picks])
    assert numpy.array_equal(got["info"][:, 1], want), got["info"][:, 1]
    for i, (a, kind) in enumerate(picks):
        co.assert_tree_equal(got, i, trees[i], A, flags=int(want[i]))
        if kind != 2:
            assert len(trees[i].actions[0]) == len(legal[i]) and got["n_nodes"][i] == 2 * S + 1     # the old root, whole
        assert numpy.array_equal(dev_rngs[i].get_state()[1], ora_rngs[i].get_state()[1])
    ls.close()


@pytest.mark.parametrize("game", ["tictactoe", "lunarlander"])
def test_hostcheck_bad_carry_keeps_the_old_root_and_flags_it(backend, game):
    bad_carry_lockstep(backend, game, 9, 3 if game == "tictactoe" else 2)


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
