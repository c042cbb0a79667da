"""
Continued searches inside the whole-search kernels on the MI355X: fc2_search_kernel (fully connected networks) imports each
carried tree into LDS, hidden states included, and rt_search_kernel (connect4-class residual networks) walks the carried
trees in the arena with the roots' visit counts read from the trees.  Handles with spare node capacity
(BatchedMCTS(max_carried_nodes=...)) take these kernels for fresh and continued searches alike:
  * the route (mzx_search_route / kernel_name) for C2 (cartpole 4096 x 50) and connect4 (1024 x 200);
  * bit identity with the per-operator path (mode 0) for fully connected networks, and with the launch-by-launch tower route
    (tuning "rt_search" = 0) for connect4 -- the per-operator path runs connect4's network on the LDS-resident engine, which
    sums a convolution in another order (csrc/mzx_row_search.h) -- over chains of continuations with ragged carried counts;
  * the oracle helper's restatement of the continued search (tests/continue_oracle.py) on small shapes;
  * the capacity edges, the to_play refusal and the fall-back of a capacity fc2's LDS cannot hold;
  * trees imported with mzx_search_load (run_from_trees) against the device carry.
"""
import numpy
import pytest
import torch

from mzx import _lib, configs, models, self_play, synthetic
from oracle import mcts_oracle as mo

import continue_oracle as co

pytestmark = pytest.mark.gpu

FC2, RT = "mzx::fc2_search_kernel", "mzx::rt_search_kernel"
PER_OPERATOR = "one kernel per step of a simulation"
TREE_KEYS = ("visit", "value_sum", "reward", "to_play", "parent", "child", "prior", "minmax", "n_nodes")


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _net(cfg, seed, zero=(), uniform_policy=False):
    """Synthetic weights; `zero`: key prefixes whose weight matrices / kernels are zeroed (outputs that do not depend on the
    input); uniform_policy: the policy head outputs equal logits (tie-prone trees: at most one tie-break draw per
    simulation, so that 12 simulations stay within the 16 tape words a carryable search has)."""
    net = models.MuZeroNetwork(cfg)
    sd = synthetic.fill_state_dict(net.state_dict(), seed)
    for k, v in sd.items():
        if zero and k.startswith(zero) and v.dim() > 1:
            v.zero_()
        if uniform_policy and "policy" in k and v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.zero_()
    net.set_weights(sd)
    return net


def _route(engine, B):
    lib = engine.backend.lib
    out = (lib.mzx_search_route.argtypes[1]._type_)()
    lib.check(lib.mzx_search_route(engine.handle(B), out))
    return list(out)


def _pick(res, trees, i, r, legal):
    """Chosen action of tree i in round r: the old root again, the most visited child, or the least visited expanded one."""
    v = res.visit_counts[i]
    k = (i + r) % 4
    if k == 0:
        return -1
    if k == 2:
        seen = [a for a in legal if v[a] > 0]
        return int(min(seen, key=lambda a: (v[a], a)))
    return int(numpy.argmax(v))


def _chain(engine, cfg, net, B, rounds, seed, pick=_pick):
    obs = synthetic.observations(B, net.input_shape, seed=seed)
    legal = [list(cfg.action_space)] * B
    rngs = [numpy.random.RandomState(seed + i) for i in range(B)]
    res = engine.run(list(obs), legal, [0] * B, True, rngs)
    trees = engine.export_trees(B)
    out = [(res, trees, engine.kernel_name(B), _route(engine, B))]
    to_play = numpy.zeros(B, numpy.int64)
    P = len(cfg.players)
    for r in range(rounds):
        acts = [pick(res, trees, i, r, list(cfg.action_space)) for i in range(B)]
        to_play = numpy.array([(to_play[i] + 1) % P if a >= 0 else to_play[i] for i, a in enumerate(acts)])
        res = engine.continue_search(acts, list(to_play), True, rngs)
        assert (res.flags == 0).all()
        trees = engine.export_trees(B)
        out.append((res, trees, engine.kernel_name(B), _route(engine, B)))
    torch.cuda.synchronize()
    return out


def _bits(a):
    return a.view(numpy.int64) if a.dtype == numpy.float64 else a


def _assert_same(a, b, label):
    (ra, ta, _, _), (rb, tb, _, _) = a, b
    assert numpy.array_equal(ra.visit_counts, rb.visit_counts), label
    assert numpy.array_equal(_bits(ra.root_values), _bits(rb.root_values)), label
    for k in ("max_tree_depth", "flags", "tape_used", "sum_depth"):
        assert numpy.array_equal(getattr(ra, k), getattr(rb, k)), (label, k)
    for k in TREE_KEYS:
        assert numpy.array_equal(_bits(ta[k]), _bits(tb[k])), (label, k)


# ---------------------------------------------------------------- 1. the route

def test_route_c2_and_connect4_on_spare_capacity(backend):
    cfg = configs.cartpole(num_simulations=50)
    B, S = 4096, 50
    net = _net(cfg, 3)
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=2 * S + 1)
    assert _route(engine, B)[0] == 4

    def pick(res, trees, i, r, legal):       # bounded by the capacity: at most 2 S + 1 nodes carried in every round
        return -1 if r == 0 and i % 2 else int(numpy.argmax(res.visit_counts[i]))

    outs = _chain(engine, cfg, net, B, 2, 5, pick)
    for res, t, kernel, route in outs:
        assert kernel == FC2 and route[0] == 4, (kernel, route)
        assert (res.flags == 0).all()
    assert (outs[-1][1]["n_nodes"] > S + 1).any()

    cfg = configs.connect4()
    B, S = 1024, cfg.num_simulations
    assert S == 200
    net = _net(cfg, 4)
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=S + 1)
    assert _route(engine, B)[0] == 3
    outs = _chain(engine, cfg, net, B, 1, 6, lambda res, t, i, r, legal: int(numpy.argmax(res.visit_counts[i])))
    for res, t, kernel, route in outs:
        assert kernel == RT and route[0] == 3, (kernel, route)


# ---------------------------------------------------------------- 2. bit identity with the per-operator path

@pytest.mark.parametrize("game,B,S,ties", [("cartpole", 256, 30, False), ("cartpole", 96, 12, True),
                                           ("lunarlander", 128, 20, False)])
def test_fc2_continuations_equal_per_operator_path(backend, game, B, S, ties):
    cfg = configs.BY_NAME[game](num_simulations=S)
    net = _net(cfg, 11, uniform_policy=ties)
    outs = {}
    for mode in (None, 0):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=4 * S)
        outs[mode] = _chain(engine, cfg, net, B, 3, 31)
    assert all(k == FC2 and rt[0] == 4 for _, _, k, rt in outs[None]), [(k, rt[0]) for _, _, k, rt in outs[None]]
    assert all(PER_OPERATOR in k and rt[0] == 0 for _, _, k, rt in outs[0])
    for r, (a, b) in enumerate(zip(outs[None], outs[0])):
        _assert_same(a, b, (game, "round", r))
    n = outs[None][-1][1]["n_nodes"]
    assert n.min() < n.max() and n.max() >= 2 * S + 1      # ragged carried counts, deep carries
    if ties:
        assert (outs[None][-1][0].tape_used > 0).any()


def test_rt_continuations_equal_tower_launches(backend):
    cfg = configs.connect4(num_simulations=30)
    B, S = 64, 30
    net = _net(cfg, 12)
    outs = {}
    for label, tuning in (("rt", {}), ("launches", {"rt_search": 0})):
        with backend.lib.tuning(**tuning):
            engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=4 * S)
            outs[label] = _chain(engine, cfg, net, B, 3, 41)
    assert all(k == RT and rt[0] == 3 for _, _, k, rt in outs["rt"]), [k for _, _, k, _ in outs["rt"]]
    assert all("row_select_kernel" in k and "rb_tower_kernel" in k and rt[0] == 2 for _, _, k, rt in outs["launches"])
    for r, (a, b) in enumerate(zip(outs["rt"], outs["launches"])):
        _assert_same(a, b, ("connect4", "round", r))
    n = outs["rt"][-1][1]["n_nodes"]
    assert n.min() < n.max() and n.max() >= 2 * S + 1


# ---------------------------------------------------------------- 3. the oracle helper

class _Constant:
    """recurrent_inference of a network whose dynamics ignore their input: every expansion gets the same outputs."""

    def __init__(self, value, reward, priors):
        self.value, self.reward, self.priors = value, reward, priors

    def recurrent(self, hidden, action, actions):
        return self.value, self.reward, list(self.priors[: len(actions)]), None


def _oracle_tree(t, i, root_actions, A):
    n = int(t["n_nodes"][i])
    tr = mo.Tree()
    for k in range(n):
        acts = list(root_actions) if k == 0 else list(range(A))
        m = len(acts)
        tr.actions.append(acts)
        tr.visit.append(int(t["visit"][i, k]))
        tr.value_sum.append(float(t["value_sum"][i, k]))
        tr.reward.append(float(t["reward"][i, k]))
        tr.to_play.append(int(t["to_play"][i, k]))
        tr.hidden.append(None)
        tr.prior.append([float(x) for x in t["prior"][i, k, :m]])
        tr.child.append([int(x) for x in t["child"][i, k, :m]])
        tr.parent.append(int(t["parent"][i, k]))
        tr.parent_slot.append(-1)
    for k in range(n):
        for s, c in enumerate(tr.child[k]):
            if c >= 0:
                tr.parent_slot[c] = s
    tr.minimum, tr.maximum = float(t["minmax"][i, 0]), float(t["minmax"][i, 1])
    return tr


@pytest.mark.parametrize("game,B,S,kernel,prefixes", [
    ("cartpole", 16, 12, FC2, ("representation", "dynamics_encoded_state")),
    ("connect4", 8, 12, RT, ("representation", "dynamics")),
])
def test_continuations_equal_oracle_helper(backend, game, B, S, kernel, prefixes):
    """The representation and dynamics networks ignore their inputs (zeroed weight tensors, random biases), so every
    expansion of a continued search gets the same value / reward / priors: read off the fresh trees, they drive the oracle
    helper's restatement (tests/continue_oracle.py) from the fresh trees, and the device's continued trees must equal it."""
    cfg = configs.BY_NAME[game](num_simulations=S)
    A, P = len(cfg.action_space), len(cfg.players)
    net = _net(cfg, 21, zero=prefixes)
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=4 * S)
    obs = synthetic.observations(B, net.input_shape, seed=2)
    legal = [list(cfg.action_space)] * B
    rngs = [numpy.random.RandomState(900 + i) for i in range(B)]
    res = engine.run(list(obs), legal, [0] * B, True, rngs)
    assert engine.kernel_name(B) == kernel
    t = engine.export_trees(B)
    # the network's constant recurrent outputs, and the premise that they are constant
    leaf = [(i, k) for i in range(B) for k in range(1, int(t["n_nodes"][i])) if t["visit"][i, k] == 1]
    assert leaf
    i0, k0 = leaf[0]
    value, reward, priors = float(t["value_sum"][i0, k0]), float(t["reward"][i0, 1]), [float(x) for x in t["prior"][i0, 1]]
    for i in range(B):
        n = int(t["n_nodes"][i])
        assert (co.bits(t["reward"][i, 1:n]) == co.bits([reward])).all()
        assert (co.bits(t["prior"][i, 1:n]) == co.bits([priors])).all()
    assert all(co.bits([t["value_sum"][i, k]])[0] == co.bits([value])[0] for i, k in leaf)
    ev = _Constant(value, reward, priors)
    trees = [_oracle_tree(t, i, legal[i], A) for i in range(B)]
    roots = [list(legal[i]) for i in range(B)]
    tp = numpy.zeros(B, numpy.int64)
    for r in range(3):
        acts = [_pick(res, None, i, r, roots[i]) for i in range(B)]
        tp = numpy.array([(tp[i] + 1) % P if a >= 0 else tp[i] for i, a in enumerate(acts)])
        ora_rngs = [numpy.random.RandomState() for _ in range(B)]
        for i in range(B):
            ora_rngs[i].set_state(rngs[i].get_state())
        trees = [co.carry(trees[i], cfg, acts[i]) for i in range(B)]
        for i in range(B):
            co.continue_search(cfg, ev, trees[i], int(tp[i]), True, ora_rngs[i])
        res = engine.continue_search(acts, list(tp), True, rngs)
        assert engine.kernel_name(B) == kernel
        got = engine.export_trees(B)
        got.update(visits=res.visit_counts, root_value=res.root_values,
                   info=numpy.stack([res.max_tree_depth, res.flags, res.tape_used, res.sum_depth], 1))
        for i in range(B):
            co.assert_tree_equal(got, i, trees[i], A)
            assert numpy.array_equal(rngs[i].get_state()[1], ora_rngs[i].get_state()[1]) and \
                rngs[i].get_state()[2] == ora_rngs[i].get_state()[2], i
        roots = [trees[i].actions[0] for i in range(B)]


# ---------------------------------------------------------------- 4. capacity edges

def _fresh_then_root_again(engine, cfg, net, B, to_play=0):
    obs = synthetic.observations(B, net.input_shape, seed=8)
    rngs = [numpy.random.RandomState(70 + i) for i in range(B)]
    engine.run(list(obs), [list(cfg.action_space)] * B, [0] * B, True, rngs)
    return engine.continue_search([-1] * B, [to_play] * B, True, rngs), engine.export_trees(B)


def test_capacity_edges(backend):
    S, B = 10, 64
    cfg = configs.cartpole(num_simulations=S)
    net = _net(cfg, 5)
    # a carried tree of S + 1 nodes and S more simulations fill a capacity of 2 S + 2 exactly (one slot stays free for the
    # leaf index of a simulation past the last)
    got = []
    for mode in (None, 0):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=S + 1)
        assert engine.num_nodes == 2 * S + 2
        res, t = _fresh_then_root_again(engine, cfg, net, B)
        assert (engine.kernel_name(B) == FC2) == (mode is None), engine.kernel_name(B)
        assert (t["n_nodes"] == 2 * S + 1).all() and (res.flags == 0).all()
        got.append((res, t, None, None))
    _assert_same(got[0], got[1], "exact capacity")
    # one node slot less: refused before any simulation, the per-operator path's error text
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=S)
    with pytest.raises(_lib.MzxError, match=f"carries {S + 1} nodes; with {S} simulations it needs {2 * S + 2} node slots, "
                                            f"the handle has {2 * S + 1}"):
        _fresh_then_root_again(engine, cfg, net, B)
    # to_play of a carried root differs
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=2 * S)
    with pytest.raises(_lib.MzxError, match="to_play 1 of tree 0 differs"):
        _fresh_then_root_again(engine, cfg, net, B, to_play=1)


def test_capacity_beyond_fc2_lds_falls_back(backend):
    S, B = 20, 64
    cfg = configs.cartpole(num_simulations=S)
    net = _net(cfg, 6)
    big = 4000
    outs = {}
    for mode in (None, 0):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=big)
        outs[mode] = _chain(engine, cfg, net, B, 2, 17)
    small = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=2 * S)
    assert _route(small, B)[0] == 4
    assert all(PER_OPERATOR in k and rt[0] == 0 for _, _, k, rt in outs[None]), [(k, rt) for _, _, k, rt in outs[None]]
    for a, b in zip(outs[None], outs[0]):
        _assert_same(a, b, "capacity beyond fc2's LDS")


# ---------------------------------------------------------------- 5. run_from_trees

@pytest.mark.parametrize("game,B,S,kernel", [("cartpole", 1024, 50, FC2), ("connect4", 256, 200, RT)])
def test_loaded_trees_continue_like_the_device_carry(backend, game, B, S, kernel):
    cfg = configs.BY_NAME[game](num_simulations=S)
    net = _net(cfg, 9)
    got = []
    for path in ("advance", "load"):
        engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=S + 1)
        obs = synthetic.observations(B, net.input_shape, seed=4)
        legal = [list(cfg.action_space)] * B
        rngs = [numpy.random.RandomState(300 + i) for i in range(B)]
        res = engine.run(list(obs), legal, [0] * B, True, rngs)
        assert engine.kernel_name(B) == kernel
        acts = [int(numpy.argmax(res.visit_counts[i])) if i % 3 else -1 for i in range(B)]
        P = len(cfg.players)
        tp = [(1 % P) if a >= 0 else 0 for a in acts]
        if path == "advance":
            res2 = engine.continue_search(acts, tp, True, rngs)
        else:
            trees = engine.export_trees(B)
            roots = [engine.node_graph(B, i, legal[i], _trees=trees) for i in range(B)]
            roots = [r.children[a] if a >= 0 else r for r, a in zip(roots, acts)]
            res2 = engine.run_from_trees(roots, tp, True, rngs)
        assert engine.kernel_name(B) == kernel
        torch.cuda.synchronize()
        got.append((res2, engine.export_trees(B)))
    (ra, ta), (rb, tb) = got
    assert numpy.array_equal(ra.visit_counts, rb.visit_counts) and numpy.array_equal(ra.root_values, rb.root_values)
    assert numpy.array_equal(ra.max_tree_depth, rb.max_tree_depth) and numpy.array_equal(ra.tape_used, rb.tape_used)
    for k in ("visit", "value_sum", "reward", "to_play", "parent", "minmax", "n_nodes"):
        assert numpy.array_equal(ta[k], tb[k]), k
    for i in range(B):       # slots past a node's children are padding
        n = int(ta["n_nodes"][i])
        assert numpy.array_equal(ta["child"][i, :n], tb["child"][i, :n])
        assert numpy.array_equal(ta["prior"][i, 1:n], tb["prior"][i, 1:n])
