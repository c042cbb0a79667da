"""
fc2_search_kernel with 64-bit DPP operands ("64-bit DPP operands"): in the two-action instantiations
binary64 row broadcasts are ONE v_mov_b64_dpp (bcast_d64: the walk's two scores, the chunk hand-over, carry_inv) and the value
chain takes the reward as the DPP operand of its addition (v_fmac_f64_dpp with a multiplier of one: a step is mul, add, the
next step's compare, two selects).  The four- and sixteen-lane instantiations keep two 32-bit moves and the plain addition
behind the same compile-time switch, so they are run here too.

The yardstick is the per-operator path (mode 0); every array of export_trees and every result bit for bit on both engines
(SmallNetCartpole, mode 3; LdsNet, mode 7) at 1, 3, 5 and 17 trees, the kernel asserted by name.  The weight cases and their
yardstick cache are those of tests/test_gpu_fc2_lean_loop.py.  The chain case is the one that matters here: at 33 plies and
more it walks every step of the value chain (1 to 15), all three guarded groups, the loop's copy for further chunks and the
hand-over broadcast.  New here: discount 1 (the multiply of a step is the identity, the addition is all that rounds) and two
players, where r_eff is +reward for the path nodes of one player and -reward for the other's: the precondition asserts that
some backed-up path holds nodes of both players with non-zero rewards, so that both forms of the sign select feed the DPP
operand within one chain; the four- and sixteen-lane record instantiations (A = 3 and A = 6) at five trees.
"""
import numpy
import pytest

import test_gpu_continue_shapes as shapes
import test_gpu_fc2_lean_loop as lean
from mzx import _lib, configs, self_play, synthetic

pytestmark = pytest.mark.gpu

RESULT_KEYS = lean.RESULT_KEYS
_bits = lean._bits
_extra = {}     # (case, B) -> inputs and the per-operator path's result, computed once and never changed


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _assert_equal(want, want_trees, res, trees):
    for key in RESULT_KEYS:
        assert numpy.array_equal(_bits(getattr(want, key)), _bits(getattr(res, key))), key
    assert set(trees) == set(want_trees)
    for key, w in want_trees.items():
        assert numpy.array_equal(_bits(trees[key]), _bits(w)), key
    assert (res.flags == 0).all()


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [3, 7], ids=["small", "lds"])
@pytest.mark.parametrize("case", sorted(lean.CASES))
def test_weight_cases(backend, case, mode, B):
    """Both signs with one and two players, all ties, the chain of 33 plies and more."""
    cfg, net, obs, legal, to_play, want, want_trees = lean._yardstick(case, B)
    if lean.CASES[case][1] == "chain":       # every step of the chain, three chunks, two hand-overs
        assert (want.max_tree_depth >= 33).all(), want.max_tree_depth
    res, trees, kernel = lean._search(cfg, net, mode, B, obs, legal, to_play)
    assert "fc2_search_kernel" in kernel, kernel
    _assert_equal(want, want_trees, res, trees)
    assert (res.visit_counts.sum(1) == cfg.num_simulations).all()


def _node_depths(trees, i):
    """Depth of every node of tree i from its parent links (root: 0)."""
    n = int(trees["n_nodes"][i])
    parent = trees["parent"][i]
    depth = numpy.zeros(n, numpy.int64)
    for k in range(1, n):                     # a node's index is above its parent's
        assert 0 <= parent[k] < k
        depth[k] = depth[parent[k]] + 1
    return depth


#        case: players, discount
EXTRA = {
    "discount-one": ([0], 1.0),
    "two-players-both-parities": ([0, 1], 0.997),
}


def _extra_yardstick(case, B):
    if (case, B) not in _extra:
        players, discount = EXTRA[case]
        S = 16
        cfg = configs.cartpole(players=players, num_simulations=S, discount=discount)
        assert cfg.discount == discount
        net = lean._weights(cfg, "signs")
        legal = [list(cfg.action_space)] * B
        to_play = [int(i % len(players)) for i in range(B)]
        obs = synthetic.observations(B, net.input_shape, seed=B + 3)
        res, trees, _ = lean._search(cfg, net, 0, B, obs, legal, to_play)
        assert (trees["n_nodes"] == S + 1).all() and (res.flags == 0).all()
        assert (res.max_tree_depth >= 2).all()
        # the precondition (two players): players alternate by depth, and back-propagation from a leaf takes +reward at the
        # path nodes of one player and -reward at the other's.  A node k with a non-zero reward whose parent (below the root)
        # has one too was a leaf whose chain read both forms of r_eff, side by side in lanes depth - 1 and depth; both signs
        # of the reward itself occur as well
        both_forms, signs = 0, set()
        for i in range(B):
            depth = _node_depths(trees, i)
            reward, parent = trees["reward"][i], trees["parent"][i]
            for k in range(1, len(depth)):
                if reward[k] != 0:
                    signs.add(bool(reward[k] > 0))
                    both_forms += int(depth[k] >= 2 and reward[parent[k]] != 0)
        print(f"{case} B={B}: leaves with both forms of r_eff on their path {both_forms}, reward signs {sorted(signs)}, "
              f"deepest walks {res.max_tree_depth.min()} .. {res.max_tree_depth.max()}")
        assert len(players) == 1 or (both_forms > 0 and signs == {False, True})
        _extra[case, B] = (cfg, net, obs, legal, to_play, res, trees)
    return _extra[case, B]


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [3, 7], ids=["small", "lds"])
@pytest.mark.parametrize("case", sorted(EXTRA))
def test_discount_one_and_leaf_parities(backend, case, mode, B):
    cfg, net, obs, legal, to_play, want, want_trees = _extra_yardstick(case, B)
    res, trees, kernel = lean._search(cfg, net, mode, B, obs, legal, to_play)
    assert "fc2_search_kernel" in kernel, kernel
    _assert_equal(want, want_trees, res, trees)
    assert (res.visit_counts.sum(1) == cfg.num_simulations).all()


#        name: config factory, number of actions
WIDE = {
    "three-actions": (shapes._lds16(3), 3),     # A = 3: the four-lane records (pick by DPP, dead slot row)
    "six-actions": (shapes._lds16(6), 6),       # 4 < A <= 16: the sixteen-lane records (row_max_d, generic walk and refresh)
}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wider_records(backend, name):
    """The other side of the compile-time switch (D64 = false): four- and sixteen-lane records at five trees, ragged legal sets, a fresh search and one
    continuation against the per-operator path."""
    B, S = 5, 12
    make, A = WIDE[name]
    cfg = make(num_simulations=S)
    P = len(cfg.players)
    assert len(cfg.action_space) == A
    net = shapes.whole._net(cfg, 11)
    legal = shapes.ragged_legal(A, B, 23)
    assert len({len(a) for a in legal}) > 1
    to_play = [i % P for i in range(B)]
    outs = {}
    for m, check in ((None, shapes._is(shapes.FC2, 4)), (0, shapes._is(shapes.PER_OPERATOR, 0))):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=m, max_carried_nodes=3 * S)
        outs[m] = shapes._chain(engine, cfg, net, B, 1, 31, legal, to_play, check)
    shapes._assert_same(outs[None], outs[0], name)

