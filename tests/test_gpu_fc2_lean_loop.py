"""
The simulation loop of fc2_search_kernel after its row-uniform scalar work was cut ("Leaner loop"):
the inverse transform of the value and the reward head in ONE pass (even lanes the value, odd lanes the reward, a sign
branch per lane), a value chain in which every lane advances its own copy of the value and stops at its node (lane 0 hands
the value to the chunk above), operand reads of back-propagation without guards (lanes at and beyond the leaf read the
leaf's parent).  The yardstick is the per-operator path (mode 0: one thread per tree, none of the above): every exported
node and slot record, MinMaxStats, counter and result bit for bit, on both network engines of the kernel -- SmallNetCartpole
(mode 3) and the same network forced onto LdsNet (mode 7) -- at 1, 3, 5 and 17 trees (a lone row, a partial wave, a wave plus
one row, a workgroup plus one row).

The weights were chosen on the CPU oracle (oracle/mcts_oracle.py) before the tests relied on them: seed 32 decodes values AND
rewards of both signs at every tree count used here, with one and with two players; all-zero weights decode exactly zero and
tie at every level; seed 19 with the policy head's output bias at +20 / -20 grows a chain (deepest walk 35 .. 40 plies in
40 simulations: three 16-level chunks, the loop's copy of the value chain and two hand-overs).  Each property is asserted
again here on the yardstick's trees, so a case that no longer exercises its path fails instead of proving nothing.
"""
import numpy
import pytest
import torch

import test_gpu_continue_shapes as shapes
from mzx import _lib, configs, models, self_play, synthetic

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("visit_counts", "root_values", "root_predicted_values", "max_tree_depth", "sum_depth", "tape_used", "flags")


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _bits(a):
    return a.view(numpy.int64) if a.dtype == numpy.float64 else a


def _weights(cfg, kind):
    net = models.MuZeroNetwork(cfg)
    sd = synthetic.fill_state_dict(net.state_dict(), 19 if kind == "chain" else 32)
    if kind == "zero":
        sd = {k: torch.zeros_like(v) for k, v in sd.items()}
    if kind == "chain":
        last = [k for k in sd if "policy" in k and k.endswith(".bias")][-1]
        sd[last] = torch.tensor([20.0, -20.0], dtype=sd[last].dtype)
    net.set_weights(sd)
    return net


#      case: players, weights, simulations (12 tied simulations stay within the tape's 16 words), ragged legal sets
CASES = {
    "signs": ([0], "signs", 16, True),
    "signs-two-players": ([0, 1], "signs", 16, True),
    "ties": ([0], "zero", 12, True),
    "ties-two-players": ([0, 1], "zero", 12, True),
    "chain": ([0], "chain", 40, False),
    "chain-two-players": ([0, 1], "chain", 40, False),
}
_made = {}      # (case, B) -> inputs and the per-operator path's result: computed once, shared by both engines, never changed


def _search(cfg, net, mode, B, obs, legal, to_play):
    engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
    res = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(900 + i) for i in range(B)])
    return res, engine.export_trees(B), engine.kernel_name(B)


def _yardstick(case, B):
    if (case, B) not in _made:
        players, kind, S, ragged = CASES[case]
        cfg = configs.cartpole(players=players, num_simulations=S)
        net = _weights(cfg, kind)
        A = len(cfg.action_space)
        rs = numpy.random.RandomState(B)
        legal = [list(cfg.action_space) if not ragged or i % 4 != 3
                 else sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for i in range(B)]
        to_play = [int(i % len(players)) for i in range(B)]
        obs = synthetic.observations(B, net.input_shape, seed=B + 3)
        res, trees, _ = _search(cfg, net, 0, B, obs, legal, to_play)
        n = trees["n_nodes"]
        assert (n == S + 1).all() and (res.flags == 0).all()
        inner = numpy.arange(trees["visit"].shape[1])[None, :] < n[:, None]
        inner[:, 0] = False
        reward = trees["reward"][inner]
        leaves = trees["value_sum"][inner & (trees["visit"] == 1)]     # a node visited once holds its decoded value
        print(f"{case} B={B}: rewards +{(reward > 0).sum()} -{(reward < 0).sum()} 0:{(reward == 0).sum()}, leaf values "
              f"+{(leaves > 0).sum()} -{(leaves < 0).sum()} 0:{(leaves == 0).sum()}, deepest walks {res.max_tree_depth.min()} .. "
              f"{res.max_tree_depth.max()}, tape words {res.tape_used.min()} .. {res.tape_used.max()}")
        if kind == "signs":
            assert (reward > 0).any() and (reward < 0).any() and (leaves > 0).any() and (leaves < 0).any()
        if kind == "zero":
            assert (reward == 0).all() and (leaves == 0).all() and (res.tape_used >= 4).all()
        if kind == "chain":
            assert (res.max_tree_depth >= 33).all(), res.max_tree_depth
        assert res.tape_used.max() <= self_play.TAPE_WORDS        # no tree was searched again in another launch
        _made[case, B] = (cfg, net, obs, legal, to_play, res, trees)
    return _made[case, B]


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("mode", [3, 7], ids=["small", "lds"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fc2_kernel_equals_the_per_operator_path(backend, case, mode, B):
    cfg, net, obs, legal, to_play, want, want_trees = _yardstick(case, B)
    res, trees, kernel = _search(cfg, net, mode, B, obs, legal, to_play)
    assert "fc2_search_kernel" in kernel, kernel
    for key in RESULT_KEYS:
        assert numpy.array_equal(_bits(getattr(want, key)), _bits(getattr(res, key))), key
    for key, w in want_trees.items():       # node and slot records, MinMaxStats, node counts
        assert numpy.array_equal(_bits(trees[key]), _bits(w)), key
    assert (res.visit_counts.sum(1) == cfg.num_simulations).all()


@pytest.mark.parametrize("players", [[0], [0, 1]], ids=["one-player", "two-players"])
def test_given_roots(backend, players):
    """OVERRIDE at five trees: the caller's hidden states, priors and rewards (both signs and zero) replace
    initial_inference; one root has a single legal action."""
    B, S = 5, 16
    cfg = configs.cartpole(players=players, num_simulations=S)
    net = _weights(cfg, "signs")
    outs = []
    for mode in (0, 3):
        roots = []
        state = numpy.random.RandomState(11)
        for i in range(B):
            root = self_play.Node(0)
            hidden = torch.as_tensor(state.rand(1, net.hidden_size).astype(numpy.float32))
            logits = torch.as_tensor(state.randn(1, len(cfg.action_space)).astype(numpy.float32))
            root.expand(cfg.action_space if i != 3 else [1], i % len(players), [0.75, -1.5, 0.0][i % 3], logits, hidden)
            roots.append(root)
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        res = engine.run_from_roots(roots, [i % len(players) for i in range(B)], True,
                                    [numpy.random.RandomState(500 + i) for i in range(B)])
        outs.append((res, engine.export_trees(B), engine.kernel_name(B)))
    (r0, t0, _), (r1, t1, kernel) = outs
    assert "fc2_search_kernel" in kernel, kernel
    for key in RESULT_KEYS:
        if key != "root_predicted_values":      # (none: the roots were given)
            assert numpy.array_equal(_bits(getattr(r0, key)), _bits(getattr(r1, key))), key
    for key, w in t0.items():
        assert numpy.array_equal(_bits(t1[key]), _bits(w)), key
    assert (r1.visit_counts.sum(1) == S).all() and (r1.flags == 0).all()
    assert (t0["reward"][:, 0] == numpy.array([0.75, -1.5, 0.0, 0.75, -1.5])).all()


@pytest.mark.parametrize("mode", [None, 7], ids=["small", "lds"])
def test_continued_search(backend, mode):
    """A fresh search and two continuations at five trees, two players: the arena import in place of the prologue, walks
    that start in a carried tree."""
    B, S = 5, 12
    cfg = configs.cartpole(players=[0, 1], num_simulations=S)
    net = _weights(cfg, "signs")
    legal = [list(cfg.action_space)] * B
    to_play = [i % 2 for i in range(B)]
    outs = {}
    for m, check in ((mode, shapes._is(shapes.FC2, 4)), (0, shapes._is(shapes.PER_OPERATOR, 0))):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=m, max_carried_nodes=3 * S)
        outs[m] = shapes._chain(engine, cfg, net, B, 2, 31, legal, to_play, check)
    shapes._assert_same(outs[mode], outs[0], "continued")
    assert outs[0][-1][1]["n_nodes"].max() > S + 1
