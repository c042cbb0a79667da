"""
Continued searches on the MI355X (CPU twin: tests/test_search_continue.py):
  * tree_advance_kernel + the continued root preparation + the lock-step simulations against the oracle helper
    (tests/continue_oracle.py), bit for bit, chained, for the action spaces of cartpole (2), tictactoe (9), connect4 (7)
    and games/gomoku.py (121), with tie-prone priors;
  * network-driven continue_search: the streamed row route (games/gomoku.py-class networks) against the per-operator
    path, identical trees;
  * tree_advance_kernel against the host flattening of node_graph (run_from_trees): identical trees at size;
  * three chained continuations of every tree.
"""
import numpy
import pytest
import torch

from mzx import _lib, configs, models, self_play, synthetic

import test_search_continue as cpu
from test_search_continue import _carry_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.mark.parametrize("game,B,S,noise,ties", [("cartpole", 32, 50, True, False), ("tictactoe", 16, 20, True, True),
                                                 ("connect4", 16, 30, False, True), ("gomoku", 8, 10, True, False)])
def test_device_chained_continuations_equal_helper(backend, game, B, S, noise, ties):
    trees = _carry_case(backend, game, B, S, 3, noise, ties, seed=3)
    assert all(len(t.visit) > S for t in trees)


@pytest.mark.parametrize("game,noise,ties", cpu.CHAINS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_device_ragged_roots_mixed_players_equal_helper(backend, game, noise, ties):
    """GPU twin of test_hostcheck_ragged_roots_mixed_players_equal_helper: tree_advance_kernel, ContinueRootOp and the
    lock-step simulations on ragged legal sets (a single-action root), both players, the old root and a child in the same
    shard and round -- action spaces 2, 4, 9, 32 and 121 against the oracle helper, bit for bit."""
    B, S = 16, 12
    cfg = cpu._config(game, S)
    log = []
    _carry_case(backend, game, B, S, 3, noise, ties, pick=cpu.pick_alternating, seed=5, ragged=True, mixed_to_play=True, log=log)
    cpu.assert_root_shapes(log, len(cfg.action_space), len(cfg.players), B)


@pytest.mark.parametrize("game,ties", cpu.LATE, ids=lambda v: getattr(v, "__name__", str(v)))
def test_device_carry_starts_past_the_first_chunk(backend, game, ties):
    """GPU twin of test_hostcheck_carry_starts_past_the_first_chunk: a new root at an old node index >= 64 (the chunk loop
    of tree_advance_kernel starts at `c & ~63`) next to trees that carry more than 64 nodes."""
    log = []
    _carry_case(backend, game, 6, 20, 4, True, ties, pick=lambda r, i, t: -1 if i % 2 else cpu.pick_late_child(r, i, t), seed=9,
                ragged=True, mixed_to_play=True, log=log)
    assert max(log[3]["chosen"]) >= 64, log[3]["chosen"]
    assert max(log[3]["carried"]) > 64


@pytest.mark.parametrize("game", ["tictactoe", "lunarlander"])
def test_device_bad_carry_keeps_the_old_root_and_flags_it(backend, game):
    """GPU twin of test_hostcheck_bad_carry_keeps_the_old_root_and_flags_it (TF_BAD_CARRY through the lock-step ABI)."""
    cpu.bad_carry_lockstep(backend, game, 9, 3 if game == "tictactoe" else 2)


def _net(cfg, seed):
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), seed))
    return net


def _chain(engine, cfg, net, B, rounds, seed, export=True):
    obs = synthetic.observations(B, net.input_shape, seed=seed)
    legal = [list(cfg.action_space)] * B
    rngs = [numpy.random.RandomState(seed + i) for i in range(B)]
    res = engine.run(list(obs), legal, [0] * B, True, rngs)
    to_play = numpy.zeros(B, numpy.int64)
    out = []
    P = len(cfg.players)
    for r in range(rounds):
        acts = [int(numpy.argmax(res.visit_counts[i])) if (i + r) % 4 else -1 for i in range(B)]
        to_play = numpy.array([(to_play[i] + 1) % P if a >= 0 else to_play[i] for i, a in enumerate(acts)])
        before = res
        res = engine.continue_search(acts, list(to_play), True, rngs)
        assert (res.flags == 0).all()
        # every continued simulation passes the new root once; the root's children keep what they had
        for i, a in enumerate(acts):
            if a < 0:
                assert res.visit_counts[i].sum() == before.visit_counts[i].sum() + engine.num_simulations
        assert numpy.isfinite(res.root_values).all()
        out.append((res, engine.export_trees(B) if export else None, engine.kernel_name(B)))
    return out


def test_streamed_row_route_continues_like_the_per_operator_path(backend):
    cfg = configs.gomoku(num_simulations=10)
    net = _net(cfg, 5)
    B = 8
    outs = {}
    for mode in (None, 0):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=40)
        outs[mode] = _chain(engine, cfg, net, B, 3, 21)
    assert all("row_select" in k for _, _, k in outs[None]), [k for _, _, k in outs[None]]
    assert all("one-thread-per-tree" in k for _, _, k in outs[0]), [k for _, _, k in outs[0]]
    for (ra, ta, _), (rb, tb, _) in zip(outs[None], outs[0]):
        assert numpy.array_equal(ra.visit_counts, rb.visit_counts) and numpy.array_equal(ra.root_values, rb.root_values)
        for k in ta:
            assert numpy.array_equal(ta[k], tb[k]), k


def _fc_e10_a6(num_simulations):
    """A fully connected network with ten hidden features (no multiple of four: tree_advance_kernel copies the hidden rows
    float by float) and six actions."""
    return configs.cartpole(action_space=list(range(6)), encoding_size=10, num_simulations=num_simulations)


@pytest.mark.parametrize("game,B,S", [("cartpole", 1024, 50), ("connect4", 256, 200), ("fc_e10_a6", 64, 80)])
def test_advance_kernel_equals_host_flattening(backend, game, B, S):
    """fc_e10_a6: ragged legal sets, more than one 64-node chunk carried, and the hidden states of the kept nodes as well --
    node j of the advance path against node j of the load path over every tree's n_nodes rows."""
    scalar_rows = game == "fc_e10_a6"
    cfg = _fc_e10_a6(S) if scalar_rows else configs.BY_NAME[game](num_simulations=S)
    net = _net(cfg, 9)
    A = len(cfg.action_space)
    got = []
    for path in ("advance", "load"):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=0, max_carried_nodes=S + 1)
        obs = synthetic.observations(B, net.input_shape, seed=4)
        legal = cpu.ragged_legal(A, B, 14) if scalar_rows else [list(cfg.action_space)] * B
        rngs = [numpy.random.RandomState(300 + i) for i in range(B)]
        res = engine.run(list(obs), legal, [0] * B, True, rngs)
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
        torch.cuda.synchronize()
        hidden = None
        if scalar_rows:
            off, N, Hf = engine.arena_offsets(B), engine.num_nodes, net.hidden_size
            assert Hf % 4 != 0
            hidden = engine.arena(B)[off["hidden"]: off["hidden"] + B * N * Hf * 4].view(torch.int32).view(B, N, Hf).cpu().numpy()
        got.append((res2, engine.export_trees(B), hidden))
    (ra, ta, ha), (rb, tb, hb) = got
    assert numpy.array_equal(ra.visit_counts, rb.visit_counts) and numpy.array_equal(ra.root_values, rb.root_values)
    assert numpy.array_equal(ra.max_tree_depth, rb.max_tree_depth)
    for k in ("visit", "value_sum", "reward", "to_play", "parent", "minmax", "n_nodes"):
        assert numpy.array_equal(ta[k], tb[k]), k
    for i in range(B):       # slots past a node's children are padding
        n = int(ta["n_nodes"][i])
        assert numpy.array_equal(ta["child"][i, :n], tb["child"][i, :n])
        assert numpy.array_equal(ta["prior"][i, 1:n], tb["prior"][i, 1:n])
        if scalar_rows:
            assert numpy.array_equal(ha[i, :n], hb[i, :n]), i
    if scalar_rows:
        assert (ta["n_nodes"] - S > 64).any() and len({len(a) for a in legal}) > 1 and min(len(a) for a in legal) == 1


def test_three_chained_continuations(backend):
    cfg = configs.cartpole(num_simulations=30)
    net = _net(cfg, 2)
    B = 64
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=3 * 30 + 1)
    outs = _chain(engine, cfg, net, B, 3, 8)
    for res, t, _ in outs:
        assert (t["n_nodes"] <= engine.num_nodes).all() and (t["n_nodes"] > 30).all()
        # the root's visits: one per simulation through it (its own expansion included when it was a child)
        assert (t["visit"][:, 0] >= res.visit_counts.sum(1)).all() and (t["visit"][:, 0] <= t["n_nodes"]).all()
        assert (t["visit"].sum(1) > 0).all()
