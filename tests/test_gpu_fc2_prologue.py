"""
The launch prologue of fc2_search_kernel ("Launch prologue"): every global input of a launch -- the
thread's table entry, the lane's weight rows (SmallNetCartpole), the tree's observation, its legal-action row, player and
noise row, or the caller's root -- is requested at kernel entry, AHEAD of the exit of rows without a tree, and waited for
once; load_row reads without guards (a lane without a neuron reads the layer's last row and selects zeros); the root's
action count is a row ballot of `legal[s] >= 0` and a count of trailing ones instead of a serial scan.

The yardstick is the per-operator path (mode 0: one thread per tree, none of the above): every result array and every array
of the exported trees bit for bit, the kernel asserted by name.  Shapes are the smallest at which what changed can go wrong,
at 8 simulations (12 for the continued chain):
  * trees 1 (fifteen rows of the workgroup exit behind the early reads, which index a clamped tree), 3 and 5 (a partial
    wave; a second wave with one live row), 16 (an exact workgroup), 17 (a second workgroup with one tree);
  * SmallNetCartpole (mode 3) and LdsNet (mode 7) with two actions, LdsNet with three (four-lane records) and with six
    actions (sixteen-lane records: lanes 6 .. 15 read a clamped entry of the legal-action and noise rows);
  * legal sets: full; exactly one legal action (of varying index); for six actions the lengths 1 .. 6 within one batch, so
    that the ballot count meets every prefix length;
  * exploration noise on and off (off: a null noise pointer);
  * two players, the player to move alternating over the batch;
  * a fresh search, the caller's roots (mzx_search_run_from_roots) and one continued search on a handle with spare capacity.
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
S = 8
TREES = [1, 3, 5, 16, 17]


def _two_actions(**kw):
    return configs.cartpole(players=[0, 1], **kw)


def _wide(A):
    make = shapes._lds16(A)
    return lambda **kw: make(players=[0, 1], **kw)


#        engine: config factory, fc2 mode, actions
ENGINES = {
    "small-a2": (_two_actions, 3, 2),
    "lds-a2": (_two_actions, 7, 2),
    "lds-a3": (_wide(3), 3, 3),       # (mode 3 = the whole-search kernel with the tree export; not cartpole's shape: LdsNet)
    "lds-a6": (_wide(6), 3, 6),
}
_nets = {}      # config factory -> (config, network): "small-a2" and "lds-a2" share theirs, hence their yardsticks
_made = {}      # (config factory, legal, noise, B) -> inputs and the per-operator path's result: computed once, never changed


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _net(make, simulations=S):
    if (make, simulations) not in _nets:
        cfg = make(num_simulations=simulations)
        assert len(cfg.players) == 2
        _nets[make, simulations] = (cfg, shapes.whole._net(cfg, 11))
    return _nets[make, simulations]


def _legal(kind, A, B):
    if kind == "full":
        return [list(range(A))] * B
    if kind == "one":
        return [[(i + 1) % A] for i in range(B)]
    assert kind == "ragged" and A == 6
    # every prefix length 1 .. 6 (B = 1: the single length 3); sorted subsets that are not prefixes of 0 .. A - 1
    return [sorted(numpy.random.RandomState(50 + i).choice(A, size=(i + 2) % A + 1, replace=False).tolist()) for i in range(B)]


def _search(cfg, net, mode, B, obs, legal, to_play, noise):
    engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
    res = engine.run(list(obs), legal, to_play, noise, [numpy.random.RandomState(900 + i) for i in range(B)])
    return res, engine.export_trees(B), engine.kernel_name(B)


def _yardstick(make, A, kind, noise, B):
    key = (make, kind, noise, B)
    if key not in _made:
        cfg, net = _net(make)
        legal = _legal(kind, A, B)
        to_play = [i % 2 for i in range(B)]
        obs = synthetic.observations(B, net.input_shape, seed=B + 3)
        res, trees, kernel = _search(cfg, net, 0, B, obs, legal, to_play, noise)
        assert shapes.PER_OPERATOR in kernel, kernel
        assert (trees["n_nodes"] == S + 1).all() and (res.flags == 0).all()
        assert (trees["to_play"][:, 0] == numpy.array(to_play)).all()
        for i, acts in enumerate(legal):       # nothing outside the legal set was visited; every simulation counted
            assert res.visit_counts[i].sum() == S and res.visit_counts[i][acts].sum() == S
        if kind == "ragged" and B >= 6:
            assert {len(a) for a in legal} == set(range(1, A + 1))
        _made[key] = (cfg, net, obs, legal, to_play, res, trees)
    return _made[key]


def _assert_equal(want, want_trees, res, trees, skip=()):
    for key in RESULT_KEYS:
        if key not in skip:
            assert numpy.array_equal(_bits(getattr(want, key)), _bits(getattr(res, key))), key
    assert set(trees) == set(want_trees)
    for key, w in want_trees.items():
        assert numpy.array_equal(_bits(trees[key]), _bits(w)), key
    assert (res.flags == 0).all()


CASES = [(e, k) for e in sorted(ENGINES) for k in ("full", "one") + (("ragged",) if ENGINES[e][2] == 6 else ())]


@pytest.mark.parametrize("B", TREES)
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no-noise"])
@pytest.mark.parametrize("engine,kind", CASES, ids=[f"{e}-{k}" for e, k in CASES])
def test_fresh_search(backend, engine, kind, noise, B):
    make, mode, A = ENGINES[engine]
    cfg, net, obs, legal, to_play, want, want_trees = _yardstick(make, A, kind, noise, B)
    res, trees, kernel = _search(cfg, net, mode, B, obs, legal, to_play, noise)
    assert "fc2_search_kernel" in kernel, kernel
    _assert_equal(want, want_trees, res, trees)


@pytest.mark.parametrize("B", TREES)
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no-noise"])
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_given_roots(backend, engine, noise, B):
    """OVERRIDE: the caller's hidden states, priors and rewards in place of initial_inference; legal sets of every length
    from one action up in one batch (B = 1: a single action), the player to move alternating."""
    make, mode, A = ENGINES[engine]
    cfg, net = _net(make)
    outs = []
    for m in (0, mode):
        state = numpy.random.RandomState(11)
        roots = []
        for i in range(B):
            root = self_play.Node(0)
            hidden = torch.as_tensor(state.rand(1, net.hidden_size).astype(numpy.float32))
            logits = torch.as_tensor(state.randn(1, A).astype(numpy.float32))
            acts = sorted(numpy.random.RandomState(70 + i).choice(A, size=i % A + 1, replace=False).tolist())
            root.expand(acts, i % 2, [0.75, -1.5, 0.0][i % 3], logits, hidden)
            roots.append(root)
        eng = self_play.BatchedMCTS(cfg, net, B, mode=m)
        res = eng.run_from_roots(roots, [i % 2 for i in range(B)], noise, [numpy.random.RandomState(500 + i) for i in range(B)])
        outs.append((res, eng.export_trees(B), eng.kernel_name(B)))
    (want, want_trees, k0), (res, trees, kernel) = outs
    assert shapes.PER_OPERATOR in k0 and "fc2_search_kernel" in kernel, (k0, kernel)
    _assert_equal(want, want_trees, res, trees, skip=("root_predicted_values",))      # (none: the roots were given)
    assert (res.visit_counts.sum(1) == S).all()
    assert (want_trees["reward"][:, 0] == numpy.array([[0.75, -1.5, 0.0][i % 3] for i in range(B)])).all()


@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no-noise"])
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_continued_search(backend, engine, noise):
    """A fresh search and one continuation at five trees on a handle with spare capacity: the CONT instantiation requests
    tables and weights only and takes its roots from the arena; the fresh launch of the same handle exports its trees."""
    make, mode, A = ENGINES[engine]
    B, S2 = 5, 12
    cfg, net = _net(make, S2)
    legal = shapes.ragged_legal(A, B, 23)
    to_play = [i % 2 for i in range(B)]
    outs = {}
    mode = None if mode == 3 else mode      # (the handle's own choice; a handle with spare capacity always exports)
    for m, check in ((mode, shapes._is(shapes.FC2, 4)), (0, shapes._is(shapes.PER_OPERATOR, 0))):
        eng = self_play.BatchedMCTS(cfg, net, B, mode=m, max_carried_nodes=3 * S2)
        outs[m] = shapes._chain(eng, cfg, net, B, 1, 31, legal, to_play, check, noise=noise)
    shapes._assert_same(outs[mode], outs[0], engine)
    assert outs[0][-1][1]["n_nodes"].max() > S2 + 1
