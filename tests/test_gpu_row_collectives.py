"""
The row collectives of csrc/mzx_fused_fc.h (DPP moves inside a tree's 16-lane row: broadcasts, butterflies, picks) at the
shapes where one can go wrong -- waves whose other rows have left the kernel, both network engines of fc2_search_kernel, the
2-, 4- and 16-lane child records, ties at every level, two players, a walk deeper than a row -- and one small case each on
the other routes that share them.  The yardstick is the per-operator path (one thread per tree, no row collective): every
exported tree statistic, MinMaxStats and counter bit for bit.
"""
import numpy
import pytest
import torch

import test_gpu_parity as parity
import test_gpu_streamed as streamed
import trainer_loss_cases
from mzx import _lib, configs, models, self_play, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _bits(a):
    return a.view(numpy.int64) if a.dtype == numpy.float64 else a


def _same_trees(cfg, net, B, legal, to_play, modes, seed0=900, noise=True):
    """(result, trees) of modes[1] after comparing it with modes[0] field for field."""
    obs = synthetic.observations(B, net.input_shape, seed=B + 3)
    outs = []
    for mode in modes:
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        res = engine.run(list(obs), legal, to_play, noise, [numpy.random.RandomState(seed0 + i) for i in range(B)])
        outs.append((res, engine.export_trees(B), engine.kernel_name(B)))
    (r0, t0, _), (r1, t1, kernel) = outs
    for key in ("visit_counts", "root_values", "root_predicted_values", "max_tree_depth", "sum_depth", "tape_used", "flags"):
        assert numpy.array_equal(_bits(getattr(r0, key)), _bits(getattr(r1, key))), key
    for key, want in t0.items():     # node and slot records, MinMaxStats, node counts
        assert numpy.array_equal(_bits(t1[key]), _bits(want)), key
    assert (r1.visit_counts.sum(1) == cfg.num_simulations).all() and (r1.flags == 0).all()
    return r1, t1, kernel


def _fc_wide(num_actions, num_simulations=16):
    """A fully connected shape no register specialisation covers (tests/test_gpu_parity.py, other shapes)."""
    return configs.cartpole(action_space=list(range(num_actions)), stacked_observations=2, encoding_size=10,
                            fc_representation_layers=[12], fc_dynamics_layers=[24, 12], fc_reward_layers=[20],
                            fc_value_layers=[], fc_policy_layers=[33], num_simulations=num_simulations)


FC_CASES = {
    # SmallNet (register-resident weights, 2-lane records), forced onto LdsNet (mode flag 4), both players
    "small": (lambda: configs.cartpole(num_simulations=16), 3, False),
    "lds": (lambda: configs.cartpole(num_simulations=16), 7, False),
    "two-player": (lambda: configs.cartpole(players=[0, 1], num_simulations=16), 3, False),
    # 4 actions: pick_i<4>, row_max_d<4> and the ballot; 6 actions: row_max_d<16> and ds_bpermute
    "four-actions": (lambda: _fc_wide(4), 3, False),
    "six-actions": (lambda: _fc_wide(6), 3, False),
    # all-zero weights: every level of every walk is a tie (tape draws in the row); 12 simulations stay within the
    # tape's 16 words -- a tree that runs out is searched again in another launch, and the exported trees are gone
    "ties": (lambda: configs.cartpole(num_simulations=12), 3, True),
    "ties-four-actions": (lambda: _fc_wide(4, 12), 3, True),
}


@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("case", sorted(FC_CASES))
def test_fc2_kernel_trees_equal_the_per_operator_path(backend, case, B):
    """1, 3 and 5 trees: a wave with three, one and (second wave) three rows gone; 17: a second workgroup with one row."""
    make, mode, zero = FC_CASES[case]
    cfg = make()
    net = models.MuZeroNetwork(cfg)
    sd = synthetic.fill_state_dict(net.state_dict(), 19)
    net.set_weights({k: torch.zeros_like(v) for k, v in sd.items()} if zero else sd)
    A = len(cfg.action_space)
    rs = numpy.random.RandomState(B)
    legal = [list(cfg.action_space) if i % 4 != 3 else sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist())
             for i in range(B)]
    to_play = [int(i % len(cfg.players)) for i in range(B)]
    res, _, kernel = _same_trees(cfg, net, B, legal, to_play, (0, mode))
    assert "fc2_search_kernel" in kernel, kernel
    assert res.tape_used.max() <= self_play.TAPE_WORDS      # no tree was searched again: the trees compared are this run's
    if zero:
        assert (res.tape_used >= 4).all()       # the walks drew their ties from the tape


def test_fc2_walk_deeper_than_a_row(backend):
    """One action: every simulation lengthens the same line, 20 plies in 20 simulations -- back-propagation in two chunks
    of sixteen path nodes, the value handed from the leaf's chunk to the one above."""
    cfg = configs.cartpole(action_space=[0], num_simulations=20)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 5))
    B = 3
    res, trees, kernel = _same_trees(cfg, net, B, [[0]] * B, [0] * B, (0, 3))
    assert "fc2_search_kernel" in kernel, kernel
    assert (res.max_tree_depth == 20).all() and (trees["n_nodes"] == 21).all()


def test_tictactoe_on_the_wave_per_tree_kernel(backend):
    cfg = configs.tictactoe(num_simulations=12)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 21))
    B, A = 7, len(cfg.action_space)
    rs = numpy.random.RandomState(8)
    legal = [sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for _ in range(B)]
    parity._compare_modes(cfg, net, B, legal, [i % 2 for i in range(B)], True, [300 + i for i in range(B)])
    engine = self_play.BatchedMCTS(cfg, net, B)
    obs = synthetic.observations(B, net.input_shape, seed=B + 1)
    engine.run(list(obs), legal, [i % 2 for i in range(B)], True, [numpy.random.RandomState(300 + i) for i in range(B)])
    assert parity._kernel_name(backend, engine, B) == "mzx::rz_wave_search_kernel"


def test_connect4_row_walk(backend):
    """The row-per-tree kernels around the streamed engine (csrc/mzx_row_search.h): row_select / row_backprop."""
    backend.lib.tuning_set("rt_search", 0)       # per-simulation launches (conftest restores the default)
    cfg = streamed.STREAMED_CASES["connect4"][0]()
    cfg.num_simulations = 12
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 12))
    net.set_mode(3)
    B, A = 6, len(cfg.action_space)
    rs = numpy.random.RandomState(4)
    legal = [sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for _ in range(B)]
    _, _, kernel = _same_trees(cfg, net, B, legal, [i % 2 for i in range(B)], (0, 1))
    assert "row_select_kernel" in kernel, kernel


def test_trainer_loss_head(backend, golden_dir):
    case = trainer_loss_cases.CASES[0]
    trainer_loss_cases.check_case(backend, case, trainer_loss_cases.golden(golden_dir))
