"""
The route table of the three search entries on the MI355X: which kernels mzx_search_run, mzx_search_run_from_roots and
mzx_search_run_continued launch (mzx_search_kernel_name) for every cell of
    (network class) x (search mode: the handle's default / 0 = per-operator) x (spare node capacity) x (how the roots arrive),
and whether mzx_search_advance takes the trees a from-roots search of a spare-capacity handle left.  One decision in the
library (search_choice, csrc/mzx_lib.cpp) serves the three entries; a from-roots search does not follow the fresh route in every
cell, and this table is what says where.

EXPECTED was recorded by running observe() of this file against the library built from commit 91618a8 ("Run continued searches
in fc2_search_kernel and rt_search_kernel"), the last one whose mzx_search_run_from_roots chose its route with a chain of its
own -- not from the code under test; every cell of it passes against that library too.  Mode flag 16 (the first-generation fully connected kernel) exists in instrumented builds
only and is not part of the table.  Toy sizes: 4 trees x 3 simulations, synthetic weights.
"""
import numpy
import pytest
import torch

from mzx import _lib, configs, models, self_play, synthetic

pytestmark = pytest.mark.gpu

B, S = 4, 3

FC2, RT, RZ = "mzx::fc2_search_kernel", "mzx::rt_search_kernel", "mzx::rz_search_kernel"
WAVE, TILE = "mzx::rz_wave_search_kernel", "mzx::rz_tile_search_kernel"
PER_OP = "one kernel per step of a simulation (select / network / expand + back-propagate)"
_STREAMED = "mzx::rb_tower_kernel / mzx::rb_gemm_kernel / mzx::rb_gemm_multi_kernel (streamed FP32-MFMA trunks, layers, head MLP levels) between "
ROWS = _STREAMED + "mzx::row_select_kernel / mzx::row_expand_backprop_kernel"
PER_OP_STREAMED = _STREAMED + "one-thread-per-tree kernels"


def _tile_3x6():
    return configs.tictactoe(observation_shape=(3, 3, 6), action_space=list(range(6)), channels=16, blocks=1,
                             reduced_channels_reward=8, reduced_channels_value=8, reduced_channels_policy=8,
                             resnet_fc_reward_layers=[16], resnet_fc_value_layers=[16], resnet_fc_policy_layers=[16])


# network class: (configuration, tuning entries moved for the whole cell, network mode: None = the default engine)
CLASSES = {
    "fc-small": (configs.cartpole, {}, None),             # fully connected, SmallNet (register-resident weights)
    "fc-lds": (configs.lunarlander, {}, None),            # fully connected, LdsNet
    "res-wave": (configs.tictactoe, {}, None),            # narrow residual network, a wave per tree
    "res-tile": (_tile_3x6, {}, None),                    # narrow residual network, a row tile per wave
    "tower": (configs.connect4, {}, None),                # connect4 class: the tower arithmetic at every shard size
    "tower-launches": (configs.connect4, {"rt_search": 0}, None),     # ... launch by launch
    "tower-off": (configs.connect4, {"wide_towers": 0}, None),        # ... switched off: the LDS-resident engine
    "tower-streamed": (configs.connect4, {}, 3),    # ... every layer on the streamed engine (network mode 3)
    "streamed": (configs.gomoku, {}, None),         # fits the streamed engine only
}
MODES = (None, 0)
# carried node slots: none; room for one continuation of the root; (fully connected only) more than fc2_search_kernel's LDS holds
CAPACITIES = {"none": 0, "spare": 4 * S, "beyond-fc2": 4000}

# (class, mode, capacity) -> (fresh, from roots) without spare capacity,
#                            (fresh, continued, from roots, advance after from roots) with it
EXPECTED = {
    ("fc-small", None, "none"): (FC2, FC2),
    ("fc-small", None, "spare"): (FC2, FC2, PER_OP, "accepted"),
    ("fc-small", None, "beyond-fc2"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("fc-small", 0, "none"): (PER_OP, PER_OP),
    ("fc-small", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("fc-small", 0, "beyond-fc2"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("fc-lds", None, "none"): (FC2, FC2),
    ("fc-lds", None, "spare"): (FC2, FC2, PER_OP, "accepted"),
    ("fc-lds", None, "beyond-fc2"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("fc-lds", 0, "none"): (PER_OP, PER_OP),
    ("fc-lds", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("fc-lds", 0, "beyond-fc2"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("res-wave", None, "none"): (WAVE, WAVE),
    ("res-wave", None, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("res-wave", 0, "none"): (PER_OP, PER_OP),
    ("res-wave", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("res-tile", None, "none"): (TILE, TILE),
    ("res-tile", None, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("res-tile", 0, "none"): (PER_OP, PER_OP),
    ("res-tile", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("tower", None, "none"): (RT, RT),
    ("tower", None, "spare"): (RT, RT, PER_OP, "accepted"),
    ("tower", 0, "none"): (PER_OP, PER_OP),
    ("tower", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("tower-launches", None, "none"): (ROWS, ROWS),
    ("tower-launches", None, "spare"): (ROWS, ROWS, PER_OP, "accepted"),
    ("tower-launches", 0, "none"): (PER_OP, PER_OP),
    ("tower-launches", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("tower-off", None, "none"): (RZ, RZ),
    ("tower-off", None, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("tower-off", 0, "none"): (PER_OP, PER_OP),
    ("tower-off", 0, "spare"): (PER_OP, PER_OP, PER_OP, "accepted"),
    ("tower-streamed", None, "none"): (RT, RT),
    ("tower-streamed", None, "spare"): (RT, RT, ROWS, "accepted"),
    ("tower-streamed", 0, "none"): (PER_OP_STREAMED, PER_OP),
    ("tower-streamed", 0, "spare"): (PER_OP_STREAMED, PER_OP_STREAMED, PER_OP, "accepted"),
    ("streamed", None, "none"): (ROWS, ROWS),
    ("streamed", None, "spare"): (ROWS, ROWS, ROWS, "accepted"),
    ("streamed", 0, "none"): (PER_OP_STREAMED, PER_OP),
    ("streamed", 0, "spare"): (PER_OP_STREAMED, PER_OP_STREAMED, PER_OP, "accepted"),
}


def cells(name):
    for mode in MODES:
        for cap in CAPACITIES:
            if cap == "beyond-fc2" and not name.startswith("fc-"):
                continue
            yield mode, cap


_nets = {}


def _net(name):
    if name not in _nets:
        cfg = CLASSES[name][0]()
        cfg.num_simulations = S
        net = models.MuZeroNetwork(cfg)
        net.set_weights(synthetic.fill_state_dict(net.state_dict(), 5))
        if CLASSES[name][2] is not None:
            net.set_mode(CLASSES[name][2])
        _nets[name] = (cfg, net)
    return _nets[name]


def observe(backend, name, mode, cap):
    cfg, net = _net(name)
    legal = [list(cfg.action_space)] * B
    obs = synthetic.observations(B, net.input_shape, seed=3)
    rngs = [numpy.random.RandomState(40 + i) for i in range(B)]
    carried = CAPACITIES[cap]
    with backend.lib.tuning(**CLASSES[name][1]):
        _, _, policy, hidden = net.initial_inference(torch.tensor(obs))
        roots = []
        for i in range(B):
            node = self_play.Node(0)
            node.expand(legal[i], 0, 0.0, policy[i:i + 1].cpu(), hidden[i:i + 1])
            roots.append(node)
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=carried)
        out = []
        res = engine.run(list(obs), legal, [0] * B, True, rngs)
        assert (res.visit_counts.sum(1) == S).all()
        out.append(engine.kernel_name(B))
        if carried:
            res = engine.continue_search([-1] * B, [0] * B, True, rngs)
            assert (res.visit_counts.sum(1) == 2 * S).all()
            out.append(engine.kernel_name(B))
        res = engine.run_from_roots(roots, [0] * B, True, rngs)
        assert (res.visit_counts.sum(1) == S).all()
        out.append(engine.kernel_name(B))
        if carried:
            try:
                res = engine.continue_search([-1] * B, [0] * B, True, rngs)
                assert (res.visit_counts.sum(1) == 2 * S).all()
                out.append("accepted")
            except _lib.MzxError as e:
                assert "did not leave every node's hidden state" in str(e), e
                out.append("refused")
        torch.cuda.synchronize()
    return tuple(out)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_route_table(name):
    backend = _lib.default_backend()
    for mode, cap in cells(name):
        got = observe(backend, name, mode, cap)
        print(name, mode, cap, got)
        assert got == EXPECTED[(name, mode, cap)], (name, mode, cap, got)
