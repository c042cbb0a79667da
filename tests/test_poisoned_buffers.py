"""
Poisoned arenas, workspaces and outputs on the serial build (tests/poison_cases.py has the method): the cells of the route
table the serial build routes -- every one of them on the per-operator path -- the network buffers, the trainers' scratch and
the sampler's workspace.  GPU twin, every route of the table: test_gpu_poisoned_buffers.py.
"""
import json

import pytest

import fc_train_cases
import hostcheck
import poison_cases as pc
import replay_sampler_cases
import resnet_stem_train_cases
import resnet_train_cases
import train_cases_common as common
import trainer_loss_cases
from mzx import configs
from test_gpu_route_table import CAPACITIES, CLASSES, PER_OP, cells


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


# the classes of the table whose networks the serial build runs in a second or two (the tuning entries and network modes of
# the others only pick device engines), and connect4's board, actions and two players on a narrow network: the serial
# build takes minutes over the 64-channel one
SERIAL = {k: CLASSES[k] for k in ("fc-small", "fc-lds", "res-wave", "res-tile")}
SERIAL["connect4-narrow"] = (lambda: configs.connect4(channels=16, blocks=1), {}, None)


@pytest.mark.parametrize("name", sorted(SERIAL))
def test_search_arena_and_outputs(backend, name):
    for mode, cap in cells(name):
        lines = pc.search_cell(backend, lambda n: pc.make_net(backend, SERIAL, n), name, mode, cap, SERIAL, CAPACITIES, per_op=PER_OP)
        entries = 4 if CAPACITIES[cap] else 3           # run, mzx_selfplay_search, from roots; carry + continue with capacity
        assert len(lines) == entries * len(pc.PATTERNS) and all(line.endswith("same") for line in lines)


# ------------------------------------------------------------------------------------------ trainers and the loss head

def _pinned(family):
    with open(common.bits.FAMILIES[family]["fixture"]) as f:
        return json.load(f)["serial"]


TRAIN_CASES = [(tables, kind, case) for tables, kind in ((fc_train_cases, "fc"), (resnet_train_cases, "resnet"),
                                                         (resnet_stem_train_cases, "resnet")) for case in pc.all_cases(tables)]


@pytest.mark.parametrize("tables,kind,case", TRAIN_CASES, ids=[f"{kind}-{case['name']}" for _, kind, case in TRAIN_CASES])
def test_trainer_scratch_and_outputs(backend, tables, kind, case):
    """mzx_train_fc_step / mzx_train_resnet_step: the gradient, losses, priorities, statistics and logits do not depend on what
    d_scratch held, every element of them is written, and the raw call under zeros gives the pinned bits."""
    assert len(pc.train_case(backend, tables, kind, case, _pinned(kind), kind)) == 3


def test_loss_head_scratch_and_outputs(backend):
    lines = pc.loss_table(backend, trainer_loss_cases)
    assert len(lines) == 3 * len(pc.all_cases(trainer_loss_cases))


# ------------------------------------------------------------------------------------------------------ network buffers

SERIAL_NETS = {"cartpole": configs.cartpole, "lunarlander": configs.lunarlander, "tictactoe": configs.tictactoe,
               "connect4-narrow": SERIAL["connect4-narrow"][0],
               # the two down-sampling stems on boards the serial build runs in seconds (breakout's 96 x 96 takes a minute)
               "breakout-16x32": lambda: configs.breakout(observation_shape=(3, 16, 32)),
               "cnn_small": lambda: configs.breakout(downsample="CNN", observation_shape=(2, 40, 56), stacked_observations=1,
                                                     channels=8, blocks=1),
               "odd": lambda: configs.tictactoe(observation_shape=(2, 4, 5), action_space=list(range(5)), stacked_observations=2,
                                                channels=6, blocks=2, reduced_channels_reward=3, reduced_channels_value=5,
                                                reduced_channels_policy=2, resnet_fc_reward_layers=[7, 9],
                                                resnet_fc_value_layers=[], resnet_fc_policy_layers=[33])}


@pytest.mark.parametrize("name", sorted(SERIAL_NETS))
def test_network_derived_and_workspace(backend, name):
    lines = pc.net_case(backend, name, SERIAL_NETS[name]())
    assert len(lines) >= len(pc.PATTERNS)


# ------------------------------------------------------------------------------------------- the sampler's workspace

@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("slots", replay_sampler_cases.SLOT_COUNTS)
def test_sampler_workspace(backend, slots, per):
    assert len(pc.sampler_case(backend, replay_sampler_cases, slots, per)) == 3 * len(replay_sampler_cases.BATCHES)


# ------------------------------------------------------------------------------- the arenas of mzx_selfplay_rounds

def _rounds_cases():
    import resident_rounds_cases as rounds
    from mzx import games
    cartpole = configs.cartpole(num_simulations=7, max_moves=5, action_space=list(range(3)), observation_shape=(2, 1, 3),
                                players=list(range(2)))
    return {"tictactoe": (games.TicTacToeNative, rounds.tictactoe_cfg(), 5, 7, rounds.TICTACTOE_CALLS, 21),
            "cartpole": (games.make_native_synthetic_game(cartpole.observation_shape, 3, 2), cartpole, 12, 11,
                         [(1.0, dict(max_rounds=7, min_games=rounds.FOREVER)), (0.5, dict(max_rounds=6, min_games=rounds.FOREVER))], 5)}


@pytest.mark.parametrize("name", ["tictactoe", "cartpole"])
def test_rounds_arena(backend, name):
    import resident_rounds_cases as rounds
    Game, cfg, trees, seed, calls, weight_seed = _rounds_cases()[name]
    lines = pc.rounds_case(backend, rounds, Game, cfg, trees, seed, calls, rounds._weights(backend, cfg, weight_seed))
    assert len(lines) == len(pc.PATTERNS)
