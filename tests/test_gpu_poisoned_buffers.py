"""
Poisoned arenas, workspaces and outputs on the device (tests/poison_cases.py has the method): every cell of the route table
of test_gpu_route_table.py -- CLASSES x MODES x CAPACITIES -- through mzx_search_run, mzx_search_run_from_roots,
mzx_search_advance + mzx_search_run_continued and mzx_selfplay_search, the arena (and the destination arena of the carry)
filled with each pattern, the outputs with a sentinel: same bits as the run that got zeros, and mzx_search_kernel_name names
the table's kernel, so that every kernel of the table has run under poison.  Then the two-stream split of the row route, the
two selection kernels of a wide action space, the networks' derived images and workspaces, the trainers' scratch.
Serial twin: test_poisoned_buffers.py.  5 trees x 6 simulations; each line printed ("poison: class | mode | capacity | entry |
kernel | pattern | same") is one line of profiles/poisoned_buffers_gpu.log.
"""
import ctypes

import pytest

import poison_cases as pc
from mzx import _lib
from test_gpu_route_table import CAPACITIES, CLASSES, EXPECTED, ROWS, cells

pytestmark = pytest.mark.gpu


def _net_of(backend):
    return lambda name: pc.make_net(backend, CLASSES, name)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_search_arena_and_outputs(name):
    backend = _lib.default_backend()
    for mode, cap in cells(name):
        pc.search_cell(backend, _net_of(backend), name, mode, cap, CLASSES, CAPACITIES, expected=EXPECTED[(name, mode, cap)])


def test_search_two_stream_split():
    """The row route as two half-shards on two streams.  The library divides no shard below 32 trees (rb_split_first), so
    the threshold "row_split_min" is lowered to 4 and the shard is the smallest one that divides: 33 trees, 16 + 17; the
    STALE arena comes from 35 trees, 32 + 3."""
    backend = _lib.default_backend()
    cfg, net = _net_of(backend)("tower-launches")
    with backend.lib.tuning(rt_search=0, row_split_min=4):
        cell = pc.SearchCell(backend, cfg, net, None, CAPACITIES["spare"], ("tower-launches split", "default", "spare"), trees=33,
                             stale_trees=35)
        route = (ctypes.c_int32 * 8)()
        backend.lib.check(backend.lib.mzx_search_route(cell.engine.handle(33), route))
        assert route[0] == 2 and (route[6], route[7]) == (16, 17), list(route)
        for entry in ("run", "selfplay_search", "continued"):
            lines = cell.check(entry)
            assert all("row_select_kernel" in line and "two half-shards" in line for line in lines)
    for line in cell.lines:
        print("poison:", line)


@pytest.mark.parametrize("wave", [0, 1])
def test_search_wave_select(wave):
    """games/gomoku.py's 121 actions on the row route: a wavefront per tree selects (wave_select_kernel, 1) or a 16-lane row
    (row_select_kernel<0>, 0)."""
    backend = _lib.default_backend()
    cfg, net = _net_of(backend)("streamed")
    with backend.lib.tuning(wave_select=wave):
        cell = pc.SearchCell(backend, cfg, net, None, CAPACITIES["spare"], (f"streamed wave_select={wave}", "default", "spare"))
        for entry in ("run", "from_roots", "continued"):
            cell.check(entry, ROWS)
    for line in cell.lines:
        print("poison:", line)


# ------------------------------------------------------------------------------------------------------ network buffers

def _networks():
    from test_gpu_parity import RESNET_CASES
    from test_gpu_streamed import STREAMED_CASES
    from mzx import configs
    nets = {"cartpole": configs.cartpole, "lunarlander": configs.lunarlander}
    nets.update({"parity-" + k: v for k, v in RESNET_CASES.items()})
    nets.update({"streamed-" + k: STREAMED_CASES[k][0] for k in ("tictactoe", "connect4", "breakout", "breakout_cnn", "cnn_small",
                                                                  "odd", "wide144")})
    return nets


NETWORKS = _networks()
# the head chains as slices of one launch per level (2) or a launch per layer (0); the tower's tail inside its launch or not
TUNINGS = tuple(dict(rb_heads=h, rb_tail=t) for h in (0, 2) for t in (0, 1))


@pytest.mark.parametrize("name", sorted(NETWORKS))
def test_network_derived_and_workspace(name):
    """d_derived poisoned before mzx_net_set_weights, d_workspace before both inferences, d_scratch and d_workspace of
    mzx_net_debug_prefix: batches 1, 5 and 37, the modes the handle accepts (default, 0, 3), "rb_heads" 0 / 2 x "rb_tail" 0 / 1
    on the MFMA engines -- logits and hidden states as under zeros, bit for bit."""
    backend = _lib.default_backend()
    for line in pc.net_case(backend, name, NETWORKS[name](), TUNINGS):
        print("poison:", line)


# ------------------------------------------------------------------------------------------ trainers and the loss head

def _train_cases():
    import fc_train_cases
    import resnet_stem_train_cases
    import resnet_train_cases
    return [(tables, kind, case) for tables, kind in ((fc_train_cases, "fc"), (resnet_train_cases, "resnet"),
                                                      (resnet_stem_train_cases, "resnet")) for case in pc.all_cases(tables)]


TRAIN_CASES = _train_cases()


@pytest.mark.parametrize("tables,kind,case", TRAIN_CASES, ids=[f"{kind}-{case['name']}" for _, kind, case in TRAIN_CASES])
def test_trainer_scratch_and_outputs(tables, kind, case):
    backend = _lib.default_backend()
    for line in pc.train_case(backend, tables, kind, case):
        print("poison:", line)


def test_loss_head_scratch_and_outputs():
    import trainer_loss_cases
    for line in pc.loss_table(_lib.default_backend(), trainer_loss_cases):
        print("poison:", line)


# ------------------------------------------------------------- the sampler's workspace, the arenas of resident rounds

def _slot_counts():
    import replay_sampler_cases
    return replay_sampler_cases.SLOT_COUNTS


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("slots", _slot_counts())
def test_sampler_workspace(slots, per):
    import replay_sampler_cases
    for line in pc.sampler_case(_lib.default_backend(), replay_sampler_cases, slots, per):
        print("poison:", line)


@pytest.mark.parametrize("name", ["tictactoe", "cartpole"])
def test_rounds_arena(name):
    import resident_rounds_cases as rounds
    from test_poisoned_buffers import _rounds_cases
    backend = _lib.default_backend()
    Game, cfg, trees, seed, calls, weight_seed = _rounds_cases()[name]
    for line in pc.rounds_case(backend, rounds, Game, cfg, trees, seed, calls, rounds._weights(backend, cfg, weight_seed)):
        print("poison:", line)
