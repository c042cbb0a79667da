"""
The tree kernels at action-width, tie-draw and depth boundaries, on the MI355X (tests/tree_edge_cases.py holds the shared
table and checks; tests/test_tree_edges.py is the CPU twin of part 1).

  1. The anchor: the per-operator tree operators through the lock-step ABI on generated tables against the CPU oracle,
     bit for bit, tape position included -- widths 1 .. 361, A-way ties with rejected tape words, depth == S.
  2. Every tuned search kernel against the per-operator path (mode 0), bit for bit -- every exported tree array, the search
     outputs, tape_used, flags == 0 -- at the widths where it changes code path (16|17, 64|65, 128|129, 256|257), with
     networks that tie at every level (`flat`), that put two equal maxima either side of a chunk border (`pair`), that walk
     through the last slot of every level as deep as the search is long (`last`), and whose min-max bounds never separate
     (`constant`).  The route that ran is asserted by name in every case, so a later change of routing fails the case
     instead of moving it silently.  (The library reports ONE name for the row route, whichever of row_select_kernel<0> and
     wave_select_kernel selected: which of the two ran rests on the tuning switch "wave_select", on which
     row_search_step<0> routes, as in tests/test_gpu_streamed.py.)
Each case prints one line: route, width, kind, kernel, deepest walk, tape words used against the simulations.
"""
import numpy
import pytest

from mzx import _lib, models, search, self_play, synthetic

import test_gpu_continue_shapes as shapes
import test_gpu_parity as parity
import test_gpu_streamed as streamed
import test_gpu_tower_search as tower
import tree_edge_cases as edges

pytestmark = pytest.mark.gpu

LONG_TAPE = 4096      # a tree that overflows its tape is searched again at another shard size: its exported tree would be gone
ROWS = "row_select_kernel"
ONE_THREAD = "one-thread-per-tree"
FC2, RT, RZ = "mzx::fc2_search_kernel", "mzx::rt_search_kernel", "mzx::rz_search_kernel"
PER_OPERATOR = "one kernel per step of a simulation"


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.fixture(autouse=True)
def _long_tape():
    old = search.TAPE_WORDS
    search.TAPE_WORDS = LONG_TAPE
    try:
        yield
    finally:
        search.TAPE_WORDS = old


# ----------------------------------------------------------------------------- 1. the anchor on the device

@pytest.mark.parametrize("name", [c["name"] for c in edges.LOCKSTEP_CASES])
def test_tree_edges_lockstep_bit_exact(backend, name):
    edges.check_lockstep(backend, edges.LOCKSTEP_BY_NAME[name], report=print)


# ----------------------------------------------------------------------------- 2. tuned kernels against mode 0

def _kinds(A, extra=()):
    """(kind, pair) of a width: random, flat, last, and a pair at each chunk border the width has."""
    return [("random", None), ("flat", None), ("last", None)] + [("pair", b) for b in edges.borders(A)] + list(extra)


def _id(v):
    if isinstance(v, tuple):
        return "-".join(str(x) for x in v)
    return str(v)


def _network(make, A, kind, S, pair=None, value_bin=None, players=None, net_mode=None, seed=12):
    cfg = make()
    cfg.action_space = list(range(A))
    cfg.num_simulations = S
    if players is not None:
        cfg.players = list(range(players))
    net = models.MuZeroNetwork(cfg)
    net.set_weights(edges.network_weights(net, kind, A, seed=seed, pair=pair, value_bin=value_bin))
    if net_mode is not None:
        net.set_mode(net_mode)
    return cfg, net


def _inputs(cfg, net, B, seed=6):
    A = len(cfg.action_space)
    obs = synthetic.observations(B, net.input_shape, seed=seed)
    legal = edges.ragged_legal(A, B, seed + 1)
    to_play = [int(i % len(cfg.players)) for i in range(B)]
    return obs, legal, to_play


def _search(backend, cfg, net, B, mode, inputs, noise, tuning):
    """One search of B trees: ((result, exported trees), kernel name)."""
    obs, legal, to_play = inputs
    with backend.lib.tuning(**tuning):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        res = engine.run(list(obs), legal, to_play, noise, [numpy.random.RandomState(500 + i) for i in range(B)])
        kernel = engine.kernel_name(B)
        out = (res, engine.export_trees(B))
    assert (res.flags == 0).all(), (kernel, res.flags)
    assert (res.tape_used < LONG_TAPE).all() and (res.visit_counts.sum(1) == cfg.num_simulations).all()
    return out, kernel


def _yardstick(backend, cfg, net, B, inputs, noise, kind, pair=None):
    """Mode 0 (SelectOp / ExpandBackpropOp, one thread per tree) and the precondition of the network kind on its result."""
    out, kernel = _search(backend, cfg, net, B, 0, inputs, noise, {})
    assert ONE_THREAD in kernel or kernel.startswith(PER_OPERATOR), kernel
    A, S = len(cfg.action_space), cfg.num_simulations
    edges.check_network_precondition(kind, A, S, out[0], inputs[1], pair=pair, trees=out[1], cfg=cfg)
    return out


def _report(route, cfg, kind, pair, kernel, res):
    S = cfg.num_simulations
    print(f"tree_edges {route}: A {len(cfg.action_space)} kind {kind}{'' if pair is None else list(pair)} players {len(cfg.players)} "
          f"kernel {kernel.split(' between ')[-1] if ' between ' in kernel else kernel} | deepest walk {int(res.max_tree_depth.max())} of {S} | "
          f"tape_used {res.tape_used.tolist()} for {S} simulations")


def _noise_of(kind):
    return kind in ("random", "constant")      # flat / last / pair: only without root noise does the root itself tie


# ---- the row route: row_select_kernel<0> and wave_select_kernel around the streamed engine

ROW_WIDTHS = (17, 64, 65, 128, 129, 255, 256)
ROW_NET = streamed.WAVE_SELECT_CASES["wide200"][0]      # a small convolutional network on a 4 x 8 board
ROW_CASES = [(A, kind, pair, 40, 2) for A in ROW_WIDTHS for kind, pair in _kinds(A)]
# walks deeper than a wavefront has lanes: lane == depth has no lane beyond 63, the path record carries them
ROW_CASES += [(A, "last", None, 70, players) for A in (128, 129) for players in (1, 2)]


@pytest.mark.parametrize("A,kind,pair,S,players", ROW_CASES, ids=_id)
def test_tree_edges_row_and_wave_selection(backend, A, kind, pair, S, players):
    """row_select_kernel<0> (row_select_wide<8> up to 128 actions, <WIDE_MAX_CHUNKS> above; tuning "wave_select" = 0) and
    wave_select_kernel (wave_select_wide<2> up to 128 actions, <4> up to 256) against one thread per tree."""
    B = 7
    cfg, net = _network(ROW_NET, A, kind, S, pair=pair, players=players, net_mode=3)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(kind)
    want = _yardstick(backend, cfg, net, B, inputs, noise, kind, pair)
    # (one name for both: the switch decides between row_select_kernel<0> and wave_select_kernel, see the module docstring)
    for label, wave in (("a row per tree", 0), ("a wavefront per tree", 1)):
        got, kernel = _search(backend, cfg, net, B, 1, inputs, noise, {"rt_search": 0, "wave_select": wave})
        assert ROWS in kernel and ONE_THREAD not in kernel, kernel
        tower._assert_same(want, got, (A, kind, pair, label))
        _report(label, cfg, kind, pair, kernel, got[0])


@pytest.mark.parametrize("A,kind,S", [(257, "random", 40), (257, "flat", 40), (361, "random", 12), (361, "flat", 12)], ids=_id)
def test_tree_edges_above_256_actions_fall_back(backend, A, kind, S):
    """More than WIDE_MAX_CHUNKS * FUSED_ROW = 256 actions (go19: 361): no row or wavefront selection kernel, and the trees
    of mode 0."""
    B = 5
    cfg, net = _network(ROW_NET, A, kind, S, net_mode=3)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(kind)
    want = _yardstick(backend, cfg, net, B, inputs, noise, kind)
    for wave in (0, 1):
        # (the handle's default mode: the planners decline the width, and asking such a handle for a tuned kernel is an error)
        got, kernel = _search(backend, cfg, net, B, None, inputs, noise, {"wave_select": wave})
        assert ROWS not in kernel and ONE_THREAD in kernel, kernel
        tower._assert_same(want, got, (A, kind, "fallback"))
    _report("fallback", cfg, kind, None, kernel, got[0])


# ---- rz_search_kernel, wide child records

RZ_NET = parity.RESNET_CASES["gomoku"]      # 16 channels x 2 blocks on 11 x 11: the LDS-resident engine takes it
RZ_CASES = [(A, kind) for A in (17, 128, 129, 256) for kind in ("random", "flat", "last")]


@pytest.mark.parametrize("A,kind", RZ_CASES, ids=_id)
def test_tree_edges_residual_whole_search_wide_records(backend, A, kind):
    B, S = 5, 40
    cfg, net = _network(RZ_NET, A, kind, S)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(kind)
    with backend.lib.tuning(wide_towers=0):
        want = _yardstick(backend, cfg, net, B, inputs, noise, kind)
    got, kernel = _search(backend, cfg, net, B, 1, inputs, noise, {"wide_towers": 0})
    assert kernel == RZ, (A, kernel)
    tower._assert_same(want, got, (A, kind, "rz_search_kernel"))
    _report("rz", cfg, kind, None, kernel, got[0])


# ---- rt_search_kernel, wide child records

RT_NET = tower.CASES["wide32"]              # 64 channels, one block, 4 x 8
RT_CASES = [(A, kind) for A in (17, 128, 129, 256) for kind in ("random", "flat", "last")]
# widths rt_search_kernel declines -- rt_structure: a head layer of more than eight 16-column tiles (a policy layer of more than
# 128 outputs: one column tile per wave) -- and a string the name of what runs instead contains: the per-simulation launches
RT_KERNEL = {129: ROWS, 256: ROWS}


@pytest.mark.parametrize("A,kind", RT_CASES, ids=_id)
def test_tree_edges_tower_whole_search_wide_records(backend, A, kind):
    """rt_search_kernel against one thread per tree, and equal to the per-simulation launches of the same engine.  Above 128
    actions the library itself takes the per-simulation launches (RT_KERNEL): asserted by name and held to one thread per
    tree; a second run of the launches would be the same run."""
    B, S = 5, 40
    cfg, net = _network(RT_NET, A, kind, S)
    _, net3 = _network(RT_NET, A, kind, S, net_mode=3)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(kind)
    want = _yardstick(backend, cfg, net3, B, inputs, noise, kind)
    got, kernel = _search(backend, cfg, net, B, 1, inputs, noise, {"rt_search": 1})
    assert (kernel == RT) if A not in RT_KERNEL else (RT_KERNEL[A] in kernel and kernel != RT), (A, kernel)
    tower._assert_same(want, got, (A, kind, "rt_search_kernel"))
    if A not in RT_KERNEL:
        launches, k2 = _search(backend, cfg, net, B, 1, inputs, noise, {"rt_search": 0})
        assert ROWS in k2 and "rb_tower_kernel" in k2, k2
        tower._assert_same(got, launches, (A, kind, "rt vs launches"))
    _report("rt", cfg, kind, None, kernel, got[0])


# ---- fc2_search_kernel on LdsNet: child records of 2 / 4 / 16 lanes

def _fc_kinds():
    out = []
    for A in (1, 3, 4, 5, 15, 16):
        for players in (1, 2):
            out += [(A, "flat", players), (A, "last", players), (A, "constant+5", players), (A, "constant-5", players)]
    return out


def _fc_network(A, kind, S, players):
    make = lambda: shapes._lds16(A)(players=list(range(players)))
    if kind.startswith("constant"):
        c = int(kind[len("constant"):])
        # discount 1 and rewards of zero: a backed-up value is the leaf's value itself, and a sum of n <= S + 1 equal fp32
        # values divided by n is that value again in binary64 -- the bounds of a one-player search never separate
        make = lambda: shapes._lds16(A)(players=list(range(players)), discount=1)
        return _network(make, A, "constant", S, value_bin=make().support_size + c), "constant"
    return _network(make, A, kind, S), kind


@pytest.mark.parametrize("A,kind,players", _fc_kinds(), ids=_id)
def test_tree_edges_fc2_whole_search(backend, A, kind, players):
    """fc2_search_kernel<LdsNet, AW = 2 / 4 / 16> at the record widths' ends: ties among every child at every level,
    the last slot all the way down, and `constant`: every value the same c (the decode of bin +5 / -5, about +-34.6), rewards
    zero, discount 1.  With one player max <= min holds for the whole search with q != 0: every score takes the
    unnormalised-q branch, and c > 0 digs one line while c < 0 spreads.  With two players the sign alternates, so the bounds
    are -|c| and |c| from the second simulation on: normalised q of exactly 0 or 1 at every node, ties at every level."""
    B, S = 7, 40
    (cfg, net), base = _fc_network(A, kind, S, players)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(base)
    want = _yardstick(backend, cfg, net, B, inputs, noise, base)
    got, kernel = _search(backend, cfg, net, B, 3, inputs, noise, {})      # (3: whole-search kernel + trees exported to the arena)
    assert kernel == FC2, (A, kernel)
    tower._assert_same(want, got, (A, kind, players, "fc2"))
    _report("fc2", cfg, kind, None, kernel, got[0])


@pytest.mark.parametrize("kind", ["flat", "last", "random"])
def test_tree_edges_seventeen_actions_do_not_run_fc2(backend, kind):
    """One action more than a 16-lane record: not fc2_search_kernel, and the trees of mode 0."""
    B, S, A = 7, 40, 17
    (cfg, net), _ = _fc_network(A, kind, S, 2)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(kind)
    want = _yardstick(backend, cfg, net, B, inputs, noise, kind)
    got, kernel = _search(backend, cfg, net, B, None, inputs, noise, {})      # (the default mode: what the library picks itself)
    assert kernel.startswith(PER_OPERATOR), kernel
    tower._assert_same(want, got, (A, kind, "seventeen actions"))
    _report("fc, 17 actions", cfg, kind, None, kernel, got[0])


# ---- rz_wave_search_kernel / rz_tile_search_kernel: 4-lane and 16-lane records

SMALL_CASES = [(case, A, kind) for case in ("wave-4x4", "tile-3x6") for A in (4, 5, 16) for kind in ("flat", "last")]


@pytest.mark.parametrize("case,A,kind", SMALL_CASES, ids=_id)
def test_tree_edges_small_board_kernels(backend, case, A, kind):
    make, want_kernel = parity.SMALL_BOARD_CASES[case]
    B, S = 7, 40
    cfg, net = _network(make, A, kind, S)
    inputs = _inputs(cfg, net, B)
    noise = _noise_of(kind)
    want = _yardstick(backend, cfg, net, B, inputs, noise, kind)
    got, kernel = _search(backend, cfg, net, B, 3, inputs, noise, {})
    assert kernel == want_kernel, (case, A, kernel)
    tower._assert_same(want, got, (case, A, kind))
    _report(case, cfg, kind, None, kernel, got[0])
