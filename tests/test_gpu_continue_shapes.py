"""
Continued searches at the kernels and root shapes the fresh searches are tested at (tests/test_gpu_tower_search.py,
tests/test_gpu_streamed.py, tests/test_gpu_parity.py), on the MI355X.  Every tuned route is tied, bit for bit and round by
round, to the per-operator path, which tests/test_gpu_search_continue.py ties to the oracle helper
(tests/continue_oracle.py) at the same root shapes:
  * fc2_search_kernel<LdsNet, AW = 2 / 4 / 16, CONT> and <SmallNetCartpole, CONT> against the per-operator path (mode 0):
    restricted and single-action roots, the old root again on them, two players, forced ties at restricted roots;
  * rt_search_kernel, the launch-by-launch tower route and the one-thread-per-tree operators around the streamed engine
    on the 4-lane records, one player, several slots per lane, forced tilings, ragged last workgroups, 121 actions;
  * wave_select_kernel against row_select_kernel from carried roots, walks deeper than sixteen plies from a carried root,
    the two half-shards on two streams, searches without exploration noise on aligned and ragged shards;
  * TF_BAD_CARRY (flag 4) through BatchedMCTS past the host guard: raised, kept in the arena next to the old root, and
    the same on the whole-search kernels as on the per-operator path.
The picks come from each tree's current root actions and mix the old root, the most visited and the least visited expanded
child; the route and the flags are asserted after every round.
"""
import ctypes

import numpy
import pytest
import torch

from mzx import _lib, configs, models, self_play, synthetic

import test_gpu_continue_whole_search as whole
import test_gpu_streamed as streamed
import test_gpu_tower_search as tower
from test_search_continue import ragged_legal

pytestmark = pytest.mark.gpu

FC2, RT, PER_OPERATOR = whole.FC2, whole.RT, whole.PER_OPERATOR
ONE_THREAD = "one-thread-per-tree"


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def _pick(res, i, r):
    """Chosen action of tree i in round r, from its CURRENT root actions: the old root again, the most visited child, or
    the least visited expanded one."""
    v = res.visit_counts[i]
    acts = res.legal_actions[i]
    k = (i + r) % 3
    if k == 0:
        return -1
    seen = [a for a in acts if v[a] > 0]
    if k == 2:
        return int(min(seen, key=lambda a: (v[a], a)))
    return int(max(seen, key=lambda a: (v[a], -a)))


def _is(kernel, route0):
    def check(k, rt):
        assert rt[0] == route0 and (k == kernel if kernel.startswith("mzx::") else kernel in k), (k, rt)
    return check


def _chain(engine, cfg, net, B, rounds, seed, legal, to_play, check, noise=True, obs=None):
    """A fresh search and `rounds` continuations; per round (result, trees, kernel name, route, stream states)."""
    obs = synthetic.observations(B, net.input_shape, seed=seed) if obs is None else obs
    rngs = [numpy.random.RandomState(seed + i) for i in range(B)]
    P = len(cfg.players)
    tp = numpy.array(to_play, numpy.int64)
    out = []

    def note(res):
        kernel, route = engine.kernel_name(B), whole._route(engine, B)
        check(kernel, route)
        assert (res.flags == 0).all(), res.flags
        states = [(r.get_state()[1].copy(), r.get_state()[2]) for r in rngs]
        out.append((res, engine.export_trees(B), kernel, route, states))

    res = engine.run(list(obs), [list(a) for a in legal], list(tp), noise, rngs)
    note(res)
    for r in range(rounds):
        acts = [_pick(res, i, r) for i in range(B)]
        tp = numpy.array([(tp[i] + 1) % P if a >= 0 else tp[i] for i, a in enumerate(acts)])
        res = engine.continue_search(acts, list(tp), noise, rngs)
        note(res)
        assert any(a < 0 for a in acts) and any(a >= 0 for a in acts)
    torch.cuda.synchronize()
    return out


def _assert_same(a, b, label):
    for r, (x, y) in enumerate(zip(a, b)):
        whole._assert_same(x[:4], y[:4], (label, "round", r))
        for i, ((ka, pa), (kb, pb)) in enumerate(zip(x[4], y[4])):
            assert pa == pb and numpy.array_equal(ka, kb), (label, "round", r, "stream of tree", i)
    assert len(a) == len(b)


# ---------------------------------------------------------------- fully connected networks: fc2_search_kernel<.., CONT>

def _lds16(A):
    """test_fused_lds_engine_other_shapes' network (tests/test_gpu_parity.py): E = 10, stacked observations, A actions."""
    return lambda **kw: configs.cartpole(action_space=list(range(A)), stacked_observations=2, encoding_size=10,
                                         fc_representation_layers=[12], fc_dynamics_layers=[24, 12], fc_reward_layers=[20],
                                         fc_value_layers=[], fc_policy_layers=[33], **kw)


#        case: config factory, fc2 mode, B, S, rounds, carried capacity in S, ragged legal sets, uniform policy head
FC_CASES = {
    "lds16_a6": (_lds16(6), None, 37, 10, 2, 3, False, False),
    "lds16_a16": (_lds16(16), None, 37, 10, 2, 3, False, False),
    "lds2_forced": (configs.cartpole, 7, 37, 12, 3, 4, False, False),
    "lds2_stacked": (lambda **kw: configs.cartpole(stacked_observations=2, **kw), None, 37, 12, 3, 4, False, False),
    "two_players": (lambda **kw: configs.cartpole(players=[0, 1], **kw), None, 64, 12, 3, 4, False, False),
    "two_players_forced": (lambda **kw: configs.cartpole(players=[0, 1], **kw), 7, 64, 12, 3, 4, False, False),
    "ragged_roots_cartpole": (configs.cartpole, None, 64, 12, 3, 4, True, False),
    "ragged_roots_lunarlander": (configs.lunarlander, None, 64, 12, 3, 4, True, False),
    "ragged_roots_lds16_a6": (_lds16(6), None, 64, 12, 3, 4, True, False),
    # (S = 5: this network ties below the first level too -- a walk can draw at every level, a search has sixteen tape words;
    #  twelve simulations use up to nineteen, five at most twelve in any round)
    "ties": (_lds16(6), None, 48, 5, 3, 4, True, True),
}


@pytest.mark.parametrize("case", sorted(FC_CASES))
def test_fc2_continuations_equal_per_operator_path(backend, case):
    """fc2_search_kernel's continued instantiations against the per-operator path: LdsNet with AW = 16 (5 <= A <= 16),
    AW = 4 (lunarlander) and AW = 2 (cartpole with the register network switched off, mode flag 4, and a two-action network
    of another shape), SmallNetCartpole; carried two-player nodes with tree i starting as player i % 2; ragged legal sets
    with a single-action root that is searched again (the `roota` import, the visit counts scattered through it, the
    prior scores cached at `rootn` slots); forced ties at restricted roots (tape draws in slot order)."""
    make, fc2_mode, B, S, rounds, cap, ragged, ties = FC_CASES[case]
    cfg = make(num_simulations=S)
    A, P = len(cfg.action_space), len(cfg.players)
    net = whole._net(cfg, 11, uniform_policy=ties)
    legal = ragged_legal(A, B, 23) if ragged else [list(cfg.action_space)] * B
    to_play = [i % P for i in range(B)]
    outs = {}
    for mode, check in ((fc2_mode, _is(FC2, 4)), (0, _is(PER_OPERATOR, 0))):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=cap * S)
        outs[mode] = _chain(engine, cfg, net, B, rounds, 31, legal, to_play, check)
    _assert_same(outs[fc2_mode], outs[0], case)
    n = outs[0][-1][1]["n_nodes"]
    assert n.min() < n.max() and n.max() > S + 1
    if ragged:
        first = outs[0][1][0]       # round 0: tree 0 has a single legal action and is searched again
        assert first.legal_actions[0] == legal[0] and len(legal[0]) == 1 and first.visit_counts[0].sum() == 2 * S
        assert len({len(a) for a in legal}) > 1
    if P == 2:
        assert all(len(set(t["to_play"][:, 0])) == 2 for _, t, _, _, _ in outs[0])
    if ties:
        assert any((res.tape_used > 0).any() for res, _, _, _, _ in outs[0][1:])


# ---------------------------------------------------------------- residual networks: rt_search_kernel and the row kernels

def _residual(make, S, flat=False, seed=12):
    """The config, a network on its default engines and one with the same weights on the streamed engine for everything
    (the partner of the one-thread-per-tree operators, as in tests/test_gpu_streamed.py)."""
    cfg = make()
    cfg.num_simulations = S
    nets = []
    for streamed_only in (False, True):
        net = models.MuZeroNetwork(cfg)
        sd = synthetic.fill_state_dict(net.state_dict(), seed)
        if flat:
            last = [k for k in sd if "fc_policy" in k and k.endswith(".weight")][-1]
            sd[last] = sd[last] * 0
        net.set_weights(sd)
        if streamed_only:
            net.set_mode(3)
        nets.append(net)
    return cfg, nets[0], nets[1]


def _run_engines(backend, cfg, B, S, rounds, engines, noise=True, seed=6):
    """engines: (label, network, engine mode, tuning entries, check, second run on the same engine).  Every chain must
    equal the first one, bit for bit, in every round."""
    first = None
    outs = {}
    for label, net, mode, tuning, check, again in engines:
        obs, legal, to_play = tower._inputs(cfg, net, B, seed)
        with backend.lib.tuning(**tuning):
            engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=(rounds + 1) * S)
            for run in range(2 if again else 1):
                out = _chain(engine, cfg, net, B, rounds, 500, legal, to_play, check, noise=noise, obs=obs)
                name = label if run == 0 else label + ", second run"
                outs[name] = out
                if first is None:
                    first = (name, out)
                else:
                    _assert_same(first[1], out, (first[0], "vs", name))
    assert len({len(a) for a in legal}) > 1
    return outs


RT_CASES = [
    ("narrow4", 23, 20, {}), ("narrow4", 23, 20, {"rt_trees": 7, "rt_waves": 4}),
    ("board4x4", 37, 20, {}), ("board4x4", 37, 20, {"rt_trees": 12, "rt_waves": 8}),
    ("wide32", 21, 24, {}), ("wide32", 21, 24, {"rt_trees": 3, "rt_waves": 4}),
    ("connect4", 51, 24, {"rt_trees": 2}), ("connect4", 51, 24, {"rt_trees": 6}),
]


@pytest.mark.parametrize("name,B,S,tuning", RT_CASES, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "default"
                         if isinstance(v, dict) else str(v))
def test_rt_continuations_equal_launches_and_one_thread_per_tree(backend, name, B, S, tuning):
    """rt_search_kernel (twice on the same engine), the launch-by-launch tower route (tuning "rt_search" = 0) and the
    one-thread-per-tree operators around the streamed engine continue the same trees, bit for bit, in every round: 4-lane
    child records, one-player back-propagation, several child slots per lane, forced trees per workgroup and workgroup
    sizes, a ragged last workgroup, ragged legal sets, tree i starting as player i % P."""
    cfg, net, net3 = _residual(tower.CASES[name], S)

    def rt(kernel, route):
        assert kernel == RT and route[0] == 3, (kernel, route)
        if "rt_trees" in tuning:
            assert route[1] == tuning["rt_trees"], route
        if "rt_waves" in tuning:
            assert route[6] == 64 * tuning["rt_waves"], route

    def launches(kernel, route):
        assert "row_select_kernel" in kernel and "rb_tower_kernel" in kernel and route[0] == 2, (kernel, route)

    _run_engines(backend, cfg, B, S, 2, [("rt_search_kernel", net, None, tuning, rt, True),
                                         ("launches", net, None, {"rt_search": 0}, launches, False),
                                         (ONE_THREAD, net3, 0, {}, _is(ONE_THREAD, 0), False)])


def test_gomoku_continuations_select_by_wavefront(backend):
    """games/gomoku.py as shipped (121 actions): the streamed row route continues with wave_select_kernel, against
    row_select_kernel (tuning "wave_select" = 0) and the one-thread-per-tree operators."""
    cfg, net, net3 = _residual(tower.CASES["gomoku"], 12)
    rows = _is("row_select_kernel", 2)
    _run_engines(backend, cfg, 6, 12, 2, [("a wavefront per tree", net, None, {}, rows, True),
                                          ("a row per tree", net, None, {"wave_select": 0}, rows, False),
                                          (ONE_THREAD, net3, 0, {}, _is(ONE_THREAD, 0), False)])


@pytest.mark.parametrize("name,B,S", [("wide200", 11, 20), ("wide32_deep", 10, 60)])
def test_row_route_continuations_wave_and_row_selection(backend, name, B, S):
    """The row route (tuning "rt_search" = 0) from carried roots with a wavefront per tree and with a row per tree (tuning
    "wave_select" 1 and 0) against the one-thread-per-tree operators: four 64-slot chunks per lane (wide200), and, with a
    flat policy head, continued rounds whose walks pass sixteen plies from a carried root (wide32_deep: the path record
    and the chunked back-propagation start in a carried tree)."""
    make, _, _, flat = streamed.WAVE_SELECT_CASES[name]
    cfg, _, net3 = _residual(make, S, flat=flat)
    rows = _is("row_select_kernel", 2)
    outs = _run_engines(backend, cfg, B, S, 2, [
        ("a wavefront per tree", net3, 1, {"rt_search": 0, "wave_select": 1}, rows, True),
        ("a row per tree", net3, 1, {"rt_search": 0, "wave_select": 0}, rows, False),
        (ONE_THREAD, net3, 0, {}, _is(ONE_THREAD, 0), False)])
    if flat:
        depths = [res.max_tree_depth.max() for res, _, _, _, _ in outs[ONE_THREAD][1:]]
        print(f"{name}: deepest walk of the continued rounds {depths}")
        assert max(depths) >= 17, depths


def test_two_half_shards_continue_the_same_trees(backend):
    """connect4, 130 trees: the launch-by-launch route undivided (tuning "row_split_min" = 0) and as two half-shards on two
    streams (32), both halves with the roots' visit counts read from the trees, and rt_search_kernel."""
    B, S = 130, 20
    cfg, net, _ = _residual(tower.CASES["connect4"], S)

    def undivided(kernel, route):
        assert "row_select_kernel" in kernel and "two half-shards" not in kernel and route[0] == 2, (kernel, route)

    def split(kernel, route):
        assert "row_select_kernel" in kernel and "two half-shards" in kernel and route[0] == 2 and route[7] > 0, (kernel, route)

    _run_engines(backend, cfg, B, S, 2, [("undivided", net, None, {"rt_search": 0, "row_split_min": 0}, undivided, False),
                                         ("two half-shards", net, None, {"rt_search": 0, "row_split_min": 32}, split, True),
                                         ("rt_search_kernel", net, None, {}, _is(RT, 3), False)])


@pytest.mark.parametrize("B", [32, 21])
def test_continuations_without_noise(backend, B):
    """mzx_search_run_continued with io.d_noise = NULL (add_exploration_noise = False) on a shard that is a multiple of
    sixteen trees and on one that is not: the carried priors stay as they are, on every route."""
    S = 16
    cfg, net, net3 = _residual(tower.CASES["connect4"], S)
    launches = _is("row_select_kernel", 2)
    outs = _run_engines(backend, cfg, B, S, 2, [("rt_search_kernel", net, None, {}, _is(RT, 3), True),
                                                ("launches", net, None, {"rt_search": 0}, launches, False),
                                                (ONE_THREAD, net3, 0, {}, _is(ONE_THREAD, 0), False)], noise=False)
    # no noise: a root that is searched again keeps its priors bit for bit
    before, after = outs[ONE_THREAD][0], outs[ONE_THREAD][1]
    again = [i for i in range(B) if _pick(before[0], i, 0) < 0]
    assert again
    for i in again:
        assert numpy.array_equal(whole._bits(before[1]["prior"][i, 0]), whole._bits(after[1]["prior"][i, 0])), i


# ---------------------------------------------------------------- TF_BAD_CARRY past the host guard

def _finish(engine, B):
    """mzx_search_finish on the engine's arena: visit counts by action and the four info words as the trees hold them."""
    be, lib = engine.backend, engine.backend.lib
    out = dict(visits=be.zeros((B, engine.A), torch.int32), root_value=be.zeros((B,), torch.float64),
               info=be.zeros((B, 4), torch.int32))
    io = _lib.SearchIO(None, None, None, None, None, be.ptr(out["visits"]), be.ptr(out["root_value"]), None, be.ptr(out["info"]))
    lib.check(lib.mzx_search_finish(engine.handle(B), ctypes.byref(io), be.ptr(engine.arena(B)), be.stream()))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bad_carry(engine, cfg, net, B, S, legal, to_play):
    """A fresh search, then mzx_search_advance and _run_continued as continue_search calls them, with actions the host guard
    of continue_search refuses: kind 0 = a legal action whose child was never expanded, 1 = an action outside the root's
    legal set, 2 = an expanded child."""
    A, P = engine.A, len(cfg.players)
    obs = synthetic.observations(B, net.input_shape, seed=3)
    rngs = [numpy.random.RandomState(90 + i) for i in range(B)]
    res = engine.run(list(obs), legal, to_play, True, rngs)
    fresh = engine.export_trees(B)
    picks = []
    for i, acts in enumerate(legal):
        v = res.visit_counts[i]
        options = ([a for a in acts if v[a] == 0], [a for a in range(A) if a not in acts], [a for a in acts if v[a] > 0])
        kind = next(k for k in ((i + d) % 3 for d in range(3)) if options[k])
        picks.append((options[kind][-1], kind))
    acts = numpy.array([a for a, _ in picks], numpy.int32)
    root_actions = [list(range(A)) if kind == 2 else legal[i] for i, (_, kind) in enumerate(picks)]
    tp = [(to_play[i] + 1) % P if kind == 2 else to_play[i] for i, (_, kind) in enumerate(picks)]
    noise, tape, states = engine._root_draws([len(r) for r in root_actions], True, rngs)
    be, lib = engine.backend, engine.backend.lib
    engine._arena_alt = be.zeros((engine._arena.numel(),), torch.uint8)
    t_act = torch.as_tensor(acts).to(be.device)
    engine._carry = None
    lib.check(lib.mzx_search_advance(engine.handle(B), be.ptr(t_act), be.ptr(engine._arena), be.ptr(engine._arena_alt), be.stream()))
    engine._arena, engine._arena_alt = engine._arena_alt, engine._arena
    with pytest.raises(_lib.MzxError, match=r"flags \{[^}]*4[^}]*\}.*4 = not an expanded child"):
        engine._run_continued(B, root_actions, tp, noise, tape, states, rngs)
    kernel = engine.kernel_name(B)
    torch.cuda.synchronize()
    return picks, fresh, engine.export_trees(B), _finish(engine, B), kernel, [r.get_state()[2] for r in rngs]


@pytest.mark.parametrize("game", ["cartpole", "narrow4"])
def test_bad_carry_is_flagged_and_keeps_the_old_root(backend, game):
    """An action that names no expanded child, put past continue_search's host guard: _run_continued raises MzxError naming
    flag 4; the arena's trees still carry the flag (info word 1 is 4 exactly on those trees) and the old root -- its
    legal actions, every node of the fresh tree and S more; the whole-search kernel (fc2_search_kernel imports and
    exports the flag, rt_search_kernel leaves it where it is) and the per-operator path agree on trees and info words."""
    if game == "cartpole":
        S, B = 6, 37
        cfg = configs.cartpole(num_simulations=S)
        nets = [whole._net(cfg, 11)] * 2
        engines = [(None, FC2), (0, PER_OPERATOR)]
    else:
        S, B = 3, 23
        cfg, net, net3 = _residual(tower.CASES["narrow4"], S)
        nets = [net, net3]
        engines = [(None, RT), (0, ONE_THREAD)]
    A, P = len(cfg.action_space), len(cfg.players)
    legal = ragged_legal(A, B, 41)
    to_play = [i % P for i in range(B)]
    got = []
    for net, (mode, kernel) in zip(nets, engines):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=2 * S + 1)
        got.append(_bad_carry(engine, cfg, net, B, S, legal, to_play))
        assert kernel in got[-1][4], got[-1][4]
    picks, fresh, trees, fin, _, _ = got[0]
    kinds = {k for _, k in picks}
    assert {1, 2} <= kinds and (game == "cartpole" or 0 in kinds), kinds
    want = numpy.array([0 if k == 2 else 4 for _, k in picks])
    assert numpy.array_equal(fin["info"][:, 1], want), fin["info"][:, 1]
    for i, (a, kind) in enumerate(picks):
        if kind == 2:
            continue
        n = S + 1
        assert trees["n_nodes"][i] == 2 * S + 1 and trees["visit"][i, 0] == 2 * S
        assert numpy.array_equal(trees["parent"][i, :n], fresh["parent"][i, :n])
        assert numpy.array_equal(whole._bits(trees["reward"][i, :n]), whole._bits(fresh["reward"][i, :n]))
        assert numpy.array_equal(trees["to_play"][i, :n], fresh["to_play"][i, :n])
        assert (fin["visits"][i][[x for x in range(A) if x not in legal[i]]] == 0).all() and fin["visits"][i].sum() == 2 * S
    for other in got[1:]:
        assert [p for p in other[0]] == picks
        for k in whole.TREE_KEYS:
            assert numpy.array_equal(whole._bits(trees[k]), whole._bits(other[2][k])), k
        for k in fin:
            assert numpy.array_equal(whole._bits(fin[k]), whole._bits(other[3][k])), k
        assert got[0][5] == other[5]
