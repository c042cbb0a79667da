"""
The streamed MFMA engine for fully connected networks (mzx_net_set_fc_engine, csrc/mzx_fc_streamed.hip) on the device: both
inferences against the oracle network evaluated in binary64 at the smallest shapes that reach every path of the kernels and
both sides of every border (the split-K threshold, the accepted host limits, the tile rule, the degenerate min/max scales),
with the per-operator path of the same handle as a second yardstick; the indexed call in the forms the searches use;
searches on the row route and on the one-thread-per-tree kernels around it against the per-operator path of the same handle,
and the switch left off.
"""
import numpy
import pytest
import torch

import fc_train_cases
import test_gpu_parity as parity
from test_gpu_streamed_at_size import _traces
from mzx import _lib, configs, models, self_play
from oracle import net_oracle, parallel

pytestmark = pytest.mark.gpu

TOL = 1e-4      # the project's gate on every logit and on the hidden state
# The relative gate: the engine's error against binary64 may be at most MARGIN x the larger of the per-operator path's error
# on the same inputs and one binary32 ulp of the output's largest expected magnitude.  Both paths round the same sums in
# binary32, in another order, so the ratio is of order 1.  MARGIN was not fixed in advance: one run on an MI355X over every
# row of SHAPES, the two degenerate ranges and every output (profiles/fc_streamed_edges.log, 140 ratios) gave 2.130 as the
# largest (wide-input, recurrent policy: 6.8e-08 against 3.2e-08), and MARGIN is twice the largest observed ratio, never
# below 2.  The largest error of the engine itself in that run is 7.0e-07.
MARGIN = 4.26


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def wide(width, **kw):
    layers = dict(fc_representation_layers=width, fc_dynamics_layers=width, fc_reward_layers=width, fc_value_layers=width,
                  fc_policy_layers=width)
    return dict(layers, **kw)


W63 = wide([63], encoding_size=63, action_space=list(range(5)))

# name: (config overrides, batch, forced rows per workgroup or 0) -- what each row is the smallest shape for
SHAPES = {
    # every layer below 64 columns: the split-K route alone; one partial row tile; a 128-bit weight row only where 4 | K
    "w16-splitk": (wide([16], action_space=list(range(3))), 17, 0),
    # 72 = 4 * 16 + 8: five column tiles over four waves (a second, ragged pass), ragged K for the next layer, E = 24, A = 18
    "w72-ragged": (wide([72], encoding_size=24, action_space=list(range(18))), 65, 0),
    # 520 columns: 33 tiles, three passes of a wave.  17 rows are far from 256 workgroups, so the rule takes the smallest tile,
    # 16 rows (as for every unforced case here); 32 forced: the multi-pass column split with two row tiles per wave (64 rows
    # of this width do not fit LDS)
    "w520": (wide([520]), 17, 0),
    "w520-tm32": (wide([520]), 17, 32),
    # F = 601 = 37 * 16 + 9 output columns on the column-split route, straight to the output tensor; a batch of one
    "support300": (wide([16], support_size=300), 1, 0),
    # MLPs that are one Linear (games/lunarlander.py's heads) / two hidden layers through both ping-pong buffers
    "no-hidden": (wide([]), 17, 0),
    "two-hidden": (wide([72, 16], encoding_size=24), 17, 0),
    # an observation wider than any LDS row, 101 values: no 128-bit loads, ragged last group
    "wide-input": (wide([16], observation_shape=(1, 1, 101)), 17, 0),
    # the other two instantiations forced: 65 rows = three workgroups of 32 / two of 64, the last one row deep
    "w16-tm32": (wide([16], action_space=list(range(3))), 65, 32),
    "w72-tm64": (wide([72], encoding_size=24, action_space=list(range(18))), 65, 64),
    # the last width on the split-K route: four column tiles in the partial buffer (KT = 4), the last one 15 columns, every k
    # range ragged (63, and 63 + 5 actions), a zero-fed 64th column under every layer
    "w63": (W63, 17, 0),
    # the first width on the column-split route: exactly one column tile per wave (live = 1 of NB), no ragged tile or k-group
    "w64": (wide([64], encoding_size=64), 17, 0),
    # the largest partial buffer: four row tiles x four column tiles per wave, the second workgroup one row deep
    "w63-tm64": (W63, 65, 64),
    # the widest layer mzx_net_set_fc_engine accepts, at the only tile size whose LDS plan fits it (16 rows): 64 column tiles,
    # four full passes of a wave; 64 k-groups of 1024 on the split-K heads
    "w1024": (wide([1024]), 17, 0),
    # the largest observation it accepts: 256 k-groups read from global memory, 64 per wave of the split-K route
    "in4096": (wide([16], observation_shape=(1, 1, 4096)), 3, 0),
    # observation reads (XG) on the column-split route: 101 inputs = six k-groups and a ragged seventh, no 128-bit loads, four
    # row tiles per wave, the second workgroup one row deep
    "in101-nsplit-tm64": (wide([72], encoding_size=24, observation_shape=(1, 1, 101)), 65, 64),
    # its vectorised twin: 100 inputs = 128-bit observation and weight loads up to a last group of one quad, two row tiles
    "in100-tm32": (wide([72], encoding_size=24, observation_shape=(1, 1, 100)), 65, 32),
    # one state value: lo == hi in every row, the `scale += 1e-5` branch of fcs_scale with 15 idle lanes per row, K = 1 layers
    "enc1": (wide([16], encoding_size=1), 17, 0),
}
KEYS = ("value", "reward", "policy", "hidden")


def network(overrides, seed, engine="streamed"):
    cfg = configs.cartpole(**overrides)
    torch.manual_seed(seed)
    net = models.MuZeroNetwork(cfg)
    net.fc_engine = engine
    return cfg, net, net.get_weights()


def _inferences(net, obs, act, hidden=None):
    """Both inferences as host tensors; the recurrent one on ``hidden`` (default: the initial inference's own state)."""
    init = [t.cpu() for t in net.initial_inference(obs)]
    rec = [t.cpu() for t in net.recurrent_inference(init[3] if hidden is None else hidden, act)]
    return init, rec


def _gate(name, net, oracle, obs, act, tm=0):
    """Both inferences of ``net`` on the streamed engine against ``oracle`` (binary64): the 1e-4 gate and the relative gate
    against the per-operator path of the same handle on the same inputs; a second call repeats every bit.  -> (initial,
    recurrent) outputs."""
    lib = net.backend.lib
    assert net.fc_engine == "streamed"
    with lib.tuning(fcs_tm=tm):
        init, rec = _inferences(net, obs, act)
        again = _inferences(net, obs, act)
    for a, b in zip(init + rec, again[0] + again[1]):      # no atomics, no dependence on what LDS held: every bit repeats
        assert torch.equal(a, b), name
    net.fc_engine = "ops"
    try:
        ops = dict(zip(("initial", "recurrent"), _inferences(net, obs, act, init[3])))
    finally:
        net.fc_engine = "streamed"
    want_init = oracle.initial_inference(obs.double())
    want_rec = oracle.recurrent_inference(init[3].double(), act.view(-1, 1))
    assert torch.equal(init[1].double(), want_init[1].double())          # the -inf / 0 reward row exactly
    failed = []
    for tag, got, want in (("initial", init, want_init), ("recurrent", rec, want_rec)):
        for key, a, o, b in zip(KEYS, got, ops[tag], want):
            if (tag, key) == ("initial", "reward"):
                continue
            assert a.shape == b.shape == o.shape, (name, tag, key)
            err = (a.double() - b.double()).abs().max().item()
            err_ops = (o.double() - b.double()).abs().max().item()
            floor = float(numpy.spacing(numpy.float32(b.abs().max().item())))
            ratio = err / max(err_ops, floor)
            print(f"edges: {name} | {tag} {key} | streamed {err:.3e} | per-operator {err_ops:.3e} | ulp {floor:.3e} | ratio {ratio:.3f}")
            if not (err < TOL and ratio <= MARGIN):
                failed.append((name, tag, key, err, err_ops, ratio))
    assert not failed, failed
    return init, rec


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_inferences_against_binary64(backend, name):
    overrides, B, tm = SHAPES[name]
    cfg, net, sd = network(overrides, 5)
    oracle = net_oracle.make_oracle_network(cfg, sd, dtype=torch.float64)
    g = torch.Generator().manual_seed(3)
    obs = torch.rand((B, net.input_size), generator=g)
    act = torch.randint(0, len(cfg.action_space), (B,), generator=g)
    init, rec = _gate(name, net, oracle, obs, act, tm)
    if net.hidden_size == 1:      # (s - lo) / (0 + 1e-5) with s == lo
        assert (init[3] == 0.0).all() and (rec[3] == 0.0).all(), name
    if tm:      # a row's bits depend neither on the tile size nor on the workgroup it falls into
        for a, b in zip(init + rec, list(net.initial_inference(obs)) + list(net.recurrent_inference(init[3], act))):
            assert torch.equal(a, b.cpu()), name


def test_degenerate_state_ranges(backend):
    """The `scale += 1e-5` branch of fcs_scale with a range strictly between 0 and 1e-5 (fc_train_cases.tiny_range: the last
    representation and dynamics layers get weight x 1e-7 and bias 0) and with a range of exactly 0 (those layers get weight 0
    and one constant bias) on a wide([16], encoding_size=6) network, 17 rows.  Tiny range: the gates of _gate.  The binary32
    oracle (net_oracle in float32), evaluated here on the same inputs, stays within 1e-4 of binary64 (measured 5.3e-8 at
    most), so the gate is one a correct binary32 kernel meets and the inputs are torch.rand's, not shrunk.  Zero range: every
    hidden state is exactly 0.0, the logits within the gate."""
    B = 17
    cfg, net, sd = network(wide([16], encoding_size=6), 5)
    g = torch.Generator().manual_seed(3)
    obs = torch.rand((B, net.input_size), generator=g)
    act = torch.randint(0, len(cfg.action_space), (B,), generator=g)
    last = [f"{mlp}.module.2.{leaf}" for mlp in ("representation_network", "dynamics_encoded_state_network") for leaf in ("weight", "bias")]
    tiny = fc_train_cases.tiny_range({k: v.clone() for k, v in sd.items()}, 1, 1)
    zero = {k: v.clone() for k, v in sd.items()}
    for k in last:
        zero[k] = torch.zeros_like(zero[k]) if k.endswith("weight") else torch.full_like(zero[k], 0.375)
    for name, weights in (("tiny-range", tiny), ("zero-range", zero)):
        net.set_weights(weights)
        o64 = net_oracle.make_oracle_network(cfg, weights, dtype=torch.float64)
        o32 = net_oracle.make_oracle_network(cfg, weights, dtype=torch.float32)
        init, rec = _gate(name, net, o64, obs, act)
        # the raw states the two scales see, in binary64: the branch is the one this case is for
        onehot = torch.nn.functional.one_hot(act, len(cfg.action_space)).double()
        for raw in (net_oracle._mlp(o64.sd, "representation_network.module.", obs.double()),
                    net_oracle._mlp(o64.sd, "dynamics_encoded_state_network.module.", torch.cat((init[3].double(), onehot), 1))):
            span = raw.max(1)[0] - raw.min(1)[0]
            assert ((span > 0) & (span < 1e-5)).all() if name == "tiny-range" else (span == 0).all(), (name, span)
        if name == "zero-range":
            assert (init[3] == 0.0).all() and (rec[3] == 0.0).all()
            continue
        pairs = list(zip(o32.initial_inference(obs), o64.initial_inference(obs.double())))[2:]
        pairs += list(zip(o32.recurrent_inference(init[3], act.view(-1, 1)), o64.recurrent_inference(init[3].double(), act.view(-1, 1))))
        worst = max((a.double() - b).abs().max().item() for a, b in pairs)
        print(f"{name}: binary32 oracle against binary64, max |error| {worst:.3e}")
        assert worst < TOL, worst


def test_tile_rule_takes_larger_tiles_unforced(backend):
    """fcs_tm_rule (csrc/mzx_tuning.h) takes the largest tile that still gives 256 workgroups: 64 rows at a batch of 256 x 64,
    32 rows at 256 x 32 -- the only unforced launches of those two instantiations.  A row's bits do not depend on the tile:
    every output equals the same batch at 16 rows per workgroup, bit for bit."""
    cfg, net, _ = network(SHAPES["w16-splitk"][0], 5)
    for rows in (64, 32):
        B = 256 * rows
        g = torch.Generator().manual_seed(rows)
        obs = torch.rand((B, net.input_size), generator=g)
        act = torch.randint(0, len(cfg.action_space), (B,), generator=g)
        with backend.lib.tuning(fcs_tm=0):
            free = _inferences(net, obs, act)
        with backend.lib.tuning(fcs_tm=16):
            forced = _inferences(net, obs, act)
        for a, b in zip(free[0] + free[1], forced[0] + forced[1]):
            assert a.shape[0] == B and torch.equal(a, b), rows


# (nodes per sample of the store read, of the store written, one store for both)
INDEXED = {"5-to-5": (5, 5, False), "3-to-7": (3, 7, False), "aliased": (5, 5, True)}


def test_indexed_inference_equals_the_dense_call_and_leaves_other_nodes(backend):
    """One recurrent call through node stores with permuted in / out nodes (two workgroups of 16 rows, the second ragged;
    ragged N and K): every output has the bits of the dense call on the gathered rows, the state lands in node out_node[b]
    and nowhere else.  5-to-5: two stores of 5 nodes per sample; 3-to-7: stores of different node counts; aliased: ONE store
    read and written, out_node[b] != in_node[b], the form the searches use -- the nodes not written keep their input."""
    cfg, net, _ = network(wide([72], encoding_size=24, action_space=list(range(18))), 5)
    for case in sorted(INDEXED):
        _indexed_case(backend, net, *INDEXED[case])


def _indexed_case(backend, net, n_in, n_out, aliased):
    B = 21
    g = torch.Generator().manual_seed(8)
    nodes = torch.rand((B, n_in, net.hidden_size), generator=g).to(backend.device)
    if n_in == n_out:
        in_node = torch.stack([torch.randperm(n_in, generator=g)[0] for _ in range(B)])
        out_node = (in_node + 1 + torch.randint(0, n_in - 1, (B,), generator=g)) % n_in
        assert (out_node != in_node).all()
    else:
        in_node = torch.randint(0, n_in, (B,), generator=g)
        out_node = torch.randint(0, n_out, (B,), generator=g)
    act = torch.randint(0, 18, (B,), generator=g)
    rows = torch.arange(B)
    want = net.recurrent_inference(nodes[rows, in_node.to(backend.device)], act)
    before = nodes.clone() if aliased else torch.full((B, n_out, net.hidden_size), float("nan"), device=backend.device)
    out = nodes if aliased else before.clone()
    got = net.recurrent_inference_indexed(nodes, in_node, act, out, out_node)
    for a, b in zip(got, want[:3]):
        assert torch.equal(a, b)
    assert torch.equal(out[rows, out_node.to(backend.device)], want[3])
    untouched = torch.ones((B, n_out), dtype=torch.bool)
    untouched[rows, out_node] = False
    untouched = untouched.to(backend.device)
    assert untouched.sum() == B * (n_out - 1)
    if aliased:
        assert torch.equal(out[untouched], before[untouched])
    else:
        assert torch.isnan(out[untouched]).all()
    assert len(set(in_node.tolist())) == n_in and len(set(out_node.tolist())) == n_out


PER_OP = "one kernel per step of a simulation (select / network / expand + back-propagate)"


def _route(engine, B):
    lib = engine.backend.lib
    route = (lib.mzx_search_route.argtypes[1]._type_)()
    lib.check(lib.mzx_search_route(engine.handle(B), route))
    return int(route[0])


def _expanded_roots(net, obs, legal):
    """Roots expanded from the network's own initial inference, as test_gpu_route_table.observe builds them."""
    _, _, policy, hidden = net.initial_inference(torch.tensor(obs))
    roots = []
    for i in range(len(legal)):
        node = self_play.Node(0)
        node.expand(legal[i], 0, 0.0, policy[i:i + 1].cpu(), hidden[i:i + 1])
        roots.append(node)
    return roots


def _search(cfg, net, B, obs, legal, seeds, roots=None, mode=None):
    engine = self_play.BatchedMCTS(cfg, net, B, mode=mode, max_carried_nodes=2 * cfg.num_simulations + 1)
    rngs = [numpy.random.RandomState(s) for s in seeds]
    if roots is None:
        res = engine.run(list(obs), legal, [0] * B, True, rngs)
    else:
        res = engine.run_from_roots(roots, [0] * B, True, rngs)
    return engine, res, _route(engine, B), _traces(engine.export_trees(B), range(B), legal)


# cell: (actions, roots given, route and kernel of the search on the engine)
SEARCHES = {"fresh-18": (18, False, 2, "fcs_recurrent_kernel"), "from-roots-18": (18, True, 2, "fcs_recurrent_kernel"),
            "generic-300": (300, False, 0, PER_OP)}


@pytest.mark.parametrize("cell", sorted(SEARCHES))
def test_search_on_the_row_route_against_the_per_operator_path(backend, cell):
    """A network outside fc2_search_kernel's plan (128 wide), 33 trees x 16 simulations: the engine's trees against the
    per-operator path of the SAME handle.  fresh-18: 18 actions, mzx_search_run on the row route; from-roots-18: the roots
    expanded from the engine's own initial inference, mzx_search_run_from_roots on both paths with the same roots;
    generic-300: 300 actions, beyond row_search_supported, so the one-thread-per-tree kernels (route 0) run with their network
    calls as indexed calls into the engine.  fp32 summation order differs, so a walk may take the other branch at a
    near-tie: every differing tree must diverge first at a near-tie of the oracle's UCB scores (test_gpu_parity.near_tie),
    and no more trees may differ than twice those on which the per-operator path itself leaves the binary64 oracle."""
    B, S = 33, 16
    A, given, want_route, want_kernel = SEARCHES[cell]
    cfg, net, sd = network(wide([128], action_space=list(range(A)), num_simulations=S), 7, engine="ops")
    obs = torch.rand((B,) + tuple(cfg.observation_shape), generator=torch.Generator().manual_seed(4)).numpy()
    rs = numpy.random.RandomState(2)
    legal = [sorted(rs.choice(A, size=rs.randint(2, A + 1), replace=False).tolist()) for _ in range(B)]
    seeds = [500 + i for i in range(B)]
    net.fc_engine = "streamed"
    roots = _expanded_roots(net, obs, legal) if given else None
    net.fc_engine = "ops"
    _, res_ops, route_ops, tr_ops = _search(cfg, net, B, obs, legal, seeds, roots)
    net.fc_engine = "streamed"
    engine, res, route, tr = _search(cfg, net, B, obs, legal, seeds, roots)
    assert route_ops == 0 and route == want_route and want_kernel in engine.kernel_name(B), (route, engine.kernel_name(B))
    assert (want_kernel == PER_OP) == (engine.kernel_name(B) == PER_OP)
    parity._tree_invariants(cfg, res, S)
    jobs = [(obs[i], legal[i], 0, seeds[i]) for i in range(B)]
    s32 = parallel.run_searches(cfg, sd, jobs)
    s64 = parallel.run_searches(cfg, sd, jobs, dtype_name="float64")
    cap = max(2, 2 * sum(int(t["trace"] != a) for t, a in zip(s64, tr_ops)))
    differing = 0
    for i in range(B):
        k = next((k for k in range(S) if tr[i][k] != tr_ops[i][k]), None)
        if k is None:
            assert list(res.visit_counts[i]) == list(res_ops.visit_counts[i])
            assert abs(res.root_values[i] - res_ops.root_values[i]) < 10 * TOL * max(1.0, abs(res_ops.root_values[i])), i
            continue
        differing += 1
        # the margins of an oracle search that walked the common prefix
        t = next((t for t in (s32[i], s64[i]) if t["trace"][:k] == tr[i][:k]), None)
        assert t is not None, (i, k, "neither oracle search shares the walks before the divergence")
        gap, vgap = t["margins"][k][0], t["value_margins"][k]
        print(f"tree {i} differs from the per-operator path at simulation {k}: oracle UCB top-2 margin {gap:.3e} ({vgap:.3e})")
        assert parity.near_tie(gap, vgap), (i, k, gap, vgap)
    print(f"{cell}: {differing} of {B} trees differ from the per-operator path (cap {cap})")
    assert differing <= cap
    # a continued search on the same handle: the node store the route left serves mzx_search_advance
    pick = [int(numpy.argmax(res.visit_counts[i])) for i in range(B)]
    more = engine.continue_search(pick, [0] * B, True, [numpy.random.RandomState(900 + i) for i in range(B)])
    assert want_kernel in engine.kernel_name(B)
    t = engine.export_trees(B)
    carried = numpy.array([res.visit_counts[i][pick[i]] for i in range(B)])
    assert (t["visit"][:, 0] == carried + S).all() and numpy.isfinite(more.root_values).all() and (more.flags == 0).all()


def test_mode0_walks_the_row_route_trees(backend):
    """The same handle on the engine, searched in mode 0 (mzx_search_set_mode: the one-thread-per-tree kernels, route 0) and
    in the default mode (the row kernels, route 2), 33 trees x 16 simulations, 18 actions.  The network calls are the same
    indexed calls into the engine in both, so their bits are identical and the comparison is between the tree kernels alone;
    those are not documented as summing in different orders but as "bit-identical to the generic operators"
    (csrc/mzx_row_search.h, the header comment on row_select / row_backprop), so traces, visit counts and root values are
    asserted EQUAL, with no near-tie allowance."""
    B, S, A = 33, 16, 18
    cfg, net, _ = network(wide([128], action_space=list(range(A)), num_simulations=S), 7)
    obs = torch.rand((B,) + tuple(cfg.observation_shape), generator=torch.Generator().manual_seed(4)).numpy()
    rs = numpy.random.RandomState(2)
    legal = [sorted(rs.choice(A, size=rs.randint(2, A + 1), replace=False).tolist()) for _ in range(B)]
    seeds = [500 + i for i in range(B)]
    flat, flat_res, flat_route, flat_tr = _search(cfg, net, B, obs, legal, seeds, mode=0)
    assert flat_route == 0 and flat.kernel_name(B) == PER_OP and net.fc_engine == "streamed", flat.kernel_name(B)
    rows, rows_res, rows_route, rows_tr = _search(cfg, net, B, obs, legal, seeds)
    assert rows_route == 2 and "fcs_recurrent_kernel" in rows.kernel_name(B), rows.kernel_name(B)
    assert flat_tr == rows_tr
    assert numpy.array_equal(flat_res.visit_counts, rows_res.visit_counts)
    assert numpy.array_equal(numpy.asarray(flat_res.root_values), numpy.asarray(rows_res.root_values))


def test_switch_off_changes_nothing_and_a_residual_handle_refuses(backend):
    overrides = wide([128], action_space=list(range(18)), num_simulations=8)
    cfg, plain, sd = network(overrides, 7, engine="ops")
    _, toggled, _ = network(overrides, 7)
    toggled.fc_engine = "ops"
    obs = torch.rand((9, plain.input_size), generator=torch.Generator().manual_seed(1))
    act = torch.arange(9) % 18
    for a, b in zip(plain.recurrent_inference(plain.initial_inference(obs)[3], act),
                    toggled.recurrent_inference(toggled.initial_inference(obs)[3], act)):
        assert torch.equal(a, b)
    legal = [list(cfg.action_space)] * 9
    names = []
    for net in (plain, toggled):
        engine, res, route, _ = _search(cfg, net, 9, obs.numpy().reshape((9,) + tuple(cfg.observation_shape)), legal, list(range(9)))
        names.append((route, engine.kernel_name(9), res.visit_counts.tolist(), res.root_values.tolist()))
    assert names[0] == names[1] and names[0][0] == 0
    resnet = models.MuZeroNetwork(configs.tictactoe())
    with pytest.raises(_lib.MzxError, match="residual"):
        resnet.fc_engine = "streamed"
    assert resnet.fc_engine == "ops"
