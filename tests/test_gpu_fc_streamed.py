"""
The streamed MFMA engine for fully connected networks (mzx_net_set_fc_engine, csrc/mzx_fc_streamed.hip) on the device: both
inferences against the oracle network evaluated in binary64 at the smallest shapes that reach every path of the kernels, a
search on the row route around it against the per-operator path of the same handle, and the switch left off.
"""
import numpy
import pytest
import torch

import test_gpu_parity as parity
from test_gpu_streamed_at_size import _traces
from mzx import _lib, configs, models, self_play
from oracle import net_oracle, parallel

pytestmark = pytest.mark.gpu

TOL = 1e-4      # the project's gate on every logit and on the hidden state


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def wide(width, **kw):
    layers = dict(fc_representation_layers=width, fc_dynamics_layers=width, fc_reward_layers=width, fc_value_layers=width,
                  fc_policy_layers=width)
    return dict(layers, **kw)


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
}


def network(overrides, seed, engine="streamed"):
    cfg = configs.cartpole(**overrides)
    torch.manual_seed(seed)
    net = models.MuZeroNetwork(cfg)
    net.fc_engine = engine
    return cfg, net, net.get_weights()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_inferences_against_binary64(backend, name):
    overrides, B, tm = SHAPES[name]
    cfg, net, sd = network(overrides, 5)
    assert net.fc_engine == "streamed"
    oracle = net_oracle.make_oracle_network(cfg, sd, dtype=torch.float64)
    g = torch.Generator().manual_seed(3)
    obs = torch.rand((B, net.input_size), generator=g)
    act = torch.randint(0, len(cfg.action_space), (B,), generator=g)
    with backend.lib.tuning(fcs_tm=tm):
        init = [t.cpu() for t in net.initial_inference(obs)]
        rec = [t.cpu() for t in net.recurrent_inference(init[3], act)]
    want_init = oracle.initial_inference(obs.double())
    want_rec = oracle.recurrent_inference(init[3].double(), act.view(-1, 1))
    assert torch.equal(init[1].double(), want_init[1].double())          # the -inf / 0 reward row exactly
    for tag, got, want in (("initial", init, want_init), ("recurrent", rec, want_rec)):
        for key, a, b in zip(("value", "reward", "policy", "hidden"), got, want):
            if (tag, key) == ("initial", "reward"):
                continue
            err = (a.double() - b.double()).abs().max().item()
            print(f"{name}: {tag} {key} max |error| {err:.3e}")
            assert a.shape == b.shape and err < TOL, (name, tag, key, err)
    if tm:      # a row's bits depend neither on the tile size nor on the workgroup it falls into
        for a, b in zip(init + rec, list(net.initial_inference(obs)) + list(net.recurrent_inference(init[3], act))):
            assert torch.equal(a, b.cpu()), name


def test_indexed_inference_equals_the_dense_call_and_leaves_other_nodes(backend):
    """One recurrent call through node stores of 5 nodes per sample with permuted in / out nodes (two workgroups of 16 rows,
    the second ragged; ragged N and K): every output has the bits of the dense call on the gathered rows, the state lands in
    node out_node[b] and nowhere else."""
    B, N = 21, 5
    cfg, net, _ = network(wide([72], encoding_size=24, action_space=list(range(18))), 5)
    g = torch.Generator().manual_seed(8)
    nodes = torch.rand((B, N, net.hidden_size), generator=g).to(backend.device)
    in_node = torch.stack([torch.randperm(N, generator=g)[0] for _ in range(B)])
    out_node = (in_node + 1 + torch.randint(0, N - 1, (B,), generator=g)) % N
    act = torch.randint(0, 18, (B,), generator=g)
    poison = torch.full((B, N, net.hidden_size), float("nan"), device=backend.device)
    out = poison.clone()
    got = net.recurrent_inference_indexed(nodes, in_node, act, out, out_node)
    rows = torch.arange(B)
    want = net.recurrent_inference(nodes[rows, in_node.to(backend.device)], act)
    for a, b in zip(got, want[:3]):
        assert torch.equal(a, b)
    assert torch.equal(out[rows, out_node.to(backend.device)], want[3])
    untouched = torch.ones((B, N), dtype=torch.bool)
    untouched[rows, out_node] = False
    assert torch.isnan(out[untouched.to(backend.device)]).all() and len(set(in_node.tolist())) == N == len(set(out_node.tolist()))


def _search(cfg, net, B, obs, legal, seeds):
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=2 * cfg.num_simulations + 1)
    res = engine.run(list(obs), legal, [0] * B, True, [numpy.random.RandomState(s) for s in seeds])
    lib = engine.backend.lib
    route = (lib.mzx_search_route.argtypes[1]._type_)()
    lib.check(lib.mzx_search_route(engine.handle(B), route))
    return engine, res, int(route[0]), _traces(engine.export_trees(B), range(B), legal)


def test_search_on_the_row_route_against_the_per_operator_path(backend):
    """A network outside fc2_search_kernel's plan (128 wide, 18 actions), 33 trees x 16 simulations: the engine's trees
    against the per-operator path of the SAME handle.  fp32 summation order differs, so a walk may take the other branch at a
    near-tie: every differing tree must diverge first at a near-tie of the oracle's UCB scores (test_gpu_parity.near_tie),
    and no more trees may differ than twice those on which the per-operator path itself leaves the binary64 oracle."""
    B, S = 33, 16
    cfg, net, sd = network(wide([128], action_space=list(range(18)), num_simulations=S), 7, engine="ops")
    A = len(cfg.action_space)
    obs = torch.rand((B,) + tuple(cfg.observation_shape), generator=torch.Generator().manual_seed(4)).numpy()
    rs = numpy.random.RandomState(2)
    legal = [sorted(rs.choice(A, size=rs.randint(2, A + 1), replace=False).tolist()) for _ in range(B)]
    seeds = [500 + i for i in range(B)]
    _, res_ops, route_ops, tr_ops = _search(cfg, net, B, obs, legal, seeds)
    net.fc_engine = "streamed"
    engine, res, route, tr = _search(cfg, net, B, obs, legal, seeds)
    assert route_ops == 0 and route == 2 and "fcs_recurrent_kernel" in engine.kernel_name(B), engine.kernel_name(B)
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
    print(f"{differing} of {B} trees differ from the per-operator path (cap {cap})")
    assert differing <= cap
    # a continued search on the same handle: the node store the row route left serves mzx_search_advance
    pick = [int(numpy.argmax(res.visit_counts[i])) for i in range(B)]
    more = engine.continue_search(pick, [0] * B, True, [numpy.random.RandomState(900 + i) for i in range(B)])
    assert "fcs_recurrent_kernel" in engine.kernel_name(B)
    t = engine.export_trees(B)
    carried = numpy.array([res.visit_counts[i][pick[i]] for i in range(B)])
    assert (t["visit"][:, 0] == carried + S).all() and numpy.isfinite(more.root_values).all() and (more.flags == 0).all()


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
