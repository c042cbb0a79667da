"""
GPU parity tests proper (-m gpu): the HIP path, called through the C ABI
(include/mzx.h via mzx._lib), against
  * traces of the unmodified reference (tests/golden/*): lock-step tree
    arithmetic BIT-EXACT; network heads within 1e-4; end-to-end visit counts
    identical; whole games identical;
  * the CPU oracle on seeded inputs at BASELINE.json's full size (C2: 4096 trees x
    50 simulations) through size-independent invariants + a sampled tree-by-tree
    comparison.
"""
import json
import os

import numpy
import pytest
import torch

import at_size
import lockstep
import shipped_shapes
import test_hostcheck_search as common
from conftest import GOLDEN
from mzx import _lib, configs, models, search, self_play, synthetic
from oracle import mcts_oracle, net_oracle, parallel

pytestmark = pytest.mark.gpu

TOL = 1e-4  # BASELINE.json north_star: policy/value logits within 1e-4 of the CPU reference


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


def test_native_library_is_loaded(backend):
    assert backend.lib.mzx_is_device_build() == 1
    with open("/proc/self/maps") as f:
        assert "libmzx.so" in f.read()


@pytest.mark.parametrize("name", ["cartpole", "tictactoe", "connect4", "cartpole_ties", "tictactoe_custom",
                                  "cartpole_custom", "lunarlander_pretrained"])
def test_lockstep_tree_bit_exact(backend, name):
    got = lockstep.run_fixture(backend, name)
    if name == "cartpole_ties":
        assert (got["info"][:, 2] > 3).all()


@pytest.mark.parametrize("engine", ["fused", "per-operator"])
@pytest.mark.parametrize("name", ["fc_cartpole", "fc_cartpole_pretrained", "fc_lunarlander_pretrained", "fc_cartpole_stacked",
                                  "resnet_tictactoe", "resnet_connect4", "resnet_breakout", "resnet_breakout_cnn",
                                  "resnet_cnn_small"])
def test_network_heads_within_tolerance(backend, name, engine):
    z = numpy.load(os.path.join(GOLDEN, f"net_{name}.npz"))
    meta = json.loads(str(z["meta"]))
    cfg = configs.BY_NAME[meta["game"]](**meta["overrides"])
    net = models.MuZeroNetwork(cfg)
    if engine == "per-operator":
        if not net.fused_supported():
            pytest.skip("fully connected networks have one engine outside the search kernel")
        net.set_mode(0)
    else:
        assert net.fused_supported() == (3 if cfg.network == "resnet" else 0)
    assert [k for k, _, _ in meta["keys"]] == list(net.state_dict().keys())
    if "flat_weights" in z.files:
        sd, off = {}, 0
        for k, t in net.state_dict().items():
            if t.dtype.is_floating_point:
                sd[k] = torch.from_numpy(z["flat_weights"][off:off + t.numel()].reshape(tuple(t.shape)).copy())
                off += t.numel()
    else:
        sd = synthetic.fill_state_dict(net.state_dict(), meta["weight_seed"])
    net.set_weights(sd)
    o = net.initial_inference(torch.tensor(z["obs"]))
    r1 = net.recurrent_inference(o[3], torch.tensor(z["act1"]))
    r2 = net.recurrent_inference(r1[3], torch.tensor(z["act2"]))
    o1 = net.initial_inference(torch.tensor(z["obs"][:1]))
    for tag, res in (("init", o), ("rec1", r1), ("rec2", r2), ("init_b1", o1)):
        for key, t in zip(("value", "reward", "policy", "hidden"), res):
            ref, got = z[f"{tag}_{key}"], t.cpu().numpy()
            assert got.shape == ref.shape
            if key == "reward" and tag.startswith("init"):
                assert numpy.array_equal(got, ref)  # -inf / 0 pattern exactly
            else:
                assert numpy.abs(got - ref).max() < TOL, (name, tag, key)
        # decoded scalar: the inverse value transform computes sqrt(1 + 0.004 (|x| + 1.001)) - 1 in fp32, which
        # cancels ~3 digits -- two evaluations of logits that agree to 1e-6 differ by up to ~1e-4 after decoding
        vs = models.support_to_scalar(res[0], cfg.support_size).cpu().numpy()
        assert numpy.allclose(vs, z[f"{tag}_value_scalar"], atol=3 * TOL, rtol=3 * TOL)
    # get_weights round trip in reference format
    back = net.get_weights()
    for k, v in sd.items():
        assert torch.equal(back[k], v)


@pytest.mark.parametrize("kind,mode", [("fc", None), ("resnet", None), ("resnet", 0), ("resnet", 3)],
                         ids=["fc", "resnet-fused", "resnet-per-operator", "resnet-streamed"])
def test_tiny_range_states_within_tolerance(backend, kind, mode):
    """States of range between 0 and 1e-5 (test_hostcheck_search.check_tiny_range): the `scale += 1e-5` branch of the
    min-max scaling with a non-zero range, on every inference engine, against net_oracle within 1e-4."""
    common.check_tiny_range(backend, kind, mode, TOL)


@pytest.mark.parametrize("mode", ["generic", "fused"])
@pytest.mark.parametrize("name", ["cartpole", "tictactoe", "connect4", "cartpole_ties", "tictactoe_custom",
                                  "cartpole_custom", "lunarlander_pretrained"])
def test_search_matches_reference(backend, name, mode, monkeypatch):
    if mode == "generic":
        orig = self_play.BatchedMCTS.__init__
        monkeypatch.setattr(self_play.BatchedMCTS, "__init__",
                            lambda self, *a, **k: orig(self, *a, **{**k, "mode": 0}))
    common.test_search_matches_reference(backend, name)   # whole-search kernel (fully connected or residual)


@pytest.mark.parametrize("name", ["tictactoe", "connect4", "cartpole_synth", "tictactoe_stacked",
                                  "cartpole_synth_stacked"])
def test_whole_game_matches_reference(backend, name):
    common.test_whole_game_matches_reference(backend, name)


@pytest.mark.parametrize("protocol", ["per-object", "per-object-pipelined", "batched", "batched-pipelined"])
def test_refilled_slots_equal_lone_actors_on_device(backend, protocol):
    """SelfPlay.play_rounds on the device (tests/test_selfplay_refill.py runs the host logic on the CPU double): slot s's
    games = a lone actor's seeded seed + s, also when two slot groups take turns on the GPU (a worker thread launches the
    searches on the submitting thread's stream while the main thread steps the other group and pushes its frames)."""
    import test_selfplay_refill as refill

    refill.test_refill_with_stacked_observations_and_fixed_length_games(backend, protocol)


@pytest.mark.parametrize("protocol", ["per-object", "per-object-pipelined", "batched", "batched-pipelined"])
@pytest.mark.parametrize("name", ["tictactoe", "tictactoe-threshold", "connect4"])
def test_refilled_board_game_slots_equal_lone_actors_on_device(backend, name, protocol):
    """The same contract with the real rules and residual networks (ragged game lengths, temperature threshold): a
    tree's arithmetic does not depend on how many trees share the launch."""
    import test_selfplay_refill as refill

    refill.test_slot_games_equal_a_lone_actor_s_sequence(backend, name, protocol)


def test_batched_shard_of_4096_cartpole_games_two_groups_against_one_and_against_the_separate_calls(backend):
    """
    BASELINE C2's shard behind the batched protocol (4096 games, 50 simulations, games of 6 moves, three rounds of
    games): (a) the move behind two library calls (mzx_selfplay_search asynchronous + mzx_selfplay_select, two slot
    groups of 2048 taking turns on the GPU -- the default at this size), (b) one group, (c) one group on the SEPARATE
    calls of rounds 1 - 4 (root_draws, upload, mzx_search_run, download, advance, numpy action draw): the same games,
    slot by slot and field by field, in the same order.
    """
    import copy

    cfg = copy.copy(configs.cartpole())
    cfg.max_moves = 6
    Batched = synthetic.make_synthetic_batched_game(cfg.observation_shape, len(cfg.action_space), len(cfg.players))
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg).state_dict(), 4)
    B, seed = 4096, 1000

    def play(pipeline, fused):
        c = copy.copy(cfg)
        c.self_play_pipeline = pipeline
        sp = self_play.SelfPlay({"weights": weights}, Batched, c, seed, num_games=B)
        sp.engine.fused_move = fused
        out, slots = [], []
        for _ in range(3):
            out += sp.play_rounds(1.0, None)
            slots += sp.finished_slots
        groups = len(sp._live["groups"])
        sp.close_game()
        return out, slots, groups

    a, slots_a, groups_a = play(None, True)
    b, slots_b, groups_b = play(False, True)
    c, slots_c, _ = play(False, False)
    assert groups_a == 2 and groups_b == 1 and len(a) == len(b) == len(c) == 3 * B
    assert slots_a == slots_b == slots_c
    for k in range(0, 3 * B, 7):
        for other in (b, c):
            assert a[k].action_history == other[k].action_history, k
            assert a[k].child_visits == other[k].child_visits and a[k].reward_history == other[k].reward_history, k
            assert numpy.array_equal(numpy.array(a[k].root_values).view(numpy.int64), numpy.array(other[k].root_values).view(numpy.int64)), k
            assert all(numpy.array_equal(x, y) for x, y in zip(a[k].observation_history, other[k].observation_history)), k


def test_pipelined_shard_of_1024_connect4_games_plays_what_one_group_plays(backend):
    """
    1024 per-object connect4 games: two slot groups of 512 taking turns on the GPU against ONE group of 1024 (in
    round 4 the two shard sizes were routed to different engines -- the LDS-resident whole-search kernel below 640 trees, the
    streamed towers above -- whose convolutions sum in different orders, so the claim "which slots share a launch changes
    nothing a slot plays" was not bit-true on the device).  The library now searches a wide network on ONE arithmetic at
    every shard size (csrc/mzx_row_search.h wide_search_route): every game of every slot, field for field.
    """
    from mzx import games as board_games

    def run(pipeline):
        cfg = configs.connect4(num_simulations=12)
        cfg.self_play_pipeline = pipeline
        weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg).state_dict(), 5)
        shard = self_play.SelfPlay({"weights": weights}, board_games.PER_OBJECT["connect4"], cfg, 3, num_games=1024)
        by_slot = {}
        for gh, slot in zip(shard.play_rounds(1.0, None, min_games=1 << 60, max_rounds=14), shard.finished_slots):
            by_slot.setdefault(slot, []).append(gh)
        groups = [g.engine for g in shard._live["groups"]]
        kernels = sorted({e.kernel_name(len(g.slots)) for e, g in zip(groups, shard._live["groups"])})
        shard.close_game()
        return by_slot, kernels

    one, k1 = run(False)
    two, k2 = run(True)
    assert k1 == k2 == ["mzx::rt_search_kernel"], (k1, k2)
    assert one.keys() == two.keys() and len(one) > 100
    for slot in one:
        assert len(one[slot]) == len(two[slot])
        for a, b in zip(one[slot], two[slot]):
            assert a.action_history == b.action_history and a.reward_history == b.reward_history, slot
            assert a.child_visits == b.child_visits and a.root_values == b.root_values, slot


def _tree_invariants(cfg, res, S):
    assert (res.visit_counts.sum(1) == S).all()          # every simulation passes the root once
    assert (res.visit_counts >= 0).all()
    assert (res.flags == 0).all()
    assert (res.max_tree_depth >= 1).all() and (res.max_tree_depth <= S).all()
    assert (res.sum_depth >= S).all() and (res.sum_depth <= res.max_tree_depth.astype(numpy.int64) * S).all()
    assert numpy.isfinite(res.root_values).all()


def _device_trace(engine_factory, cfg, obs, legal, to_play, seeds):
    """(parent, action) of every simulation of each tree, rebuilt from the exported canonical-order trees."""
    B = len(legal)
    engine = engine_factory(B)
    engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(s) for s in seeds])
    t = engine.export_trees(B)
    traces = []
    for i in range(B):
        tr = []
        for n in range(1, int(t["n_nodes"][i])):
            par = int(t["parent"][i, n])
            slot = int(numpy.nonzero(t["child"][i, par] == n)[0][0])
            tr.append((par, legal[i][slot] if par == 0 else slot))
        traces.append(tr)
    return traces


def _compare_sample_with_oracle(cfg, sd, res, obs, legal, to_play, seeds, sample, engine_factory, value_tol, label,
                                traces=None):
    """
    Tree-by-tree comparison of a sample against the CPU oracle (the reference's algorithm with its torch
    network), SIMULATION BY SIMULATION: the (parent, action) of every expansion, rebuilt from the exported
    device trees, against the oracle's trace.  fp32 summation order differs between any two network
    implementations, so a simulation whose best and second-best UCB scores are closer than that noise may take
    the other branch.  For every tree that diverges this finds the FIRST diverging simulation, prints the
    oracle's UCB top-2 margin on that walk (SURVEY.md section 8c') and requires it to be tiny: a divergence with a
    comfortable margin is a bug, not noise.  Trees whose every simulation agrees must also agree on root
    value (tolerance) and maximum depth.  Returns the number of trees identical in every simulation.
    """
    if traces is None:     # (else: the sampled trees of the at-size run itself, exported by the caller)
        traces = _device_trace(engine_factory, cfg, [obs[i] for i in sample], [legal[i] for i in sample],
                               [to_play[i] for i in sample], [seeds[i] for i in sample])
    # the oracle searches run in a pool of single-thread worker processes (oracle/parallel.py): hundreds of trees
    # in seconds on the GPU box's host cores
    jobs = [(obs[i], legal[i], to_play[i], seeds[i]) for i in sample]
    summaries = parallel.run_searches(cfg, sd, jobs)
    # yardstick: the SAME searches with the oracle network evaluated in binary64 -- how often does the reference's own
    # fp32 arithmetic leave exact arithmetic on these trees?  (the device should diverge from the oracle's fp32 about as
    # often, not more)
    exact = parallel.run_searches(cfg, sd, jobs, dtype_name="float64")
    identical = 0
    for i, got, tree in zip(sample, traces, summaries):
        want = tree["trace"]
        k = next((k for k in range(len(want)) if k >= len(got) or got[k] != want[k]), None)
        if k is None:
            identical += 1
            assert tree["root_visit_counts"] == list(res.visit_counts[i]), (label, i)
            rv = tree["root_value"]
            assert abs(res.root_values[i] - rv) < value_tol * max(1.0, abs(rv)), (label, i)
            assert res.max_tree_depth[i] == tree["max_depth"], (label, i)
            continue
        gap, depth = tree["margins"][k]
        vgap = tree["value_margins"][k]
        print(f"{label}: tree {i} diverges at simulation {k} of {len(want)} (oracle {want[k]}, device "
              f"{got[k] if k < len(got) else None}); oracle UCB top-2 margin on that walk {gap:.3e} at depth {depth}"
              f" (in units of the backed-up values: {vgap:.3e})")
        # observed margins of diverging trees: <= 8e-5 (profiles/r02_pytest_gpu_full_v2.log); the gate leaves 6x
        assert near_tie(gap, vgap), (label, i, k, gap, vgap, "divergence with a comfortable UCB margin: not fp32 noise")
    # what the replay buffer consumes (root child_visits, root value) on ALL sampled trees, diverged ones included, with
    # ABSOLUTE per-case bounds (tests/at_size.py; round 5 gated the divergence count relative to the oracle's own fp32-vs-
    # binary64 instability, which cannot fail where that is total)
    stats = at_size.statistics(cfg.num_simulations, [res.visit_counts[i] for i in sample], [res.root_values[i] for i in sample],
                               summaries, exact, identical)
    at_size.gate(label, stats)
    return identical


def weights_for(cfg, net, kind, seed):
    """State dict of an at-size case.  "synthetic": mzx.synthetic.fill_state_dict(seed) (large random weights: the stress
    case).  "reference": what SURVEY.md section 8(d) prescribes and bench.py times -- torch.manual_seed(0);
    models.MuZeroNetwork(config) of the UNMODIFIED reference (oracle/_ref bytecode; skipped where it did not travel).
    "checkpoint": the reference's shipped results/cartpole/model.checkpoint (bench.py's `c2-ckpt`), carried by the
    committed fixture tests/golden/net_fc_cartpole_pretrained.npz."""
    if kind == "synthetic":
        return synthetic.fill_state_dict(net.state_dict(), seed)
    if kind == "checkpoint":
        z = numpy.load(os.path.join(GOLDEN, "net_fc_cartpole_pretrained.npz"), allow_pickle=True)
        sd, off = {}, 0
        for k, t in net.state_dict().items():
            if t.dtype.is_floating_point:
                sd[k] = torch.from_numpy(z["flat_weights"][off:off + t.numel()].reshape(tuple(t.shape)).copy())
                off += t.numel()
        assert off == z["flat_weights"].size
        return sd
    assert kind == "reference"
    from oracle import build_ref
    if not build_ref.available():
        pytest.skip("oracle/_ref not built (no /root/reference at build time)")
    ref_models, _ = build_ref.load()
    torch.manual_seed(0)
    return {k: v.clone() for k, v in ref_models.MuZeroNetwork(cfg).get_weights().items()}


MARGIN_GATE = 5e-4


def near_tie(gap, value_gap):
    """A divergence from the fp32 oracle is fp32 noise when the oracle's best and second-best UCB scores on that walk were a
    near-tie: closer than MARGIN_GATE in score units -- or in units of the backed-up values r + gamma v relative to their
    magnitude (oracle/mcts_oracle.py ``value_margins``).  A score contains (q - min) / (max - min) over the TREE-WIDE range
    (MinMaxStats): in the first simulations of a search that range is a few hundredths, and the 1e-4 round-off of the
    decoded values (fp32 inverse transform) is a 1e-2 step in score units.  Found with the reference
    constructor's breakout weights (round 6): the oracle's OWN fp32 and binary64 searches part at simulation 2 of a tree
    with a score margin of 2.2e-3 -- and the device follows the binary64 line (profiles/r06_at_size_breakout_probe.txt)."""
    return gap < MARGIN_GATE or value_gap < MARGIN_GATE


@pytest.mark.parametrize("mode,weights", [(0, "synthetic"), (1, "synthetic"), (1, "reference"), (1, "checkpoint")])
def test_full_size_c2_cartpole(backend, mode, weights):
    """BASELINE config C2: CartPole-FC, 4096 trees x 50 simulations on one GPU -- on synthetic stress weights (both
    search paths), and on EXACTLY the two weight sets bench.py times: the reference constructor's under
    torch.manual_seed(0) (the headline number's inputs) and the reference's shipped checkpoint (`c2-ckpt`)."""
    cfg = configs.cartpole()
    B, S = 4096, cfg.num_simulations
    net = models.MuZeroNetwork(cfg)
    sd = weights_for(cfg, net, weights, 11)
    net.set_weights(sd)
    engine = self_play.BatchedMCTS(cfg, net, B, mode=0 if mode == 0 else None)
    if mode == 1 and not backend.lib.mzx_search_fused_supported(engine.handle(B)):
        pytest.skip("fused kernel not available")
    obs = synthetic.observations(B, cfg.observation_shape, seed=123)
    legal = [list(cfg.action_space)] * B
    rngs = [numpy.random.RandomState(1000 + i) for i in range(B)]
    res = engine.run(list(obs), legal, [0] * B, True, rngs)
    _tree_invariants(cfg, res, S)
    if mode == 1:
        assert "fc2_search_kernel" in engine.kernel_name(B), engine.kernel_name(B)     # the kernel the headline number times
    # determinism: same inputs, same streams -> identical outputs
    res2 = engine.run(list(obs), legal, [0] * B, True, [numpy.random.RandomState(1000 + i) for i in range(B)])
    assert numpy.array_equal(res.visit_counts, res2.visit_counts)
    assert numpy.array_equal(res.root_values.view(numpy.int64), res2.root_values.view(numpy.int64))
    # 1024 sampled trees (whole-search kernel; 256 on the generic path) against the CPU oracle (reference
    # network arithmetic on the host, oracle searches in a process pool)
    sample = list(range(0, B, 4 if mode == 1 else 16))
    seeds = [1000 + i for i in range(B)]
    factory = lambda n: self_play.BatchedMCTS(cfg, net, n, mode=0 if mode == 0 else 3)
    label = f"C2 mode {mode}" + ("" if weights == "synthetic" else f" ({weights} weights)")
    # fp32 network arithmetic is not bit-reproducible across implementations; a near-tie may flip one simulation on rare
    # trees: each such tree's margin is printed and bounded (MARGIN_GATE), the visit statistics are gated in at_size.GATES
    # (root value of a tree identical in every simulation: 1e-4 on the synthetic weights; the trained checkpoint's values
    # are larger and its decoded scalars carry the 3e-4 of DESIGN.md section 2 -- measured 1.4e-4 on tree 664)
    _compare_sample_with_oracle(cfg, sd, res, obs, legal, [0] * B, seeds, sample, factory,
                                TOL if weights == "synthetic" else 3 * TOL, label)


@pytest.mark.parametrize("players", [1, 2])
def test_generic_and_fused_trees_bit_identical(backend, players):
    """
    The fused kernels (register-resident SmallNet and LDS-weight LdsNet engines) against the
    generic one-kernel-per-operator path ON THE DEVICE: same inline tree arithmetic, same
    canonical fp32 reduction order -> every node statistic must agree bit for bit.
    """
    cfg = configs.cartpole(players=list(range(players)))
    B = 256
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 17))
    obs = synthetic.observations(B, cfg.observation_shape, seed=9)
    rs = numpy.random.RandomState(3)
    legal = [list(cfg.action_space) if i % 5 else [int(rs.randint(0, 2))] for i in range(B)]  # some single-action roots
    to_play = [int(i % players) for i in range(B)]
    outs = {}
    # (the first-generation kernel, mode flag 16, is in instrumented builds only since round 6)
    for name, mode in (("generic", 0), ("fused-small", 3), ("fused-lds", 7)):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        res = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(7 + i) for i in range(B)])
        outs[name] = (res, engine.export_trees(B))
    ref_res, ref_tree = outs["generic"]
    for name in ("fused-small", "fused-lds"):
        res, tree = outs[name]
        assert numpy.array_equal(res.visit_counts, ref_res.visit_counts), name
        assert numpy.array_equal(res.root_values.view(numpy.int64), ref_res.root_values.view(numpy.int64)), name
        assert numpy.array_equal(res.root_predicted_values.view(numpy.int64),
                                 ref_res.root_predicted_values.view(numpy.int64)), name
        assert numpy.array_equal(res.max_tree_depth, ref_res.max_tree_depth) and numpy.array_equal(res.tape_used, ref_res.tape_used)
        for k, v in ref_tree.items():
            a, b = tree[k], v
            if a.dtype == numpy.float64:
                a, b = a.view(numpy.int64), b.view(numpy.int64)
            assert numpy.array_equal(a, b), (name, k)


@pytest.mark.parametrize("num_actions", [3, 6, 16])
def test_fused_lds_engine_other_shapes(backend, num_actions):
    """Fully connected shapes no register specialisation covers (wider, deeper, more actions, stacked obs)."""
    cfg = configs.cartpole(action_space=list(range(num_actions)), stacked_observations=2, encoding_size=10,
                           fc_representation_layers=[12], fc_dynamics_layers=[24, 12], fc_reward_layers=[20],
                           fc_value_layers=[], fc_policy_layers=[33], num_simulations=30)
    B = 96
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 23))
    obs = synthetic.observations(B, net.input_shape, seed=4)
    legal = [list(cfg.action_space)] * B
    outs = []
    for mode in (0, 3):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        assert backend.lib.mzx_search_fused_supported(engine.handle(B))
        res = engine.run(list(obs), legal, [0] * B, True, [numpy.random.RandomState(70 + i) for i in range(B)])
        outs.append((res, engine.export_trees(B)))
    assert numpy.array_equal(outs[0][0].visit_counts, outs[1][0].visit_counts)
    for k, v in outs[0][1].items():
        a, b = outs[1][1][k], v
        if a.dtype == numpy.float64:
            a, b = a.view(numpy.int64), b.view(numpy.int64)
        assert numpy.array_equal(a, b), k


# ----------------------------------------------------------------------------- fused residual engine (MFMA)
RESNET_CASES = {
    "tictactoe": lambda: configs.tictactoe(),
    "connect4": lambda: configs.connect4(),
    "breakout": lambda: configs.breakout(),
    # shapes no BASELINE config has: channel counts that are not multiples of 4 / 16, two blocks, stacked
    # observations, empty and two-layer head MLPs, a 4 x 5 board
    "odd": lambda: configs.tictactoe(
        observation_shape=(2, 4, 5), action_space=list(range(5)), stacked_observations=2, channels=6, blocks=2,
        reduced_channels_reward=3, reduced_channels_value=5, reduced_channels_policy=2,
        resnet_fc_reward_layers=[7, 9], resnet_fc_value_layers=[], resnet_fc_policy_layers=[33]),
    "wide": lambda: configs.connect4(channels=40, blocks=1, observation_shape=(3, 5, 5), action_space=list(range(25)),
                                     resnet_fc_policy_layers=[48, 20]),
    # games/gomoku.py:22-23 geometry (11 x 11 board, 121 actions, two players) with a network small enough for
    # the fused engine: several child slots per lane in the whole-search kernel
    "gomoku": lambda: configs.connect4(observation_shape=(3, 11, 11), action_space=list(range(121)), channels=16, blocks=2,
                                       reduced_channels_reward=2, reduced_channels_value=2, reduced_channels_policy=4,
                                       resnet_fc_reward_layers=[32], resnet_fc_value_layers=[32],
                                       resnet_fc_policy_layers=[32], num_simulations=60, root_dirichlet_alpha=0.3),
    # games/atari.py:58-59 style heads: 18 actions and a support wider than two 16-lane rows (F = 41)
    "widesupport": lambda: configs.tictactoe(observation_shape=(3, 6, 6), action_space=list(range(18)), support_size=20,
                                             channels=8, players=list(range(1))),
}


def _resnet(name, seed=31):
    cfg = RESNET_CASES[name]()
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), seed))
    return cfg, net


@pytest.mark.parametrize("name", sorted(RESNET_CASES))
def test_fused_resnet_operator_by_operator(backend, name):
    """
    Bisection harness: the output tensor of EVERY operator of both programs, fused MFMA engine vs the
    one-kernel-per-operator engine, on a batch that does not fill the last workgroup.
    """
    cfg, net = _resnet(name)
    assert net.fused_supported() == 3
    B = 37
    rs = numpy.random.RandomState(5)
    obs = torch.tensor(rs.rand(B, *net.input_shape).astype(numpy.float32))
    hid = torch.tensor(rs.rand(B, *net.hidden_shape).astype(numpy.float32))
    act = torch.tensor(rs.randint(0, len(cfg.action_space), size=B).astype(numpy.int32))
    for recurrent, x, a in ((0, obs, None), (1, hid, act)):
        covered = 0
        for n_ops in range(1, net.num_operators(recurrent) + 1):
            got = net.debug_prefix(recurrent, 1, n_ops, x, a).cpu().numpy()
            want = net.debug_prefix(recurrent, 0, n_ops, x, a).cpu().numpy()
            err = numpy.abs(got - want).max()
            assert err < 2e-5 * (1.0 + numpy.abs(want).max()), (name, "recurrent" if recurrent else "initial", n_ops, err)
            covered += 1
        assert covered >= 10



def _check_loose_samples_against_oracle(cfg, sd, net, obs, hidden_in, act, outs_fused, loose, label):
    """
    Samples on which the fused engine and the per-operator engine differ by more than the tight bound: compare
    the FUSED outputs with the oracle instead of waiving them.  These are samples with a near-flat plane in
    front of the per-plane min-max scaling (models.py:541-549), where fp32 round-off is divided by the plane's
    range: NO fp32 implementation reproduces the others there -- the reference's own torch arithmetic included.
    So the yardstick is the oracle evaluated in binary64: on every output the fused engine's error against it
    must stay within 1e-4 (north_star) or within a bounded multiple (32x for a single output, 4x in geometric mean
    over the outputs of the sample set) of the error the reference's fp32 arithmetic itself makes on that very
    sample -- measured 2.5e-5 ... 7e-3 on these samples against ~1e-7 elsewhere.  A genuine fused-engine defect
    shows up as an error the fp32 oracle does not have.
    """
    if not len(loose):
        return
    o32 = net_oracle.make_oracle_network(cfg, sd)
    o64 = net_oracle.make_oracle_network(cfg, sd, dtype=torch.float64)
    idx = torch.as_tensor(numpy.asarray(loose))
    h_in = hidden_in.cpu()[idx]
    a = act[idx].long().reshape(-1, 1)
    with torch.no_grad():
        w32 = o32.initial_inference(obs[idx]) + o32.recurrent_inference(h_in, a)
        w64 = o64.initial_inference(obs[idx].double()) + o64.recurrent_inference(h_in.double(), a)
    ratios = []
    for k in range(8):
        got = outs_fused[k][loose].astype(numpy.float64)
        ref64 = w64[k].numpy().reshape(len(loose), -1)
        ref32 = w32[k].numpy().reshape(len(loose), -1).astype(numpy.float64)
        if k == 1:
            assert numpy.array_equal(got, ref32)
            continue
        err_fused = numpy.abs(got - ref64).max(axis=1)
        err_ref32 = numpy.abs(ref32 - ref64).max(axis=1)
        bad = err_fused > numpy.maximum(TOL, 32 * err_ref32)
        print(f"{label}: output {k}: {len(loose)} loose samples, fused-vs-f64 {err_fused.max():.2e}, "
              f"torch-fp32-vs-f64 {err_ref32.max():.2e}")
        assert not bad.any(), (label, k, err_fused[bad].tolist(), err_ref32[bad].tolist())
        ratios += [f / r for f, r in zip(err_fused.tolist(), err_ref32.tolist()) if r > 1e-7 and f > 1e-7]
    # Any single output may sit in the tail (two round-off realisations of one ill-conditioned quotient: the ratio of
    # their errors is heavy-tailed -- measured 1/30 ... 14 on these samples, and UNCHANGED by IEEE division / libm expf,
    # profiles/r03_ieee_math_ab.txt), but a SYSTEMATIC loss of accuracy would move all of a sample's outputs: their
    # geometric-mean ratio must stay below 4
    if ratios:
        gmean = float(numpy.exp(numpy.mean(numpy.log(ratios))))
        print(f"{label}: geometric mean of fused / torch-fp32 error over {len(ratios)} ill-conditioned outputs: {gmean:.2f}")
        assert gmean < 4.0, (label, gmean, ratios)


@pytest.mark.parametrize("batch", [1, 37, 1024])
@pytest.mark.parametrize("name", sorted(RESNET_CASES))
def test_fused_resnet_matches_per_operator_engine(backend, name, batch):
    cfg, net = _resnet(name, seed=8)
    sd = synthetic.fill_state_dict(net.state_dict(), 8)
    if name == "breakout" and batch > 64:
        batch = 64
    rs = numpy.random.RandomState(batch)
    obs = torch.tensor(rs.rand(batch, *net.input_shape).astype(numpy.float32))
    act = torch.tensor(rs.randint(0, len(cfg.action_space), size=batch).astype(numpy.int32))
    outs = {}
    hidden_in = None
    for mode in (0, 1):
        net.set_mode(mode)
        o = net.initial_inference(obs)
        if hidden_in is None:
            hidden_in = o[3]          # both engines continue from the SAME state
        r = net.recurrent_inference(hidden_in, act)
        outs[mode] = [t.cpu().numpy().reshape(batch, -1) for t in o + r]
    net.set_mode(1)
    loose_rows = set()
    for k, (want, got) in enumerate(zip(outs[0], outs[1])):
        assert got.shape == want.shape
        if k == 1:
            assert numpy.array_equal(got, want)   # initial reward: -inf / 0 pattern
            continue
        # the per-plane min-max scaling divides by (max - min), or by 1e-5 for a flat plane
        # (models.py:541-549): on such planes fp32 round-off of the two summation orders is amplified.
        # The bulk of the samples must agree tightly; the few that do not are compared with the ORACLE below
        err = numpy.abs(got - want).max(axis=1)
        tight = err < 5e-5 * (1.0 + numpy.abs(want).max())
        assert int((~tight).sum()) <= max(2, batch // 50), (name, batch, k, float(err.max()))
        loose_rows.update(numpy.nonzero(~tight)[0].tolist())
    _check_loose_samples_against_oracle(cfg, sd, net, obs, hidden_in, act, outs[1], sorted(loose_rows), (name, batch))


@pytest.mark.parametrize("name", ["tictactoe", "connect4"])
def test_search_with_fused_resnet_matches_per_operator_search(backend, name):
    """Whole searches: fused network engine (hidden states indexed in the arena) vs per-operator engine."""
    cfg = RESNET_CASES[name]()
    cfg.num_simulations = 20
    B = 48
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 3))
    obs = synthetic.observations(B, net.input_shape, seed=2)
    rs = numpy.random.RandomState(1)
    legal = [sorted(rs.choice(len(cfg.action_space), size=rs.randint(1, len(cfg.action_space) + 1), replace=False).tolist())
             for _ in range(B)]
    to_play = [int(i % 2) for i in range(B)]
    res = {}
    for mode in (0, 1):
        net.set_mode(mode)
        engine = self_play.BatchedMCTS(cfg, net, B)
        res[mode] = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(50 + i) for i in range(B)])
    net.set_mode(1)
    same = (res[0].visit_counts == res[1].visit_counts).all(axis=1).mean()
    print(f"visit-count match rate fused vs per-operator: {same:.3f}")
    assert same >= 0.95
    assert numpy.abs(res[0].root_values - res[1].root_values).max() < 1e-3


@pytest.mark.parametrize("name,B", [("tictactoe", 70), ("connect4", 19), ("odd", 33), ("breakout", 9), ("wide", 21),
                                    ("gomoku", 13), ("widesupport", 37)])
def test_residual_whole_search_kernel_bit_identical_to_generic(backend, name, B):
    """
    Every simulation in one launch (mzx_resnet_search.h: lane-parallel tree walks on arena-resident trees +
    fused MFMA network) against the generic path (one select / network / expand+backpropagate launch per
    simulation, one thread per tree) ON THE DEVICE: same network kernels, same binary64 tree arithmetic,
    same canonical fp32 reduction order -> every node statistic must agree bit for bit.
    """
    cfg = RESNET_CASES[name]()
    cfg.num_simulations = 30
    # (wide networks -- "connect4": 64 channels -- search on the tower arithmetic by default, whose bit-identity chain is
    # generic == row kernels == rt_search_kernel on the streamed engine: tests/test_gpu_streamed.py,
    # tests/test_gpu_tower_search.py; THIS test is about the LDS-resident kernels)
    backend.lib.tuning_set("wide_towers", 0)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 12))
    obs = synthetic.observations(B, net.input_shape, seed=6)
    rs = numpy.random.RandomState(2)
    A = len(cfg.action_space)
    legal = [sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for _ in range(B)]
    to_play = [int(i % len(cfg.players)) for i in range(B)]
    outs = {}
    for mode in (0, 1):
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        assert backend.lib.mzx_search_fused_supported(engine.handle(B)) == 2
        res = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(90 + i) for i in range(B)])
        outs[mode] = (res, engine.export_trees(B))
    (r0, t0), (r1, t1) = outs[0], outs[1]
    assert numpy.array_equal(r0.visit_counts, r1.visit_counts)
    assert numpy.array_equal(r0.root_values.view(numpy.int64), r1.root_values.view(numpy.int64))
    assert numpy.array_equal(r0.max_tree_depth, r1.max_tree_depth) and numpy.array_equal(r0.tape_used, r1.tape_used)
    for k, v in t0.items():
        a, b = t1[k], v
        if a.dtype == numpy.float64:
            a, b = a.view(numpy.int64), b.view(numpy.int64)
        assert numpy.array_equal(a, b), (name, k)


def test_gomoku_shaped_search_matches_oracle(backend):
    """121 actions (several child slots per lane), two players, ragged legal sets: whole-search kernel vs the CPU oracle."""
    cfg = RESNET_CASES["gomoku"]()
    cfg.pb_c_init = 2.5     # weight on the priors: bushier trees than the one deep chain a random network digs
    B, S = 24, cfg.num_simulations
    net = models.MuZeroNetwork(cfg)
    sd = synthetic.fill_state_dict(net.state_dict(), 33)
    net.set_weights(sd)
    engine = self_play.BatchedMCTS(cfg, net, B)
    assert backend.lib.mzx_search_fused_supported(engine.handle(B)) == 2
    obs = synthetic.observations(B, net.input_shape, seed=5)
    rs = numpy.random.RandomState(4)
    A = len(cfg.action_space)
    legal = [sorted(rs.choice(A, size=rs.randint(2, A + 1), replace=False).tolist()) for _ in range(B)]
    to_play = [int(i % 2) for i in range(B)]
    seeds = [600 + i for i in range(B)]
    res = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(s) for s in seeds])
    _tree_invariants(cfg, res, S)
    for i in range(B):
        assert set(numpy.nonzero(res.visit_counts[i])[0]).issubset(set(legal[i]))
    factory = lambda n: self_play.BatchedMCTS(cfg, net, n, mode=1)
    # root values: a path of d plies is d recurrent inferences of a random (expanding) network deep, so fp32
    # round-off of two network implementations grows with it -- 5e-3 relative here, the visit counts are the gate
    _compare_sample_with_oracle(cfg, sd, res, obs, legal, to_play, seeds, list(range(B)), factory, 50 * TOL, "gomoku-shaped")


# ----------------------------------------------------------------------------- edge cases of the whole-search kernels
def _compare_modes(cfg, net, B, legal, to_play, noise, seeds):
    outs = []
    for mode in (0, 3):   # 3 = whole-search kernel + export of LDS-resident trees to the arena
        engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
        obs = synthetic.observations(B, net.input_shape, seed=B + 1)
        res = engine.run(list(obs), legal, to_play, noise, [numpy.random.RandomState(s) for s in seeds])
        outs.append((res, engine.export_trees(B)))
    (r0, t0), (r1, t1) = outs
    assert numpy.array_equal(r0.visit_counts, r1.visit_counts)
    assert numpy.array_equal(r0.root_values.view(numpy.int64), r1.root_values.view(numpy.int64))
    assert numpy.array_equal(r0.root_predicted_values.view(numpy.int64), r1.root_predicted_values.view(numpy.int64))
    assert numpy.array_equal(r0.max_tree_depth, r1.max_tree_depth) and numpy.array_equal(r0.tape_used, r1.tape_used)
    for k, v in t0.items():
        a, b = t1[k], v
        if a.dtype == numpy.float64:
            a, b = a.view(numpy.int64), b.view(numpy.int64)
        assert numpy.array_equal(a, b), k
    return r1


def _kernel_name(backend, engine, B):
    name = backend.lib.mzx_search_kernel_name(engine.handle(B))
    return name.decode() if name else ""


# Shapes no BASELINE configuration has, chosen so that every operator of recurrent_inference belongs to a fast class
# (head MLP inputs = reduced channels x positions in 129..144, one hidden layer of <= 16): they are routed to the
# small-board kernels of csrc/mzx_resnet_wave.h and exercise their geometry edges.
SMALL_BOARD_CASES = {
    # 4 x 4 = 16 positions: every row of the wave's tile is valid; 16 actions (16-lane child records); channel counts
    # below 16 (padded K chunks / column tiles); two residual blocks
    "wave-4x4": (lambda: configs.tictactoe(observation_shape=(3, 4, 4), action_space=list(range(16)), channels=12, blocks=2,
                                           reduced_channels_reward=9, reduced_channels_value=9, reduced_channels_policy=9,
                                           resnet_fc_reward_layers=[8], resnet_fc_value_layers=[16], resnet_fc_policy_layers=[5]),
                 "mzx::rz_wave_search_kernel"),
    # 2 x 3 board, 6 actions, one player
    "wave-2x3": (lambda: configs.tictactoe(observation_shape=(2, 2, 3), action_space=list(range(6)), players=list(range(1)),
                                           channels=16, blocks=1, reduced_channels_reward=24, reduced_channels_value=23,
                                           reduced_channels_policy=22, resnet_fc_reward_layers=[16], resnet_fc_value_layers=[16],
                                           resnet_fc_policy_layers=[16], discount=0.997),
                 "mzx::rz_wave_search_kernel"),   # 22..24 reduced channels: the 1x1 head convolutions (two column tiles) are not of
                                                  # a fast class and run on the wave kernel's interpreter (rzw_gemm)
    # 3 x 6 = 18 positions: two row tiles, the second with two valid rows; 6 actions (16-lane records in the tile kernel)
    "tile-3x6": (lambda: configs.tictactoe(observation_shape=(3, 3, 6), action_space=list(range(6)), channels=16, blocks=1,
                                           reduced_channels_reward=8, reduced_channels_value=8, reduced_channels_policy=8,
                                           resnet_fc_reward_layers=[16], resnet_fc_value_layers=[16], resnet_fc_policy_layers=[16]),
                 "mzx::rz_tile_search_kernel"),
    # 6 x 8 = 48 positions: three full row tiles, 4 actions (4-lane records), an 81-bin support (wide decode)
    "tile-6x8": (lambda: configs.tictactoe(observation_shape=(2, 6, 8), action_space=list(range(4)), players=list(range(1)),
                                           channels=8, blocks=2, reduced_channels_reward=3, reduced_channels_value=3,
                                           reduced_channels_policy=3, resnet_fc_reward_layers=[16], resnet_fc_value_layers=[16],
                                           resnet_fc_policy_layers=[16], support_size=40, discount=0.997),
                 "mzx::rz_tile_search_kernel"),
}


@pytest.mark.parametrize("case", sorted(SMALL_BOARD_CASES))
def test_small_board_kernels_other_shapes(backend, case):
    """Wave-per-tree / tile-per-wave whole-search kernels == generic path, bit for bit, on boards and head shapes of
    their own, and the launch is routed to the kernel the shape is meant for (no silent fall-back)."""
    make, want_kernel = SMALL_BOARD_CASES[case]
    cfg = make()
    cfg.num_simulations = 20
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 21))
    B = 37
    A = len(cfg.action_space)
    rs = numpy.random.RandomState(7)
    legal = [sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for _ in range(B)]
    to_play = [int(i % len(cfg.players)) for i in range(B)]
    res = _compare_modes(cfg, net, B, legal, to_play, True, [300 + i for i in range(B)])
    assert (res.visit_counts.sum(1) == cfg.num_simulations).all()
    engine = self_play.BatchedMCTS(cfg, net, B)
    obs = synthetic.observations(B, net.input_shape, seed=B + 1)
    engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(300 + i) for i in range(B)])
    assert _kernel_name(backend, engine, B) == want_kernel


def test_baseline_configurations_are_routed_to_their_kernels(backend):
    want = {"cartpole": "mzx::fc2_search_kernel", "tictactoe": "mzx::rz_wave_search_kernel",
            "connect4": "mzx::rt_search_kernel", "breakout": "mzx::rz_tile_search_kernel"}
    for name, kernel in want.items():
        cfg = configs.BY_NAME[name](num_simulations=3)
        net = models.MuZeroNetwork(cfg)
        net.set_weights(synthetic.fill_state_dict(net.state_dict(), 2))
        B = 8
        engine = self_play.BatchedMCTS(cfg, net, B)
        obs = synthetic.observations(B, net.input_shape, seed=1)
        engine.run(list(obs), [list(cfg.action_space)] * B, [0] * B, True, [numpy.random.RandomState(i) for i in range(B)])
        assert _kernel_name(backend, engine, B) == kernel, name
    # the A/B routes of the wide network: the LDS-resident whole-search kernel, the per-simulation launches
    cfg = configs.connect4(num_simulations=3)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 2))
    obs = synthetic.observations(8, net.input_shape, seed=1)
    for tuning, kernel in (({"wide_towers": 0}, "mzx::rz_search_kernel"), ({"rt_search": 0}, "mzx::rb_tower_kernel")):
        with backend.lib.tuning(**tuning):
            engine = self_play.BatchedMCTS(cfg, net, 8)
            engine.run(list(obs), [list(cfg.action_space)] * 8, [0] * 8, True, [numpy.random.RandomState(i) for i in range(8)])
            assert _kernel_name(backend, engine, 8).startswith(kernel), tuning


def test_every_shipped_game_architecture_runs_on_a_tuned_kernel(backend):
    """
    The network / search shapes of EVERY game file the reference ships (games/*.py, restated here where mzx.configs
    does not carry them: the GPU box has no reference tree) must reach a tuned path -- a whole-search kernel or, for
    the two large residual networks, the streamed MFMA engine between the row-per-tree kernels -- never the
    one-thread-per-tree / one-thread-per-output element kernels.  Searches are checked against the CPU oracle.
    """
    shapes = shipped_shapes.shapes()
    tuned = ("mzx::fc2_search_kernel", "mzx::rz_wave_search_kernel", "mzx::rz_tile_search_kernel", "mzx::rz_search_kernel",
             "mzx::rt_search_kernel", "mzx::rb_tower_kernel / mzx::rb_gemm_kernel")
    for name, cfg in shapes.items():
        cfg.num_simulations = 6
        net = models.MuZeroNetwork(cfg)
        sd = synthetic.fill_state_dict(net.state_dict(), 2)
        net.set_weights(sd)
        B = 4
        engine = self_play.BatchedMCTS(cfg, net, B)
        obs = synthetic.observations(B, net.input_shape, seed=1)
        legal = [list(cfg.action_space)] * B
        res = engine.run(list(obs), legal, [0] * B, True, [numpy.random.RandomState(i) for i in range(B)])
        kernel = _kernel_name(backend, engine, B)
        assert kernel.startswith(tuned), (name, kernel)
        if kernel.startswith("mzx::rb_gemm_kernel"):
            assert "row_select_kernel" in kernel, (name, kernel)
        onet = net_oracle.make_oracle_network(cfg, sd)
        tree = mcts_oracle.run_search(cfg, net_oracle.NetworkEvaluator(onet, cfg.support_size), obs[0], legal[0], 0, True,
                                      numpy.random.RandomState(0))
        assert tree.root_visit_counts(cfg.action_space) == list(res.visit_counts[0]), name


@pytest.mark.parametrize("name", ["tictactoe", "breakout"])
def test_tie_tape_overflow_through_the_small_board_kernels(backend, name):
    """
    A network whose priors are all equal ties at every selection level: the tie tape of a tree overflows, the kernel
    flags it (TF_TAPE_OVERFLOW in the tree's records -> arena meta), BatchedMCTS.run re-runs the flagged trees with a
    longer tape.  Short tape == long tape, on the wave-per-tree (tic-tac-toe) and tile-per-wave (breakout) kernels.
    """
    cfg = configs.BY_NAME[name](num_simulations=20)
    net = models.MuZeroNetwork(cfg)
    net.set_weights({k: torch.zeros_like(v) for k, v in net.state_dict().items()})
    B = 5
    obs = synthetic.observations(B, net.input_shape, seed=3)
    legal = [list(cfg.action_space)] * B
    outs = []
    old = search.TAPE_WORDS      # (the engine reads the module constant of mzx.search; mzx.self_play only re-exports its value)
    try:
        for words, mode in ((4, None), (4096, None), (4096, 0)):
            search.TAPE_WORDS = words
            engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
            res = engine.run(list(obs), legal, [0] * B, True, [numpy.random.RandomState(40 + i) for i in range(B)])
            outs.append(res)
    finally:
        search.TAPE_WORDS = old
    short, long_, per_operator = outs
    assert (short.tape_used > 4).any()
    assert numpy.array_equal(short.visit_counts, long_.visit_counts)
    assert numpy.array_equal(short.root_values.view(numpy.int64), long_.root_values.view(numpy.int64))
    assert numpy.array_equal(short.tape_used, long_.tape_used) and (short.flags == 0).all()
    # ... and the long-tape result is the per-operator path's (mode 0), bit for bit: ties among up to nine children, whose
    # draws reject tape words, so the tape position is part of the comparison
    assert (long_.tape_used < 4096).all(), long_.tape_used
    assert numpy.array_equal(long_.visit_counts, per_operator.visit_counts)
    assert numpy.array_equal(long_.root_values.view(numpy.int64), per_operator.root_values.view(numpy.int64))
    assert numpy.array_equal(long_.root_predicted_values.view(numpy.int64), per_operator.root_predicted_values.view(numpy.int64))
    assert numpy.array_equal(long_.max_tree_depth, per_operator.max_tree_depth)
    assert numpy.array_equal(long_.tape_used, per_operator.tape_used), (long_.tape_used, per_operator.tape_used)
    assert (long_.flags == 0).all() and (per_operator.flags == 0).all()


@pytest.mark.parametrize("net_name", ["cartpole", "tictactoe"])
@pytest.mark.parametrize("B,S,noise", [(1, 1, True), (1, 40, False), (17, 3, True), (257, 7, False)])
def test_whole_search_kernels_edge_shapes(backend, net_name, B, S, noise):
    """
    One tree, one simulation, batches that do not fill the last workgroup / wave row, no exploration noise
    (NULL noise pointer), single-action roots: whole-search kernels == generic path, bit for bit.
    """
    cfg = configs.BY_NAME[net_name](num_simulations=S)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 77))
    A = len(cfg.action_space)
    rs = numpy.random.RandomState(B * 131 + S)
    legal = [[int(rs.randint(0, A))] if i % 3 == 0 else sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist())
             for i in range(B)]
    to_play = [int(i % len(cfg.players)) for i in range(B)]
    res = _compare_modes(cfg, net, B, legal, to_play, noise, [500 + i for i in range(B)])
    assert (res.visit_counts.sum(1) == S).all()
    for i in range(B):
        assert set(numpy.nonzero(res.visit_counts[i])[0]).issubset(set(legal[i]))


def test_zero_simulations(backend):
    """num_simulations = 0: the root alone (self_play.py:319 loop body never runs)."""
    for name in ("cartpole", "tictactoe"):
        cfg = configs.BY_NAME[name](num_simulations=0)
        net = models.MuZeroNetwork(cfg)
        net.set_weights(synthetic.fill_state_dict(net.state_dict(), 1))
        B = 5
        engine = self_play.BatchedMCTS(cfg, net, B)
        obs = synthetic.observations(B, net.input_shape, seed=3)
        res = engine.run(list(obs), [list(cfg.action_space)] * B, [0] * B, True, [numpy.random.RandomState(i) for i in range(B)])
        assert (res.visit_counts == 0).all() and (res.root_values == 0).all() and (res.max_tree_depth == 0).all()


@pytest.mark.parametrize("name,B,n_sample,weights", [
    ("tictactoe", 1024, 256, "synthetic"), ("connect4", 1024, 256, "synthetic"), ("connect4-ws", 1024, 64, "synthetic"),
    ("breakout", 64, 32, "synthetic"),
    # exactly what bench.py times (reference constructor weights): C3, C5 at BASELINE's 64 trees per GPU and at 512 trees on
    # one GPU (`c5-512`); C4 on these weights: tests/test_gpu_streamed_at_size.py (connect4-1024) + tests/test_gpu_tower_search.py
    ("tictactoe", 1024, 256, "reference"), ("breakout", 64, 32, "reference"), ("breakout", 512, 64, "reference"),
    ("connect4", 1024, 64, "reference")])
def test_full_size_residual_configs(backend, name, B, n_sample, weights):
    """
    BASELINE configs C3 (tic-tac-toe, 1024 trees x 25 simulations), C4 (connect4, 1024 x 200) and C5 (breakout
    96x96x3 with the resnet down-sampling stem, 64 trees per GPU x 50 simulations; 512 on one GPU) at full size on the
    whole-search kernel: size-independent invariants, determinism, and a sample of trees against the CPU
    oracle (the reference's algorithm with its torch network) -- trace by trace, and the visit statistics the replay
    buffer consumes against absolute bounds (tests/at_size.py).
    """
    want_kernel = {"connect4": "mzx::rt_search_kernel", "connect4-ws": "mzx::rz_search_kernel"}.get(name, "mzx::rz_")
    label = f"{name} x {B}" + ("" if weights == "synthetic" else f" ({weights} weights)")
    if name == "connect4-ws":      # bench.py's `c4-ws`: the LDS-resident whole-search kernel at the 1024-tree shard
        backend.lib.tuning_set("wide_towers", 0)
        name = "connect4"
    cfg = configs.BY_NAME[name](**({"num_simulations": 50} if name == "breakout" else {}))
    S = cfg.num_simulations
    net = models.MuZeroNetwork(cfg)
    sd = weights_for(cfg, net, weights, 21)
    net.set_weights(sd)
    engine = self_play.BatchedMCTS(cfg, net, B)
    assert backend.lib.mzx_search_fused_supported(engine.handle(B)) == 2
    obs = synthetic.observations(B, net.input_shape, seed=77)
    rs = numpy.random.RandomState(8)
    A = len(cfg.action_space)
    legal = [sorted(rs.choice(A, size=rs.randint(2, A + 1), replace=False).tolist()) for _ in range(B)]
    to_play = [int(i % len(cfg.players)) for i in range(B)]
    seeds = [4000 + i for i in range(B)]
    res = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(s) for s in seeds])
    _tree_invariants(cfg, res, S)
    for i in range(B):
        assert set(numpy.nonzero(res.visit_counts[i])[0]).issubset(set(legal[i]))
    res2 = engine.run(list(obs), legal, to_play, True, [numpy.random.RandomState(s) for s in seeds])
    assert numpy.array_equal(res.visit_counts, res2.visit_counts)
    assert numpy.array_equal(res.root_values.view(numpy.int64), res2.root_values.view(numpy.int64))
    sample = list(range(0, B, B // n_sample))
    # the sampled trees OF THIS RUN (residual kernels keep / write back their trees in the arena), whatever kernel the
    # library routed the shard to: connect4 runs on rt_search_kernel (every simulation in one launch, towers inside), as
    # `connect4-ws` on the LDS-resident rz_search_kernel
    kernel = _kernel_name(backend, engine, B)
    print(f"{label}: {B} trees on {kernel}")
    assert kernel.startswith(want_kernel)
    exported = engine.export_trees(B)
    traces = []
    for i in sample:
        tr = []
        for n in range(1, int(exported["n_nodes"][i])):
            par = int(exported["parent"][i, n])
            slot = int(numpy.nonzero(exported["child"][i, par] == n)[0][0])
            tr.append((par, legal[i][slot] if par == 0 else slot))
        traces.append(tr)
    # fp32 summation order differs between implementations; with 200 simulations of a 64-channel network a near-tie flips
    # somewhere in some trees.  Every divergence is printed with its UCB margin and bounded in the helper (MARGIN_GATE);
    # the share of trees identical in EVERY simulation, the share with equal root visit counts and the distance of the
    # visit distributions are reported and gated per case (at_size.GATES)
    _compare_sample_with_oracle(cfg, sd, res, obs, legal, to_play, seeds, sample, None, 10 * TOL, label, traces=traces)


# ---- observation pipeline + Reanalyse: device twins of tests/test_observations.py

import test_observations as obs_common  # noqa: E402


def test_obs_stack_matches_reference_arrays(backend):
    obs_common.test_stack_history_bit_exact(backend)


@pytest.mark.parametrize("shape,k,A,G,moves", [((3, 3, 3), 2, 9, 5, 7), ((1, 1, 4), 3, 2, 3, 9), ((2, 4, 6), 4, 5, 4, 3),
                                               ((3, 4, 4), 0, 3, 2, 4)])
def test_frame_store_ring_bit_exact(backend, shape, k, A, G, moves):
    obs_common.check_frame_store(backend, shape, k, A, G, moves)


def test_frame_store_full_size_atari_shape(backend):
    """games/atari.py geometry: 3x96x96 frames, 32 stacked -> 131 planes, 64 games; the ring wraps."""
    obs_common.check_frame_store(backend, (3, 96, 96), 32, 4, 64, 35, probe={0, 31, 63})


def test_obs_stack_rejects_bad_arguments(backend):
    obs_common.test_obs_stack_rejects_bad_arguments(backend)


def test_support_to_scalar_device(backend):
    obs_common.test_support_to_scalar_matches_oracle(backend)


@pytest.mark.parametrize("name", ["tictactoe_stacked", "cartpole_synth_stacked"])
def test_reanalyse_matches_reference(backend, name):
    obs_common.check_reanalyse(backend, name)


def test_reanalyse_long_game_matches_oracle(backend):
    """A 300-position connect4-shaped history in one batched initial_inference against the oracle network."""
    cfg = configs.connect4(stacked_observations=1)
    rs = numpy.random.RandomState(11)
    gh = self_play.GameHistory()
    T = 300
    gh.observation_history = [rs.randint(-1, 2, size=cfg.observation_shape).astype("int32") for _ in range(T + 1)]
    gh.action_history = [0] + [int(a) for a in rs.randint(0, len(cfg.action_space), size=T)]
    gh.root_values = [0.0] * T
    template = models.MuZeroNetwork(cfg).state_dict()
    weights = synthetic.fill_state_dict(template, 5)
    from mzx import replay
    worker = replay.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, cfg)
    got = worker.reanalyse_game(gh)
    net = net_oracle.make_oracle_network(cfg, weights)
    A = len(cfg.action_space)
    obs = numpy.array([mcts_oracle.stacked_observations(gh.observation_history, gh.action_history, i, 1, A) for i in range(T)])
    with torch.no_grad():
        want = torch.squeeze(net_oracle.support_to_scalar(net.initial_inference(torch.tensor(obs).float())[0],
                                                          cfg.support_size)).numpy()
    assert got.shape == want.shape == (T,)
    assert numpy.allclose(got, want, atol=3 * TOL, rtol=3 * TOL), numpy.abs(got - want).max()


# ---- replay hand-off: initial PER priorities on the device

def test_replay_priorities_on_device_match_the_reference(backend):
    """
    mzx_replay_priorities (csrc/mzx_replay.h) on the device against what the UNMODIFIED ReplayBuffer.save_game computed
    (replay_buffer.py:39-51, :230-262) for records of seeded games -- tests/golden/replay_priorities.npz, written by
    oracle/make_golden.py --replay-priorities from the imported reference: float32 priorities and game priorities BIT FOR BIT
    (PER_alpha 0.5 / 1: binary64 sqrt / identity behind bit-exact binary64 targets); one / two players, integer and float
    rewards, unvisited roots, horizons longer and shorter than the games, discount 1.
    """
    from mzx import replay
    import types

    z = numpy.load(os.path.join(GOLDEN, "replay_priorities.npz"))
    meta = json.loads(str(z["meta"]))
    checked = 0
    for c, cfg in enumerate(meta["configs"]):
        config = types.SimpleNamespace(PER=True, **cfg)
        for q in range(len(meta["shapes"])):
            key = f"c{c}_q{q}"
            pri, top, targets = replay.device_priorities(backend, z[key + "_root_values"], z[key + "_to_play"], z[key + "_rewards"],
                                                         config, want_targets=True)
            want, want_top = z[key + "_priorities"], z[key + "_game_priority"]
            assert pri.dtype == numpy.float32 and pri.shape == want.shape
            assert numpy.array_equal(pri.view(numpy.int32), want.view(numpy.int32)), (cfg, q, float(numpy.abs(pri - want).max()))
            assert numpy.array_equal(top.view(numpy.int32), want_top.view(numpy.int32)), (cfg, q)
            checked += pri.size
    assert checked > 20000


@pytest.mark.parametrize("alpha", [0.5, 1, 0.7])
def test_replay_hand_off_of_shard_records_on_device(backend, alpha):
    """fill_initial_priorities_many(..., backend) on shard records and plain histories ON THE DEVICE against the per-game host
    function (itself bit-identical to the reference, tests/test_replay_handoff.py); targets against the restatement of
    compute_target_value as binary64 bit patterns.  PER_alpha = 0.7 (no shipped configuration): the device's pow, held to
    one float32 ulp."""
    import test_replay_handoff as handoff

    handoff.check_device_priorities(backend, dict(td_steps=50, discount=0.997, PER_alpha=alpha), exact_pow=False)
    handoff.check_device_priorities(backend, dict(td_steps=5, discount=0.9, PER_alpha=alpha), exact_pow=False)


def test_native_rounds_on_device_equal_the_python_loop(backend):
    """mzx_selfplay_rounds (csrc/mzx_actor.h) on the device: BASELINE C2's shard shape in small (512 synthetic games, two slot
    groups, asynchronous searches behind events) and 96 connect4 games on the residual engine against SelfPlay._rounds_batched
    on the same game objects -- every game field for field, same order, same stream states."""
    import test_native_rounds as native

    from mzx import games

    games.NativeBatchedGame.backend = backend
    cfg = configs.cartpole(max_moves=6)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg).state_dict(), 4)
    Native = games.make_native_synthetic_game(cfg.observation_shape, len(cfg.action_space), len(cfg.players))
    calls = [(1.0, {}), (0.5, dict(max_rounds=4, min_games=1 << 60)), (1.0, dict(min_games=1500))]
    # BASELINE C2's shard as bench.py's self-play legs play it: 4096 games, two slot groups (the second on its own stream)
    a = native._run(backend, Native, cfg, weights, 4096, 1000, calls[:2] + [(1.0, dict(min_games=9000))], True, None)
    b = native._run(backend, Native, cfg, weights, 4096, 1000, calls[:2] + [(1.0, dict(min_games=9000))], False, None)
    assert a[4] and not b[4] and a[3] == b[3] == 2
    native._assert_equal_runs(a, b)
    cfg = configs.connect4(num_simulations=10)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg).state_dict(), 5)
    calls = [(1.0, dict(min_games=40)), (0.25, dict(min_games=100))]
    a = native._run(backend, games.Connect4Native, cfg, weights, 96, 3, calls, True, False)
    b = native._run(backend, games.Connect4Batched, cfg, weights, 96, 3, calls, False, False)
    assert a[4] and not b[4]
    native._assert_equal_runs(a, b)


def test_continuous_self_play_overlapped_hand_off_on_device(backend):
    """continuous_self_play on a natively played shard ON THE DEVICE: rounds on a worker thread (the submitting thread's
    stream), the hand-off -- mzx_actor_take by sequence, mzx_replay_priorities per record, save_game per game -- on the main
    thread meanwhile; the same games with the same priorities in the same order as with the hand-off strictly in turn."""
    import test_native_rounds as native

    from mzx import games

    games.NativeBatchedGame.backend = backend
    native.test_continuous_self_play_hands_native_games_off_while_the_next_call_plays(backend, True)


# ---- reference-compat facade: Node graph + override_root_with on the device

import test_virtual_trajectory as virtual_common  # noqa: E402


@pytest.mark.parametrize("name", ["cartpole", "tictactoe"])
def test_virtual_trajectory_matches_reference(backend, name):
    virtual_common.check_virtual_trajectory(backend, name)


def test_override_root_rejections(backend):
    virtual_common.test_override_root_rejections(backend)


@pytest.mark.parametrize("name", ["cartpole", "lunarlander"])
def test_fc_override_roots_on_the_whole_search_kernel(backend, name):
    """
    MCTS.run(..., override_root_with=root) (self_play.py:275-277; diagnose_model.py:57-74) for a batch of roots on the
    fully connected whole-search kernel: fc2_search_kernel takes the given hidden states / priors / rewards in place of
    its initial_inference (round 4; rounds 1-3 ran this on the per-operator path).  Every statistic of the finished
    trees bit for bit against the per-operator path, for both network engines of the kernel (register-resident
    CartPole shape, LDS weights), ragged legal sets, both noise settings.
    """
    cfg = configs.BY_NAME[name](num_simulations=30)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 17))
    A, B = len(cfg.action_space), 37
    rs = numpy.random.RandomState(3)
    obs = torch.tensor(synthetic.observations(B, net.input_shape, seed=9))
    hidden0 = net.initial_inference(obs)[3]
    act = torch.tensor(rs.randint(0, A, size=B).astype(numpy.int32))
    value, reward, policy, hidden = net.recurrent_inference(hidden0, act)
    rewards = models.support_to_scalar(reward, cfg.support_size).cpu().numpy().reshape(-1)
    legal = [sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()) for _ in range(B)]

    def roots():
        out = []
        for i in range(B):
            node = self_play.Node(0)
            node.expand(legal[i], 0, float(rewards[i]), policy[i:i + 1].cpu(), hidden[i:i + 1])
            out.append(node)
        return out

    for noise in (True, False):
        got = {}
        for mode in (0, 3):        # 3 = whole-search kernel + export of its LDS trees to the arena
            engine = self_play.BatchedMCTS(cfg, net, B, mode=mode)
            res = engine.run_from_roots(roots(), [0] * B, noise, [numpy.random.RandomState(700 + i) for i in range(B)])
            assert ("fc2_search_kernel" in engine.kernel_name(B)) == (mode == 3), engine.kernel_name(B)
            got[mode] = (res, engine.export_trees(B))
        (r0, t0), (r1, t1) = got[0], got[3]
        assert (r0.visit_counts.sum(1) == cfg.num_simulations).all()
        assert numpy.array_equal(r0.visit_counts, r1.visit_counts)
        assert numpy.array_equal(r0.root_values.view(numpy.int64), r1.root_values.view(numpy.int64))
        assert numpy.array_equal(r0.max_tree_depth, r1.max_tree_depth) and numpy.array_equal(r0.tape_used, r1.tape_used)
        for key in ("visit", "value_sum", "reward", "prior", "child", "parent", "to_play", "minmax", "n_nodes"):
            a, b = t0[key], t1[key]
            if a.dtype == numpy.float64:
                a, b = a.view(numpy.int64), b.view(numpy.int64)
            assert numpy.array_equal(a, b), (name, noise, key)


# ---- randomised configurations (tests/test_random_configs.py) on the device, every engine

import test_random_configs as random_common  # noqa: E402


@pytest.mark.parametrize("seed", range(24))
def test_random_config_matches_oracle_all_engines(backend, seed):
    """Per-operator path (mode 0) vs the CPU oracle, and the whole-search kernels (mode 3) bit-identical to it."""
    random_common.check_random_config(backend, seed, modes=(0, 3))


@pytest.mark.parametrize("batch", [300, 777, 2000])
@pytest.mark.parametrize("seed", [1, 3, 5, 7, 9, 11, 13, 15])
def test_random_residual_networks_fused_vs_per_operator(backend, seed, batch):
    """
    Random residual configurations (tests/test_random_configs.py) at batch sizes that put several trees into a
    workgroup: shared slots / wave teams / work words / offset tables of the fused engine against the
    per-operator kernels, both programs.
    """
    cfg, _ = random_common.random_config(seed)
    assert cfg.network == "resnet"
    net = models.MuZeroNetwork(cfg)
    sd = synthetic.fill_state_dict(net.state_dict(), 400 + seed)
    net.set_weights(sd)
    if not net.fused_supported():
        pytest.skip("shape outside the fused engine")
    rs = numpy.random.RandomState(batch + seed)
    obs = torch.tensor(rs.rand(batch, *net.input_shape).astype(numpy.float32))
    act = torch.tensor(rs.randint(0, len(cfg.action_space), size=batch).astype(numpy.int32))
    outs, hidden_in = {}, None
    for mode in (0, 1):
        net.set_mode(mode)
        o = net.initial_inference(obs)
        if hidden_in is None:
            hidden_in = o[3]
        r = net.recurrent_inference(hidden_in, act)
        outs[mode] = [t.cpu().numpy().reshape(batch, -1) for t in o + r]
    loose_rows = set()
    for k, (want, got) in enumerate(zip(outs[0], outs[1])):
        if k == 1:
            assert numpy.array_equal(got, want)
            continue
        err = numpy.abs(got - want).max(axis=1)
        tight = err < 5e-5 * (1.0 + numpy.abs(want).max())
        assert int((~tight).sum()) <= max(2, batch // 50), (seed, batch, k, float(err.max()))
        loose_rows.update(numpy.nonzero(~tight)[0].tolist())
    _check_loose_samples_against_oracle(cfg, sd, net, obs, hidden_in, act, outs[1], sorted(loose_rows), (seed, batch))
