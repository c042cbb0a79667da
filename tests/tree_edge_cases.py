"""
Shared by the tree edge tests (tests/test_tree_edges.py on the serial build, tests/test_gpu_tree_edges.py on the device):
searches at the action widths where the lane-parallel tree kernels change code path (16|17, 64|65, 128|129, 256|257),
with tie sets that make numpy's masked rejection consume extra tape words, and with walks deeper than a wavefront has lanes.

  * LOCKSTEP_CASES / check_lockstep: GENERATED tables of network outputs through the lock-step ABI (tests/lockstep.py)
    against the CPU oracle (oracle/mcts_oracle.py with its ReplayEvaluator), bit for bit, the tape position included.
    This anchors the per-operator path (mode 0) where the seven recorded fixtures tests/golden/tree_*.npz do not reach.
  * NETWORK_KINDS / network_weights / check_network_precondition: ways to make a real network produce the same situations,
    for the tuned kernels, which compute the network themselves and are held bit for bit to mode 0.

All inputs are rebuilt from seeds (numpy.random.RandomState, float32 only, then widened), so both sides of a comparison
read the same bits.
"""
import functools

import numpy
import torch

import lockstep
from mzx import configs, synthetic
from oracle import mcts_oracle

TAPE_WORDS = 8192      # the lock-step handle has no overflow re-run; the tie-heavy cases draw a few thousand words

# slots either side of a border between two chunks of child slots: 16-lane rows, 64-lane wavefronts
BORDERS = ((15, 16), (63, 64), (127, 128), (191, 192))


def borders(A):
    """The chunk borders an action space of A slots has."""
    return [b for b in BORDERS if b[1] < A]


def ragged_legal(A, B, seed):
    """Tree 0: every action; tree 1: the single action A - 1; the rest: random subsets (sorted) of random sizes."""
    rs = numpy.random.RandomState(seed)
    out = [list(range(A)), [A - 1]]
    for _ in range(2, B):
        out.append(sorted(rs.choice(A, size=rs.randint(1, A + 1), replace=False).tolist()))
    return out[:B]


def _case(kind, A, S, seed, B=3, players=1, noise=False, pb_c_base=19652, pb_c_init=1.25, discount=0.997, **extra):
    name = f"{kind}-a{A}-s{S}" + ("-noise" if noise else "") + (f"-p{players}" if players != 1 else "") + extra.pop("tag", "")
    return dict(name=name, kind=kind, A=A, S=S, B=B, seed=seed, players=players, noise=noise, pb_c_base=pb_c_base,
                pb_c_init=pb_c_init, discount=discount, **extra)


def _lockstep_cases():
    cases = []
    widths = (1, 2, 3, 4, 5, 16, 17, 64, 65, 128, 129, 255, 256, 257, 361)
    for i, A in enumerate(widths):
        # every width: a root that ties A ways (no noise), and a walk through the last slot of every level
        cases.append(_case("flat", A, 40, 100 + i, players=1 + i % 2, discount=(0.997, 1.0, 0.9)[i % 3]))
        cases.append(_case("last", A, 40, 200 + i, players=1 + (i + 1) % 2, pb_c_init=(1.25, 2.5)[i % 2]))
    for i, A in enumerate((3, 17, 65, 129, 257)):
        cases.append(_case("flat", A, 50, 300 + i, noise=True, players=1 + i % 2))
    # the tables used up to a few hundred visits; two actions tie at every level without ever rejecting a word
    cases.append(_case("flat", 2, 300, 310, B=3, players=2, discount=1.0))
    # walks deeper than a wavefront has lanes
    cases.append(_case("last", 129, 70, 320, players=2, discount=1.0))
    cases.append(_case("last", 128, 70, 321, players=1))
    for i, A in enumerate((17, 65, 129, 255, 256, 257, 361)):
        cases.append(_case("pair", A, 48, 400 + i, B=4, players=1 + i % 2, discount=(1.0, 0.997)[i % 2]))
    for i, A in enumerate((5, 17, 129, 257)):
        cases.append(_case("random", A, 60, 500 + i, B=4, players=1 + i % 2, noise=bool(i % 2), pb_c_base=(50, 19652)[i % 2],
                           discount=(0.9, 0.997)[i % 2]))
    cases.append(_case("random", 17, 800, 510, B=3, players=2, noise=True, pb_c_base=50, discount=0.997))
    for i, A in enumerate((4, 65, 256)):
        cases.append(_case("big", A, 60, 600 + i, B=4, players=1 + i % 2, noise=True, discount=0.997))
    for i, (A, c) in enumerate(((3, 5.0), (16, -5.0), (128, 5.0), (257, -5.0))):
        cases.append(_case("constant", A, 50, 700 + i, players=1, discount=1.0, value=c, tag=f"-{'plus' if c > 0 else 'minus'}"))
    return cases


LOCKSTEP_CASES = _lockstep_cases()
LOCKSTEP_BY_NAME = {c["name"]: c for c in LOCKSTEP_CASES}
assert len(LOCKSTEP_BY_NAME) == len(LOCKSTEP_CASES)


def config_of(case):
    return configs.HotPathConfig(action_space=list(range(case["A"])), players=list(range(case["players"])),
                                 pb_c_base=case["pb_c_base"], pb_c_init=case["pb_c_init"], discount=case["discount"],
                                 root_dirichlet_alpha=0.3, num_simulations=case["S"], support_size=10)


def _softmax32(logits):
    """fp32 softmax of a vector, as Node.expand computes the priors (self_play.py:460-462), widened to binary64."""
    logits = numpy.asarray(logits, numpy.float32)
    e = numpy.exp(logits - logits.max()).astype(numpy.float32)
    return (e / e.sum(dtype=numpy.float32)).astype(numpy.float32).astype(numpy.float64)


def _pair_of(case, tree, n):
    """The two slots of tree `tree` that carry the equal maximal priors among n slots."""
    bs = borders(n)
    if bs:
        return bs[(tree + case["seed"]) % len(bs)]
    return (0, n - 1)


def lockstep_tables(case):
    """legal [B] lists, to_play [B], values / rewards [B][S+1], priors [B][S+1][A] (binary64 holding fp32 values).  Row 0 of a
    tree is its root: the first len(legal) slots hold the priors of its legal actions."""
    kind, A, S, B = case["kind"], case["A"], case["S"], case["B"]
    rs = numpy.random.RandomState(case["seed"])
    legal = ragged_legal(A, B, case["seed"] + 1)
    to_play = [i % case["players"] for i in range(B)]
    values = numpy.zeros((B, S + 1), numpy.float32)
    rewards = numpy.zeros((B, S + 1), numpy.float32)
    priors = numpy.zeros((B, S + 1, A), numpy.float64)
    if kind in ("random", "big"):
        scale_v, scale_r = (1.0, 1.0) if kind == "random" else (1e3, 30.0)
        values[:] = (rs.standard_normal((B, S + 1)) * scale_v).astype(numpy.float32)
        if kind == "big":      # magnitudes 1e3 .. 1e5, both signs
            values[:] = (values * numpy.float32(10.0) ** rs.randint(0, 3, size=(B, S + 1)).astype(numpy.float32)).astype(numpy.float32)
        rewards[:] = (rs.standard_normal((B, S + 1)) * scale_r).astype(numpy.float32)
    if kind == "constant":
        values[:] = numpy.float32(case["value"])
    for b in range(B):
        for k in range(S + 1):
            n = len(legal[b]) if k == 0 else A
            if kind == "flat":
                logits = numpy.zeros(n, numpy.float32)
            elif kind == "last":
                logits = numpy.zeros(n, numpy.float32)
                logits[n - 1] = 8.0
            elif kind == "pair":
                logits = numpy.zeros(n, numpy.float32)
                if n >= 2:
                    i, j = _pair_of(case, b, n)
                    logits[i] = logits[j] = 3.0
            else:
                logits = (rs.standard_normal(n) * 2).astype(numpy.float32)
            p = _softmax32(logits)
            if kind in ("random", "big") and n >= 4:      # a few children the policy rules out exactly
                p[rs.choice(n, size=max(1, n // 8), replace=False)] = 0.0
            priors[b, k, :n] = p
    return legal, to_play, values.astype(numpy.float64), rewards.astype(numpy.float64), priors


def rng_inputs(case, cfg, legal):
    """Root noise and the raw-word tape of every tree, as the engine derives them from the tree's RandomState."""
    B, A = case["B"], case["A"]
    noise = numpy.zeros((B, A), numpy.float64) if case["noise"] else None
    tape = numpy.zeros((B, TAPE_WORDS), numpy.uint32)
    for i in range(B):
        rs = numpy.random.RandomState(case["seed"] * 1000 + i)
        if case["noise"]:
            noise[i, : len(legal[i])] = rs.dirichlet([cfg.root_dirichlet_alpha] * len(legal[i]))
        tape[i] = rs.randint(0, 2 ** 32, size=TAPE_WORDS, dtype=numpy.uint32)
    return noise, tape


@functools.lru_cache(maxsize=None)
def oracle_trees(name):
    """The oracle's trees of a case and, per tree, the next raw word of its RandomState after the search.  Computed once
    per process and left unchanged."""
    case = LOCKSTEP_BY_NAME[name]
    cfg = config_of(case)
    legal, to_play, values, rewards, priors = lockstep_tables(case)
    out = []
    for i in range(case["B"]):
        rng = numpy.random.RandomState(case["seed"] * 1000 + i)
        ev = mcts_oracle.ReplayEvaluator(values[i], rewards[i], priors[i])
        tree = mcts_oracle.run_search(cfg, ev, None, legal[i], to_play[i], case["noise"], rng)
        out.append((tree, int(rng.randint(0, 2 ** 32, dtype=numpy.uint32))))
    return out


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


def check_lockstep(backend, case, report=None):
    """The lock-step ABI of `backend` on the case's generated tables against the oracle: every node statistic bit for bit,
    the search outputs, the tape position; then the case's own precondition (it exercises the edge it is for)."""
    cfg = config_of(case)
    A, S, B, name = case["A"], case["S"], case["B"], case["name"]
    legal, to_play, values, rewards, priors = lockstep_tables(case)
    noise, tape = rng_inputs(case, cfg, legal)
    legal_arr = numpy.full((B, A), -1, numpy.int32)
    for i, acts in enumerate(legal):
        legal_arr[i, : len(acts)] = acts
    ls = lockstep.Lockstep(backend, cfg, B, S, tape_words=TAPE_WORDS)
    try:
        got = ls.run(legal_arr, noise, tape, numpy.asarray(to_play, numpy.int32), values, rewards, priors)
    finally:
        ls.close()
    want = oracle_trees(name)
    for c, (tree, next_word) in enumerate(want):
        n = len(tree.visit)
        label = (name, "tree", c)
        assert got["n_nodes"][c] == n == S + 1, label
        assert numpy.array_equal(got["visit"][c, :n], numpy.asarray(tree.visit, numpy.int32)), label
        assert numpy.array_equal(got["parent"][c, :n], numpy.asarray(tree.parent, numpy.int32)), label
        assert numpy.array_equal(got["to_play"][c, :n], numpy.asarray(tree.to_play, numpy.int32)), label
        assert numpy.array_equal(_bits(got["value_sum"][c, :n]), _bits(numpy.asarray(tree.value_sum, numpy.float64))), label
        assert numpy.array_equal(_bits(got["reward"][c, :n]), _bits(numpy.asarray(tree.reward, numpy.float64))), label
        assert numpy.array_equal(_bits(got["minmax"][c]), _bits([tree.minimum, tree.maximum])), label
        for i in range(n):
            k = len(tree.actions[i])
            assert numpy.array_equal(got["child"][c, i, :k], numpy.asarray(tree.child[i], numpy.int32)), label + ("node", i)
            assert numpy.array_equal(_bits(got["prior"][c, i, :k]), _bits(tree.prior[i])), label + ("node", i)
        assert numpy.array_equal(got["visits"][c], numpy.asarray(tree.root_visit_counts(cfg.action_space), numpy.int32)), label
        assert got["root_value"][c] == tree.value_sum[0] / tree.visit[0], label
        assert got["info"][c, 0] == tree.max_depth, label
        assert got["info"][c, 1] == 0, label
        used = int(got["info"][c, 2])
        assert used < TAPE_WORDS and int(tape[c, used]) == next_word, label + ("tape_used", used)
    # ---- the case exercises its edge
    kind = case["kind"]
    depth = [t.max_depth for t, _ in want]
    used = got["info"][:, 2]
    if kind == "flat" and S < A and not case["noise"]:
        assert depth[0] == 1, (name, depth)
        if A & (A - 1):
            assert (used > S).any(), (name, used)      # rejected words: more words than draws
    if kind == "last":
        # the single-action root has nothing to tie: the walk takes the last slot at every level, S plies.  A root with more
        # actions scores all zeros in its first walk (sqrt(0) visits), which the tape decides among all of them: the line
        # through the last slot starts one simulation later unless that draw hit it.
        assert depth[1] == S and depth[0] >= S - 1, (name, depth)
    if kind == "pair":
        assert all(t.tie_draws >= S / 2 for t, _ in want), (name, [t.tie_draws for t, _ in want])
    if kind == "constant":
        assert all(t.minimum == t.maximum == case["value"] for t, _ in want), name
        assert (got["minmax"][:, 0] == got["minmax"][:, 1]).all(), name
    if report is not None:
        report(f"lockstep {name}: A {A} kind {kind} depth {depth} tape_used {used.tolist()} "
               f"draws {[t.tie_draws for t, _ in want]}")
    return got


# ----------------------------------------------------------------------------- real networks that produce the situations

NETWORK_KINDS = ("random", "flat", "last", "pair", "constant", "heads")


def _last_bias(sd, head):
    """Key of the bias of the last Linear layer of a head ('policy' / 'value' / 'reward'), fully connected or residual
    network.  (The residual dynamics network names its reward layers plain `fc`.)"""
    keys = [k for k in sd if head in k and k.endswith(".bias") and sd[k].dim() == 1 and "bn" not in k]
    if head == "reward":
        keys += [k for k in sd if k.startswith("dynamics_network.") and ".fc." in k and k.endswith(".bias")]
    assert keys, (head, list(sd))
    return keys[-1]


def network_weights(net, kind, A, seed=12, pair=None, value_bin=None, heads=None):
    """A state_dict for `net` that makes a search meet the situation `kind`:
       random    synthetic.fill_state_dict
       flat      every tensor zero: equal priors, zero values -- ties at every level
       last      zero, then +8 on the last policy layer's bias at A - 1: the walk takes the last slot at every level
       pair      zero, then +3 at the two bias indices `pair`: two equal maxima
       constant  zero, then +20 on bin `value_bin` of the value head's last bias: every value the same c != 0
       heads     zero, then the last bias of the value head is the row heads[0] and the last bias of the reward head the row
                 heads[1]: with zero weights both heads return exactly those logit rows at every node"""
    assert kind in NETWORK_KINDS, kind
    sd = net.state_dict()
    if kind == "random":
        return synthetic.fill_state_dict(sd, seed)
    sd = {k: torch.zeros_like(v) for k, v in sd.items()}
    if kind in ("last", "pair"):
        key = _last_bias(sd, "policy")
        assert sd[key].numel() == A, (key, sd[key].shape)
        for i in ((A - 1,) if kind == "last" else pair):
            sd[key][i] = 8.0 if kind == "last" else 3.0
    if kind == "constant":
        key = _last_bias(sd, "value")
        sd[key][value_bin] = 20.0
    if kind == "heads":
        for head, row in zip(("value", "reward"), heads):
            key = _last_bias(sd, head)
            row = torch.from_numpy(numpy.array(row, dtype=numpy.float32))
            assert sd[key].shape == row.shape, (key, sd[key].shape, row.shape)
            sd[key] = row.to(sd[key].device)
    return sd


def check_network_precondition(kind, A, S, res, legal, pair=None, trees=None, cfg=None):
    """On the yardstick's result (mode 0): the network kind produced the situation it is for."""
    depth, used = numpy.asarray(res.max_tree_depth), numpy.asarray(res.tape_used)
    if kind == "last":      # (the first walk of a root with several actions is an all-zero tie: see check_lockstep)
        assert depth[0] >= S - 1 and len(legal[0]) == A, (kind, A, depth)
        if len(legal[1]) == 1:
            assert depth[1] == S, (kind, A, depth)
    if kind == "flat" and A > 1:
        assert used[0] > 0, (kind, A, used)
        if A & (A - 1):
            assert (used > S).any(), (kind, A, used)      # a draw among a non-power-of-two tie set rejects words
    if kind == "pair":
        assert used[0] >= S // 2, (kind, A, used)
    if kind == "constant":      # every value the same c != 0; `trees`: the yardstick's exported trees, `cfg`: its config
        v = numpy.asarray(res.root_predicted_values)
        c = v[0]
        assert (v == c).all() and abs(c) > 1, v
        assert cfg.discount == 1 and (trees["reward"] == 0).all(), cfg.discount
        mm = trees["minmax"]
        if len(cfg.players) == 1:      # max <= min for the whole search
            assert (mm[:, 0] == c).all() and (mm[:, 1] == c).all(), (c, mm)
        else:                          # the sign alternates with the player: the bounds are -|c| and |c|
            assert (mm[:, 0] == -abs(c)).all() and (mm[:, 1] == abs(c)).all(), (c, mm)
