"""
Poisoned arenas, workspaces and outputs: what include/mzx.h calls scratch ("its contents need NOT persist between calls")
may hold anything when a call begins, and what it calls an output is written by the call, every element of it.  The package
and the other tests always hand over zeros (backend.zeros), so a kernel that reads a pad word, a halo, a dead slot row or a
gap between regions before anyone wrote it, or that leaves "0 if not a child" to the allocation, passes them all.  Here every
such buffer is filled with a pattern before the call and the outputs are compared BIT FOR BIT with the run that got zeros: no
tolerance anywhere, only equalities between runs that differ in bytes the contract calls irrelevant.

Patterns (fill):
  ZERO   what the package hands over today: the baseline
  ONES   every byte 0xFF: -1 as int32 (the library's own "none"), NaN as binary32 / binary64
  WORD1  every 32-bit word 1: as int32 a node, a slot and an action that exist at every shape here (num_nodes >= 2, A >= 2);
         1.4e-45 as binary32, 2.1e-314 as a binary64 pair: non-zero and finite
  STALE  what a finished call of ANOTHER shape left in the same tensor (another num_trees / batch / case)
No random bytes, on purpose: a stale read has to show up as different output bits, not as a wild index into memory the call
does not own -- each pattern is a value the code under test could meet as a valid word of its own layout.

Outputs are pre-filled with a sentinel (-7 for integers, a NaN with a payload of its own for floating types -- a kernel
that writes NaN is told apart from one that writes nothing); no sentinel may survive.

The search part (search_cell) runs one cell of tests/test_gpu_route_table.py's table through the raw ABI with its own
mzx_search_io; the CPU twin (test_poisoned_buffers.py) runs it on the serial build, where every cell takes the per-operator
path, the GPU file (test_gpu_poisoned_buffers.py) on the device, where mzx_search_kernel_name must name the table's kernel.
"""
import ctypes

import numpy
import torch

from mzx import _lib, _rng, models, search, synthetic

ZERO, ONES, WORD1, STALE = "ZERO", "ONES", "WORD1", "STALE"
PATTERNS = (ZERO, ONES, WORD1, STALE)

INT_SENTINEL = -7
_NAN32, _NAN64 = 0x7FC00707, 0x7FF8000000000707       # quiet NaNs no arithmetic here produces


def _bytes(t):
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


def fill(tensor, pattern, stale=None):
    """Fill every byte of ``tensor`` (any dtype, contiguous) in place; STALE: zeros, then ``stale(tensor)`` runs the call of
    another shape that leaves its bytes there."""
    raw = _bytes(tensor)
    if pattern == ZERO:
        raw.zero_()
    elif pattern == ONES:
        raw.fill_(0xFF)
    elif pattern == WORD1:
        raw.zero_()
        raw[0::4] = 1                      # little-endian 0x00000001 in every word (and in a ragged tail)
    elif pattern == STALE:
        raw.zero_()
        stale(tensor)
    else:
        raise ValueError(pattern)
    return tensor


def sentinel(tensor):
    """Pre-fill an output."""
    if tensor.dtype == torch.float32:
        tensor.view(torch.int32).fill_(_NAN32)
    elif tensor.dtype == torch.float64:
        tensor.view(torch.int64).fill_(_NAN64)
    else:
        tensor.fill_(INT_SENTINEL)
    return tensor


def bits(a):
    """Bit patterns of a numpy array (floating types as integers of their width)."""
    a = numpy.ascontiguousarray(a)
    return a.view({4: numpy.int32, 8: numpy.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def untouched(a):
    """Mask of the elements of a downloaded output that still hold the sentinel."""
    a = numpy.ascontiguousarray(a)
    if a.dtype == numpy.float32:
        return a.view(numpy.int32) == _NAN32
    if a.dtype == numpy.float64:
        return a.view(numpy.int64) == _NAN64
    return a == INT_SENTINEL


def same_bits(got, want, what):
    for k in want:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape and numpy.array_equal(g, w), (what, k, numpy.argwhere(g != w)[:4].tolist())


# ------------------------------------------------------------------------------------------------------------ searches

B, SIMS, B_STALE = 5, 6, 7           # trees, simulations; the shard size whose finished search is the STALE pattern
ENTRIES = ("run", "from_roots", "continued", "selfplay_search", "run_export")
DUMP_FIELDS = ("visit", "value_sum", "reward", "to_play", "parent", "child", "prior", "minmax", "n_nodes")


def search_inputs(cfg, net, n, seed):
    """n roots: ragged legal sets (a single action at tree 0, the whole action space at tree 1), both players where the game
    has two, noise on; the roots mzx_search_run_from_roots takes come from the network's own initial inference."""
    A, players = len(cfg.action_space), len(cfg.players)
    rs = numpy.random.RandomState(seed)
    obs = numpy.ascontiguousarray(numpy.asarray(synthetic.observations(n, net.input_shape, seed=seed), numpy.float32).reshape(n, -1))
    legal = numpy.full((n, A), -1, numpy.int32)
    count = numpy.zeros(n, numpy.int32)
    for k in range(n):
        count[k] = 1 if k == 0 else (A if k == 1 else 1 + (3 * k + 1) % A)
        legal[k, :count[k]] = numpy.sort(rs.permutation(A)[:count[k]])
    to_play = (numpy.arange(n) % players).astype(numpy.int32)
    noise = numpy.zeros((n, A))
    for k in range(n):
        noise[k, :count[k]] = rs.dirichlet([cfg.root_dirichlet_alpha] * int(count[k]))
    tape = rs.randint(0, 2 ** 32, size=(n, search.TAPE_WORDS), dtype=numpy.uint32)
    _, _, policy, hidden = net.initial_inference(torch.tensor(obs).reshape((n,) + tuple(net.input_shape)))
    logits = policy.cpu().numpy().astype(numpy.float64)
    priors = numpy.zeros((n, A))
    for k in range(n):
        e = numpy.exp(logits[k, legal[k, :count[k]]] - logits[k].max())
        priors[k, :count[k]] = e / e.sum()
    be = net.backend
    dev = lambda a: torch.as_tensor(a).contiguous().to(be.device)
    return dict(n=n, A=A, players=players, count=count, h_obs=obs, h_legal=legal, h_to_play=to_play, obs=dev(obs), legal=dev(legal),
                to_play=dev(to_play), noise=dev(noise), tape=dev(tape.view(numpy.int32)), hidden=hidden.reshape(n, -1).contiguous(),
                priors=dev(priors), reward=dev(numpy.zeros(n)))


class SearchCell:
    """One (network, search mode, carried node capacity) cell: every entry under every pattern against its ZERO run."""

    def __init__(self, backend, cfg, net, mode, carried, label, trees=B, stale_trees=B_STALE):
        self.be, self.lib, self.cfg, self.net, self.label = backend, backend.lib, cfg, net, label
        self.B, self.carried, self.mode = trees, carried, mode
        self.engine = search.BatchedMCTS(cfg, net, max(trees, stale_trees), num_simulations=SIMS, mode=mode, max_carried_nodes=carried)
        self.inp = search_inputs(cfg, net, trees, 3)
        self.stale_inp = search_inputs(cfg, net, stale_trees, 4)
        self.arena_bytes = max(self.lib.mzx_search_arena_bytes(self.engine.handle(n)) for n in (trees, stale_trees))
        self.lines = []

    # -- buffers
    def outputs(self, n):
        A, be = self.inp["A"], self.be
        return dict(visits=sentinel(be.empty((n, A), torch.int32)), root_value=sentinel(be.empty((n,), torch.float64)),
                    predicted=sentinel(be.empty((n,), torch.float64)), info=sentinel(be.empty((n, 4), torch.int32)))

    def io(self, inp, out, to_play=None, noise=None):
        p = self.be.ptr
        return _lib.SearchIO(p(inp["obs"]), p(inp["legal"]), p(inp["to_play"] if to_play is None else to_play),
                             p(inp["noise"] if noise is None else noise), p(inp["tape"]), p(out["visits"]), p(out["root_value"]),
                             p(out["predicted"]), p(out["info"]))

    def _stale(self, arena):
        """A finished search of B_STALE trees (another layout of the same bytes) in ``arena``."""
        inp, out = self.stale_inp, self.outputs(self.stale_inp["n"])
        io = self.io(inp, out)
        self.lib.check(self.lib.mzx_search_run(self.engine.handle(inp["n"]), ctypes.byref(io), self.be.ptr(arena), arena.numel(),
                                               self.be.stream()))
        assert (out["visits"].cpu().numpy().sum(1) == SIMS).all()

    def arena(self, pattern):
        return fill(self.be.empty((self.arena_bytes,), torch.uint8), pattern, self._stale)

    def dump(self, handle, arena):
        be, n, N, A = self.be, self.B, self.engine.num_nodes, self.inp["A"]
        shapes = dict(visit=((n, N), torch.int32), value_sum=((n, N), torch.float64), reward=((n, N), torch.float64),
                      to_play=((n, N), torch.int32), parent=((n, N), torch.int32), child=((n, N, A), torch.int32),
                      prior=((n, N, A), torch.float64), minmax=((n, 2), torch.float64), n_nodes=((n,), torch.int32))
        t = {k: sentinel(be.empty(s, dt)) for k, (s, dt) in shapes.items()}
        d = _lib.TreeDump(*[be.ptr(t[k]) for k in DUMP_FIELDS])
        self.lib.check(self.lib.mzx_search_dump(handle, ctypes.byref(d), be.ptr(arena), be.stream()))
        t = {k: v.cpu().numpy() for k, v in t.items()}
        nn = t["n_nodes"]
        assert ((nn >= 1) & (nn <= N)).all(), nn
        out = {"dump_n_nodes": nn, "dump_minmax": t["minmax"]}
        for k in DUMP_FIELDS[:7]:            # per-node fields: the nodes that exist
            out["dump_" + k] = numpy.concatenate([t[k][i, :nn[i]].reshape(-1) for i in range(n)])
        for k, v in out.items():
            assert not untouched(v).any(), ("sentinel left in the dump", k)
        return out

    # -- entries: each returns (outputs as numpy, kernel name)
    def entry(self, name, pattern):
        be, lib, inp, n = self.be, self.lib, self.inp, self.B
        engine = self.engine
        h = engine.handle(n)
        dumps = self.mode == 0 or self.carried > 0       # routes that leave their trees in the arena
        res = {}
        if name in ("run", "from_roots", "continued", "run_export"):
            if name == "run_export":                     # mode flag 2: the whole-search kernels export their trees
                if getattr(self, "_export", None) is None:
                    self._export = search.BatchedMCTS(self.cfg, self.net, n, num_simulations=SIMS, mode=3)
                h, dumps = self._export.handle(n), True
            arena, out = self.arena(pattern), self.outputs(n)
            io = self.io(inp, out)
            if name == "from_roots":
                lib.check(lib.mzx_search_run_from_roots(h, ctypes.byref(io), be.ptr(inp["hidden"]), be.ptr(inp["priors"]),
                                                        be.ptr(inp["reward"]), be.ptr(arena), arena.numel(), be.stream()))
            else:
                lib.check(lib.mzx_search_run(h, ctypes.byref(io), be.ptr(arena), arena.numel(), be.stream()))
            res = {k: v.cpu().numpy() for k, v in out.items()}
            want = numpy.full(n, SIMS)
            if name == "continued":
                first = res["visits"]
                picks = numpy.array([-1 if i % 2 else int(first[i].argmax()) for i in range(n)], numpy.int32)
                moved = picks >= 0
                to_play = numpy.where(moved & (inp["players"] == 2), 1 - inp["h_to_play"], inp["h_to_play"]).astype(numpy.int32)
                rs = numpy.random.RandomState(11)
                noise = numpy.zeros((n, inp["A"]))
                for i in range(n):
                    c = inp["A"] if moved[i] else int(inp["count"][i])
                    noise[i, :c] = rs.dirichlet([self.cfg.root_dirichlet_alpha] * c)
                dst, out = self.arena(pattern), self.outputs(n)     # the DESTINATION of the carry is poisoned too
                t_act, t_tp, t_noise = (torch.as_tensor(a).to(be.device) for a in (picks, to_play, noise))
                lib.check(lib.mzx_search_advance(h, be.ptr(t_act), be.ptr(arena), be.ptr(dst), be.stream()))
                io = self.io(inp, out, t_tp, t_noise)
                lib.check(lib.mzx_search_run_continued(h, ctypes.byref(io), be.ptr(dst), dst.numel(), be.stream()))
                res = {"first_" + k: v for k, v in res.items()}
                res.update({k: v.cpu().numpy() for k, v in out.items()})
                want = numpy.where(moved, first[numpy.arange(n), numpy.maximum(picks, 0)] - 1, SIMS) + SIMS
                arena = dst
            kernel = lib.mzx_search_kernel_name(h).decode()
        else:                                            # mzx_selfplay_search: the draws of a bank, one library call,
            arena = self.arena(pattern)                  # on this test's own mzx_move (include/mzx.h) and staging blocks
            A, obs_floats, on_gpu = inp["A"], inp["h_obs"].shape[1], be.device.type == "cuda"

            def carve(fields):
                at, table = 0, {}
                for key, dtype, count in fields:
                    table[key] = (at, dtype, count)
                    at += (numpy.dtype(dtype).itemsize * count + 15) & ~15
                return table, at
            fin, n_in = carve([("noise", numpy.float64, n * A), ("obs", numpy.float32, n * obs_floats), ("legal", numpy.int32, n * A),
                               ("to_play", numpy.int32, n), ("tape", numpy.uint32, n * search.TAPE_WORDS)])
            fout, n_out = carve([("root_value", numpy.float64, n), ("predicted", numpy.float64, n), ("visits", numpy.int32, n * A),
                                 ("info", numpy.int32, n * 4)])
            h_in = torch.zeros(n_in, dtype=torch.uint8, pin_memory=on_gpu)
            h_out = torch.zeros(n_out, dtype=torch.uint8, pin_memory=on_gpu)
            d_in = be.empty((n_in,), torch.uint8) if on_gpu else h_in
            d_out = be.empty((n_out,), torch.uint8) if on_gpu else h_out
            torch_of = {numpy.float64: torch.float64, numpy.int32: torch.int32}
            for block in ((d_out, h_out) if on_gpu else (h_out,)):      # the sentinel under every output, device and host copy
                for key, (at, dtype, count) in fout.items():
                    sentinel(block[at:at + numpy.dtype(dtype).itemsize * count].view(torch_of[dtype]))
            bank = _rng.StreamBank(lib, [500 + i for i in range(n)])
            streams, n_legal = numpy.arange(n, dtype=numpy.int32), numpy.full(n, -7, numpy.int32)
            mv = _lib.Move()
            mv.num_games, mv.action_space_size, mv.tape_words, mv.num_threads = n, A, search.TAPE_WORDS, bank.threads
            mv.streams, mv.legal_actions, mv.to_play = streams.ctypes.data, inp["h_legal"].ctypes.data, inp["h_to_play"].ctypes.data
            mv.observation, mv.observation_floats = inp["h_obs"].ctypes.data, obs_floats
            mv.dirichlet_alpha, mv.add_exploration_noise, mv.flags = float(self.cfg.root_dirichlet_alpha), 1, 0
            mv.h_in, mv.d_in, mv.in_bytes = h_in.data_ptr(), d_in.data_ptr(), n_in
            mv.h_out, mv.d_out, mv.out_bytes = h_out.data_ptr(), d_out.data_ptr(), n_out
            pi = lambda key: ctypes.c_void_p(d_in.data_ptr() + fin[key][0])
            po = lambda key: ctypes.c_void_p(d_out.data_ptr() + fout[key][0])
            mv.io = _lib.SearchIO(pi("obs"), pi("legal"), pi("to_play"), pi("noise"), pi("tape"), po("visits"), po("root_value"),
                                  po("predicted"), po("info"))
            lib.check(lib.mzx_selfplay_search(h, bank.handle, ctypes.byref(mv), n_legal.ctypes.data, be.ptr(arena), arena.numel(),
                                              be.stream()))
            assert numpy.array_equal(n_legal, inp["count"]), n_legal
            host = {key: h_out.numpy()[at:at + numpy.dtype(dtype).itemsize * count].view(dtype).copy() for key, (at, dtype, count) in fout.items()}
            res = dict(visits=host["visits"].reshape(n, A), root_value=host["root_value"], predicted=host["predicted"],
                       info=host["info"].reshape(n, 4))
            if on_gpu:                                   # the download brought what the device block holds
                torch.cuda.synchronize()
                assert numpy.array_equal(d_out.cpu().numpy(), h_out.numpy())
            want = numpy.full(n, SIMS)
            kernel = lib.mzx_search_kernel_name(h).decode()
        if be.device.type == "cuda":
            torch.cuda.synchronize()
        for k, v in res.items():
            if k.endswith("predicted") and name == "from_roots":
                continue                                  # "io->d_root_predicted_value not written" (include/mzx.h)
            assert not untouched(v).any(), (self.label, name, pattern, "sentinel left in", k)
        assert (res["info"][:, 1] == 0).all(), (self.label, name, pattern, res["info"])
        assert numpy.array_equal(res["visits"].sum(1), want), (self.label, name, pattern, res["visits"].sum(1), want)
        illegal = numpy.ones_like(res["visits"], bool)
        if name != "continued":                           # "0 if not a child"
            for i in range(n):
                illegal[i, inp["h_legal"][i, :inp["count"][i]]] = False
            assert (res["visits"][illegal] == 0).all(), (self.label, name, pattern, res["visits"])
        if name == "from_roots":
            res.pop("predicted")
        if dumps:
            res.update(self.dump(h, arena))
        return res, kernel

    def check(self, name, expected_kernel=None, patterns=PATTERNS):
        """Entry ``name`` under every pattern: same bits as under ZERO, the kernel the table names."""
        base = None
        for pattern in patterns:
            got, kernel = self.entry(name, pattern)
            if expected_kernel is not None:
                assert kernel == expected_kernel, (self.label, name, pattern, kernel, expected_kernel)
            if base is None:
                assert pattern == ZERO
                base = got
            same_bits(got, base, (self.label, name, pattern))
            self.lines.append(" | ".join(self.label + (name, kernel, pattern, "same")))
        return self.lines


def search_cell(backend, net_of, name, mode, cap, classes, capacities, expected=None, per_op=None):
    """All entries of one route-table cell.  ``expected``: the table's tuple for the cell (None on the serial build, where
    ``per_op`` names the only route)."""
    assert not _device_errors, f"not run: an earlier call failed on the device ({_device_errors[0]})"
    cfg, net = net_of(name)
    carried = capacities[cap]
    label = (name, "default" if mode is None else str(mode), cap)
    with backend.lib.tuning(**classes[name][1]):
        cell = SearchCell(backend, cfg, net, mode, carried, label)
        fresh = expected[0] if expected else per_op
        try:
            cell.check("run", fresh)
            cell.check("selfplay_search", fresh)
            cell.check("from_roots", (expected[2] if carried else expected[1]) if expected else per_op)
            if carried:
                cell.check("continued", expected[1] if expected else per_op)
            elif mode is None and expected and backend.lib.mzx_search_fused_supported(cell.engine.handle(B)) in (1, 2):
                cell.check("run_export", fresh)
        except (RuntimeError, _lib.MzxError) as e:      # a failed launch or a fault: nothing more goes to this device
            _device_errors.append(f"{label}: {e}"[:300])
            raise
        finally:
            for line in cell.lines:
                print("poison:", line)
    return cell.lines


_device_errors = []


def make_net(backend, classes, name, cache={}):
    key = (id(backend), name)
    if key not in cache:
        cfg = classes[name][0]()
        net = models.MuZeroNetwork(cfg, _backend=backend)
        net.set_weights(synthetic.fill_state_dict(net.state_dict(), 5))
        if classes[name][2] is not None:
            net.set_mode(classes[name][2])
        cache[key] = (cfg, net)
    return cache[key]


# ------------------------------------------------------------------------------------------ trainers and the loss head

def _sync(be):
    if be.device.type == "cuda":
        torch.cuda.synchronize()


def _prefix_of(other):
    """STALE for a scratch block: the words another case's call left, laid over the start of this one."""
    def stale(t):
        n = min(t.numel(), other.numel())
        t.reshape(-1)[:n].copy_(other.reshape(-1)[:n])
    return stale


def all_cases(tables):
    """The fixture cases of a table and the ones it holds live to a restatement."""
    return list(tables.CASES) + list(getattr(tables, "LIVE_CASES", ()))


TRAIN_OUTPUTS = ("grad", "losses", "priorities", "value_logits", "reward_logits", "policy_logits", "stats")


def train_step(be, tables, kind, case, pattern, other_scratch):
    """One mzx_train_{fc,resnet}_step through the raw ABI: scratch under ``pattern``, every output under the sentinel ->
    (outputs as host arrays, the scratch the step left)."""
    import train_cases_common as common
    net, keep = tables.network(be, case), []

    def filler(name, t):
        if name == "scratch":
            fill(t, pattern, None if other_scratch is None else _prefix_of(other_scratch))
        else:
            sentinel(t)
    io, t = common.step_io(be, case, net, keep, kind, be.device, fill=filler, whole=True)
    be.lib.check(getattr(be.lib, f"mzx_train_{kind}_step")(net.handle, ctypes.byref(io), be.stream()))
    _sync(be)
    out = {k: t[k].cpu().numpy() for k in TRAIN_OUTPUTS if k in t}
    for k, v in out.items():
        assert not untouched(v).any(), (case["name"], pattern, "sentinel left in", k, int(untouched(v).sum()))
    return out, t["scratch"]


def train_case(be, tables, kind, case, pinned=None, family=None):
    """One case of a trainer table under every pattern; STALE is the scratch the step of the case before it in the table
    left.  ``pinned``: the serial section of the family's bit fixture, which the ZERO run (and so every run) has to reproduce."""
    import train_cases_common as common
    cases = all_cases(tables)
    before = cases[[c["name"] for c in cases].index(case["name"]) - 1]
    _, previous = train_step(be, tables, kind, before, ZERO, None)
    base, _ = train_step(be, tables, kind, case, ZERO, None)
    if pinned is not None and case["name"] in pinned["cases"]:
        named = dict(loss=base["losses"][0], value_loss=base["losses"][1], reward_loss=base["losses"][2],
                     policy_loss=base["losses"][3], grad_flat=base["grad"], running=base.get("stats"), **base)
        have, want = common.bits.digests(named, family), pinned["cases"][case["name"]]
        differs = [k for k in want if have[k] != want[k]]
        assert not differs, (case["name"], "the raw step under ZERO differs from the pinned bits", differs)
    lines = []
    for pattern in PATTERNS[1:]:
        got, _ = train_step(be, tables, kind, case, pattern, previous)
        same_bits(got, base, (case["name"], pattern))
        lines.append(f"{kind} | {case['name']} | {pattern} | same")
    return lines


def loss_call(be, case, x, pattern, other_scratch):
    """mzx_trainer_loss through the raw ABI -> (outputs, the scratch it left)."""
    up = lambda a: None if a is None else torch.from_numpy(numpy.ascontiguousarray(a)).to(be.device)
    t = {k: up(v) for k, v in x.items()}
    B, steps = case["B"], case["steps"]
    out = dict(packed=sentinel(be.empty((4 + B * steps,), torch.float32)), grad_value=sentinel(torch.empty_like(t["value"])),
               grad_reward=sentinel(torch.empty_like(t["reward"])), grad_policy=sentinel(torch.empty_like(t["policy"])))
    nbytes = int(be.lib.mzx_trainer_loss_scratch_bytes(B, steps))
    scratch = fill(be.empty((max(nbytes // 4, 1),), torch.float32), pattern, None if other_scratch is None else _prefix_of(other_scratch))
    io = _lib.TrainerLossIO()
    io.d_value_logits, io.d_reward_logits, io.d_policy_logits = t["value"].data_ptr(), t["reward"].data_ptr(), t["policy"].data_ptr()
    io.d_target_value, io.d_target_reward, io.d_target_policy = (t[k].data_ptr() for k in ("target_value", "target_reward", "target_policy"))
    io.d_gradient_scale = t["gradient_scale"].data_ptr()
    io.d_weight = None if t["weight"] is None else t["weight"].data_ptr()
    io.batch, io.steps, io.support_size, io.num_actions = B, steps, case["S"], case["A"]
    io.value_loss_weight, io.per_alpha = float(case["vlw"]), float(case["alpha"])
    io.d_losses, io.d_priorities = out["packed"].data_ptr(), out["packed"][4:].data_ptr()
    io.d_grad_value, io.d_grad_reward, io.d_grad_policy = (out[k].data_ptr() for k in ("grad_value", "grad_reward", "grad_policy"))
    io.d_scratch, io.scratch_bytes = scratch.data_ptr(), nbytes
    be.lib.check(be.lib.mzx_trainer_loss(ctypes.byref(io), be.stream()))
    _sync(be)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in host.items():
        assert not untouched(v).any(), (case["name"], pattern, "sentinel left in", k)
    return host, scratch


def loss_table(be, tables):
    cases = all_cases(tables)
    _, previous = loss_call(be, cases[-1], tables.inputs(cases[-1]), ZERO, None)
    lines = []
    for case in cases:
        x = tables.inputs(case)
        base, left = loss_call(be, case, x, ZERO, None)
        for pattern in PATTERNS[1:]:
            got, _ = loss_call(be, case, x, pattern, previous)
            same_bits(got, base, (case["name"], pattern))
            lines.append(f"loss | {case['name']} | {pattern} | same")
        previous = left
    return lines


# ------------------------------------------------------------------------------------------------------ network buffers

NET_MODES = (None, 0, 3)             # the handle's default engine, one kernel per operator, everything on the streamed engine
NET_BATCHES = (1, 5, 37)


class NetCase:
    """One network through the raw ABI: d_derived poisoned before mzx_net_set_weights, d_workspace before each inference,
    d_scratch and d_workspace of mzx_net_debug_prefix; every output under the sentinel."""

    def __init__(self, be, cfg, seed=31):
        self.be, self.lib, self.cfg = be, be.lib, cfg
        self.net = net = models.MuZeroNetwork(cfg, _backend=be)
        net.set_weights(synthetic.fill_state_dict(net.state_dict(), seed))
        self.flat = net.flat_weights()
        other = models.MuZeroNetwork(cfg, _backend=be)          # STALE: the derived image of other weights
        other.set_weights(synthetic.fill_state_dict(other.state_dict(), seed + 1))
        self.other_flat = other.flat_weights().clone()
        self.A, self.W = len(cfg.action_space), 2 * cfg.support_size + 1
        rs = numpy.random.RandomState(5)
        n = max(NET_BATCHES) + 2
        dev = lambda a: torch.as_tensor(a).contiguous().to(be.device)
        self.obs = dev(rs.rand(n, net.input_size).astype(numpy.float32))
        self.hid = dev(rs.rand(n, net.hidden_size).astype(numpy.float32))
        self.act = dev(rs.randint(0, self.A, size=n).astype(numpy.int32))

    def bind(self, pattern):
        """mzx_net_set_weights into a poisoned d_derived."""
        be, lib, h = self.be, self.lib, self.net.handle
        n = int(lib.mzx_net_derived_floats(h))

        def stale(t):
            lib.check(lib.mzx_net_set_weights(h, be.ptr(self.other_flat), self.other_flat.numel(), be.ptr(t), t.numel(), be.stream()))
            _sync(be)
        self.derived = fill(be.empty((max(n, 1),), torch.float32), pattern, stale)
        lib.check(lib.mzx_net_set_weights(h, be.ptr(self.flat), self.flat.numel(), be.ptr(self.derived), n, be.stream()))

    def outputs(self, n):
        be = self.be
        return dict(value=sentinel(be.empty((n, self.W), torch.float32)), reward=sentinel(be.empty((n, self.W), torch.float32)),
                    policy=sentinel(be.empty((n, self.A), torch.float32)), hidden=sentinel(be.empty((n, self.net.hidden_size), torch.float32)))

    def _call(self, recurrent, n, out, ws):
        be, lib, h = self.be, self.lib, self.net.handle
        o = [be.ptr(out[k]) for k in ("value", "reward", "policy", "hidden")]
        if recurrent:
            lib.check(lib.mzx_net_recurrent_inference(h, be.ptr(self.hid), be.ptr(self.act), n, *o, be.ptr(ws), ws.numel(), be.stream()))
        else:
            lib.check(lib.mzx_net_initial_inference(h, be.ptr(self.obs), n, *o, be.ptr(ws), ws.numel(), be.stream()))

    def workspace(self, n, pattern):
        """d_workspace for a batch of n; STALE: what both inferences of n + 2 samples left in it."""
        be, lib, h = self.be, self.lib, self.net.handle
        floats = max(int(lib.mzx_net_workspace_floats(h, n)), int(lib.mzx_net_workspace_floats(h, n + 2)), 1)

        def stale(t):
            for recurrent in (0, 1):
                self._call(recurrent, n + 2, self.outputs(n + 2), t)
            _sync(be)
        return fill(be.empty((floats,), torch.float32), pattern, stale)

    def run(self, pattern, prefix):
        """-> {(what, batch, output): host array} of both inferences at every batch (and the prefixes in ``prefix``)."""
        be, lib, h, net = self.be, self.lib, self.net.handle, self.net
        self.bind(pattern)
        got = {}
        for n in NET_BATCHES:
            for recurrent in (0, 1):
                out, ws = self.outputs(n), self.workspace(n, pattern)
                self._call(recurrent, n, out, ws)
                _sync(be)
                for k, v in out.items():
                    got[("recurrent" if recurrent else "initial", n, k)] = v.cpu().numpy()
        n = NET_BATCHES[1]
        for recurrent, fused, n_ops in prefix:
            per = int(lib.mzx_net_operator_out_floats(h, recurrent, n_ops - 1))
            out = sentinel(be.empty((n * per,), torch.float32))
            scratch = fill(be.empty(((net.hidden_size + 2 * self.W + self.A) * n,), torch.float32), pattern, _prefix_of(self.derived))
            ws = self.workspace(n, pattern)
            rc = lib.mzx_net_debug_prefix(h, recurrent, fused, n_ops, be.ptr(self.hid if recurrent else self.obs),
                                          be.ptr(self.act) if recurrent else None, n, be.ptr(out), out.numel(), be.ptr(scratch),
                                          scratch.numel(), be.ptr(ws), ws.numel(), be.stream())
            if rc == -1 and fused:         # MZX_ERR_INVALID: the tuned engine does not cover this operator -- under every pattern
                got[("prefix", recurrent, fused, n_ops)] = numpy.array([rc])
                continue
            lib.check(rc)
            _sync(be)
            got[("prefix", recurrent, fused, n_ops)] = out.cpu().numpy()
        for k, v in got.items():
            assert not untouched(v).any(), (pattern, "sentinel left in", k, int(untouched(v).sum()))
        return got

    def prefixes(self, fused):
        """The whole program and a prefix that ends in its middle, on the per-operator engine and (``fused``) the tuned one."""
        out = []
        for recurrent in (0, 1):
            ops = self.net.num_operators(recurrent)
            for n_ops in sorted({max(1, ops // 2), ops}):
                if self.lib.mzx_net_operator_out_floats(self.net.handle, recurrent, n_ops - 1) > 0:
                    out += [(recurrent, f, n_ops) for f in ((0, 1) if fused else (0,))]
        return out


def net_case(be, name, cfg, tunings=({},)):
    """Every mode the handle accepts x the tuning entries: each pattern against ZERO, bit for bit."""
    case = NetCase(be, cfg)
    lines = []
    # what the handle has to accept: one kernel per operator always; the streamed engine for every residual network here and
    # for no fully connected one (the serial build plans it as well: there the mode changes no arithmetic)
    accepts = {None: True, 0: True, 3: cfg.network == "resnet"}
    for mode in NET_MODES:
        accepted = mode is None or be.lib.mzx_net_set_mode(case.net.handle, mode) == 0
        assert accepted == accepts[mode], (name, mode, "accepted" if accepted else be.lib.mzx_last_error())
        if not accepted:
            continue
        tuned = mode != 0 and cfg.network == "resnet" and be.device.type == "cuda"
        for tuning in (tunings if tuned else ({},)):
            with be.lib.tuning(**tuning):
                prefix = case.prefixes(tuned)
                base = None
                for pattern in PATTERNS:
                    got = case.run(pattern, prefix)
                    if base is None:
                        base = got
                    assert sorted(got) == sorted(base)
                    same_bits(got, base, (name, mode, tuning, pattern))
                    lines.append(f"net | {name} | mode {'default' if mode is None else mode} | {tuning} | {pattern} | same")
    return lines


# ------------------------------------------------------------------------------------------- the sampler's workspace

def sampler_case(be, cases, slots, per):
    """mzx_replay_sample on the dyadic store of replay_sampler_cases: d_tile_prefix and d_raw under every pattern (STALE: what
    a draw of another batch size and counter left), every output under the sentinel.  d_owner is state, not scratch ("-1
    everywhere between calls"): left alone."""
    cfg, store, _ = cases.dyadic_store(be, slots, per)
    table = cases.table_of(store)
    total = int(table["len"][table["game"] >= 0].sum())
    U = cfg.num_unroll_steps
    store.sample(1, cfg.seed, 1, total, per, U)                 # (uploads pending slot columns, builds the sampler struct)
    lines = []
    for n in cases.BATCHES:
        def draw(pattern, n=n, counter=3):
            sampler = type(store.sampler).from_buffer_copy(store.sampler)
            prefix = be.empty((store._tile_prefix.numel(),), torch.float64)
            raw = be.empty((max(n, cases.BATCHES[-1]),), torch.float64)
            sampler.d_tile_prefix, sampler.d_raw, sampler.raw_capacity = prefix.data_ptr(), raw.data_ptr(), raw.numel()
            out = dict(base=sentinel(be.empty((n,), torch.int64)), len=sentinel(be.empty((n,), torch.int32)),
                       pos=sentinel(be.empty((n,), torch.int32)), tape=sentinel(be.empty((n, U + 1), torch.int32)),
                       game_id=sentinel(be.empty((n,), torch.int64)))
            if per:
                out["weight"] = sentinel(be.empty((n,), torch.float32))

            def call(count, call_counter):
                io = _lib.ReplaySampleIO()
                io.seed, io.call_counter, io.total_samples, io.num_samples = cfg.seed, call_counter, total, count
                io.per, io.num_unroll_steps, io.num_actions = int(per), U, store.A
                io.d_action_space = None if store._action_space is None else store._action_space.data_ptr()
                io.d_base, io.d_len, io.d_pos, io.d_absorbing_actions = (out[k].data_ptr() for k in ("base", "len", "pos", "tape"))
                io.d_game_id = out["game_id"].data_ptr()
                io.d_weight = out["weight"].data_ptr() if per else None
                be.lib.check(be.lib.mzx_replay_sample(ctypes.byref(sampler), ctypes.byref(io), be.stream()))
                _sync(be)

            def stale(_):
                if n > 1:
                    call(n - 1, counter + 9)
                else:
                    call(1, counter + 9)
                for v in out.values():
                    sentinel(v)
            fill(prefix, ZERO if pattern == STALE else pattern)
            fill(raw, pattern, stale)
            call(n, counter)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for k, v in got.items():
                assert not untouched(v).any(), (slots, per, n, pattern, "sentinel left in", k)
            return got
        base = draw(ZERO)
        for pattern in PATTERNS[1:]:
            same_bits(draw(pattern), base, (slots, per, n, pattern))
            lines.append(f"sampler | slots {slots} per {int(per)} n {n} | {pattern} | same")
    return lines


# ------------------------------------------------------------------------------- the arenas of mzx_selfplay_rounds

class _PoisonedArenas:
    """While active, every arena a BatchedMCTS allocates (``BatchedMCTS.arena``, what native_rounds hands the actor as
    ``d_arena``) is filled with the pattern instead of zeros; ``taken`` keeps the arenas, for the STALE run of another shard."""

    def __init__(self, pattern, left=()):
        self.pattern, self.left, self.taken = pattern, list(left), []

    def __enter__(self):
        original = self.original = search.BatchedMCTS.arena
        scope = self

        def arena(engine, num_trees):
            before = engine._arena
            tensor = original(engine, num_trees)
            if tensor is not before:
                other = scope.left[len(scope.taken) % len(scope.left)] if scope.left else None
                fill(tensor, scope.pattern, None if other is None else _prefix_of(other))
                scope.taken.append(tensor)
            return tensor
        search.BatchedMCTS.arena = arena
        return self

    def __exit__(self, *exc):
        search.BatchedMCTS.arena = self.original
        return False


def rounds_case(be, rounds, Game, cfg, trees, seed, calls, weights=None):
    """Resident rounds (tests/resident_rounds_cases.py ``run``) with the groups' arenas under every pattern: the games, the
    draw counter, the statistics and the final positions of the run on zeroed arenas.  STALE: the arenas a run of
    ``trees + 2`` games (other group sizes, another layout) left."""
    weights = rounds._weights(be, cfg) if weights is None else weights
    with _PoisonedArenas(ZERO) as scope:
        rounds.run(be, Game, cfg, weights, trees + 2, seed, calls, True)
    left = scope.taken
    assert left
    base, lines = None, []
    for pattern in PATTERNS:
        with _PoisonedArenas(pattern, left if pattern == STALE else ()) as scope:
            got = rounds.run(be, Game, cfg, weights, trees, seed, calls, True)
        assert scope.taken, "no arena was allocated under the pattern"
        if base is None:
            base = got
        rounds.assert_same(got, base)
        assert got["stats"]["searches"] == base["stats"]["searches"] and got["resident"][0] == base["resident"][0]
        lines.append(f"rounds | {Game.__name__} {trees} games | {pattern} | same")
    return lines
