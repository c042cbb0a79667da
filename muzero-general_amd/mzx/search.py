"""
The batched search behind the C ABI (split out of mzx/self_play.py in round 6; ``mzx.self_play`` re-exports every name).

``BatchedMCTS`` searches B roots per call -- MCTS.run (/root/reference/self_play.py:260-361) for a shard of games: staging
of a move's inputs and outputs, root noise / tie-break tape from the per-game streams, the library call, tape retries,
the searched trees as reference ``Node`` graphs (``node_graph``), roots the caller expanded itself (``run_from_roots``:
override_root_with, :275-277).  ``MCTS`` is the reference's single-root class on top of it (same signature and return value).
"""
import ctypes
import math
import types

import numpy
import torch

from . import _lib, draws
from .history import Node

# raw MT19937 words per tree handed to a search for its tie draws: a search normally consumes ONE (the all-zero
# scores of its first walk); a tree that needs more is searched again with a longer tape (BatchedMCTS.run)
TAPE_WORDS = 16


class SearchResult:
    """Per-root outputs of one batched search (host numpy arrays)."""

    def __init__(self, visit_counts, root_values, root_predicted_values, info, legal_actions):
        self.visit_counts = visit_counts                  # [B][A] int32, by action
        self.root_values = root_values                    # [B] float64, root.value()
        self.root_predicted_values = root_predicted_values  # [B] float64
        self.max_tree_depth = info[:, 0]
        self.flags = info[:, 1]
        self.tape_used = info[:, 2]
        self.sum_depth = info[:, 3]
        self.legal_actions = legal_actions
        self.shared_legal = None     # set when every root has the same legal-action list (list protocol)
        self.legal_array = self.n_legal = self.streams = None    # bank searches: [B][A] padded lists, their lengths, the streams
        self.pending_words = None    # tie-break words the streams have still to consume (run(..., _defer_advance=True))

    def root(self, i):
        """A ``Node`` whose children carry the visit counts of root i (self_play.py:222-245, :496-511)."""
        node = Node(0)
        total = int(self.visit_counts[i].sum())
        node.visit_count = total
        node.value_sum = float(self.root_values[i]) * total
        for a in self.legal_actions[i]:
            child = Node(0)
            child.visit_count = int(self.visit_counts[i][a])
            node.children[a] = child
        node._root_value = float(self.root_values[i])
        node.value = lambda: node._root_value if total else 0
        return node



class PendingSearch:
    """A search that may still be running on the device (``BatchedMCTS.run(..., _asynchronous=True)``)."""

    def __init__(self, complete):
        self._complete, self._result = complete, None

    def result(self):
        if self._complete is not None:
            self._result, self._complete = self._complete(), None
        return self._result


class _MoveOutputs:
    """
    The outputs of a one-call move (``BatchedMCTS._fused_move``).  Calling it waits for the event behind an asynchronous
    call and hands out host copies of visits, root values, predicted values and info, n_legal [B] and the noise the roots
    got ([B][A] view of the staging block, or None: no noise, or device draws -- ``device_noise`` is then the tensor).
    ``select`` (device draws with a temperature): the call also fills ``actions``.  (An object, not a closure with
    attributes: a function that names itself is a reference cycle per search, left to the cyclic collector.)
    """
    select, actions, device_noise = False, None, None

    def __init__(self, staging, shape, n_legal, done, host_noise, keep):
        self.staging, self.shape, self.n_legal, self.done, self.host_noise, self.keep = staging, shape, n_legal, done, host_noise, keep

    def __call__(self):
        if self.done is not None:
            self.done.synchronize()
        st, (B, A) = self.staging, self.shape
        vout = st["vout"]
        if self.select:
            self.actions = vout["action"].copy()
        return (vout["visits"].reshape(B, A).copy(), vout["root_value"].copy(), vout["predicted"].copy(),
                vout["info"].reshape(B, 4).copy(), self.n_legal, st["vin"]["noise"].reshape(B, A) if self.host_noise else None)


def _validate(config):
    A = len(config.action_space)
    if list(config.action_space) != list(range(A)):
        raise NotImplementedError("config.action_space must be list(range(n)) (the game files only edit its length)")
    P = len(config.players)
    if list(config.players) != list(range(P)):
        raise NotImplementedError("config.players must be list(range(n))")
    if P > 2:
        raise NotImplementedError("More than two player mode not implemented.")  # self_play.py:429-430


class BatchedMCTS:
    """
    MCTS.run (self_play.py:260-361) for B roots at once.  One instance owns the
    device arena for up to ``max_trees`` roots of a given network.
    """

    fused_move = True     # A/B switch of the tests: False = the separate calls (root_draws, _launch, advance, numpy select)

    def __init__(self, config, model, max_trees, num_simulations=None, mode=None, max_carried_nodes=0, device_draws=None):
        _validate(config)
        # device draws (csrc/mzx_draws.h): noise, tape and action choice as a function of (draw_seed, stream, counter); a
        # call with rngs=None takes them, streams default to the tree numbers and the counter to draw_counter (then + 1)
        self.device_draws = bool(getattr(config, "device_draws", False)) if device_draws is None else bool(device_draws)
        # (draw_seed: config.seed for an engine on its own; SelfPlay sets its actor's seed, so that actors sharing a
        # configuration draw apart -- csrc/mzx_draws.h)
        self.draw_seed = int(getattr(config, "seed", 0))
        self.draw_counter = 0
        self.tape_retries = 0      # trees searched again on a longer tape so far (diagnostics, tests)
        self.config = config
        self.model = model
        self.backend = model.backend
        self.max_trees = int(max_trees)
        self.num_simulations = int(config.num_simulations if num_simulations is None else num_simulations)
        self.A = len(config.action_space)
        n = self.num_simulations + 1
        # host tables with Python's own math (the reference's exact values, self_play.py:384-391)
        self._pbc = (ctypes.c_double * n)(
            *[math.log((k + config.pb_c_base + 1) / config.pb_c_base) + config.pb_c_init for k in range(n)]
        )
        self._sqrt = (ctypes.c_double * n)(*[math.sqrt(k) for k in range(n)])
        self._handles = {}
        self._arena = None
        self._mode = mode
        self._buffers = {}
        # continued searches (continue_search / run_from_trees): node slots per tree = num_simulations + 1 + carried nodes
        self.max_carried_nodes = int(max_carried_nodes)
        if self.max_carried_nodes < 0:
            raise ValueError("max_carried_nodes must be >= 0")
        self.num_nodes = n + self.max_carried_nodes
        if self.max_carried_nodes:
            m = self.num_nodes
            self._cap_pbc = (ctypes.c_double * m)(
                *[math.log((k + config.pb_c_base + 1) / config.pb_c_base) + config.pb_c_init for k in range(m)]
            )
            self._cap_sqrt = (ctypes.c_double * m)(*[math.sqrt(k) for k in range(m)])
        self._arena_alt = None     # the second arena of continue_search (the carried trees are copied across)
        self._carry = None         # what the last search of the max_trees-independent handle left: see _note_searched

    def __del__(self):
        try:
            for h in self._handles.values():
                self.backend.lib.mzx_search_destroy(h)
            self._handles = {}
        except Exception:
            pass

    def handle(self, num_trees, tape_words=None):
        if tape_words is None:      # (read at call time: a caller that set TAPE_WORDS gets the handle its searches ran on)
            tape_words = TAPE_WORDS
        key = num_trees if tape_words == TAPE_WORDS else (num_trees, tape_words)
        if key not in self._handles:
            lib = self.backend.lib
            c = _lib.SearchConfig()
            c.num_trees = num_trees
            c.num_simulations = self.num_simulations
            c.action_space_size = self.A
            c.num_players = len(self.config.players)
            c.support_size = self.config.support_size
            c.tape_words = tape_words
            c.discount = float(self.config.discount)
            c.root_exploration_fraction = float(self.config.root_exploration_fraction)
            c.h_pb_c_table = ctypes.cast(self._pbc, ctypes.POINTER(ctypes.c_double))
            c.h_sqrt_table = ctypes.cast(self._sqrt, ctypes.POINTER(ctypes.c_double))
            h = ctypes.c_void_p()
            net = self.model.handle if self.model is not None else None
            lib.check(lib.mzx_search_create(ctypes.byref(c), net, ctypes.byref(h)))
            if self._mode is not None:
                lib.check(lib.mzx_search_set_mode(h, int(self._mode)))
            if self.max_carried_nodes:
                lib.check(lib.mzx_search_set_capacity(h, self.num_nodes, self._cap_pbc, self._cap_sqrt))
            self._handles[key] = h
        return self._handles[key]

    def kernel_name(self, num_trees):
        """The search kernel the last ``run`` of this shard size launched (``mzx_search_kernel_name``)."""
        name = self.backend.lib.mzx_search_kernel_name(self.handle(num_trees))
        return name.decode() if name else ""

    def arena(self, num_trees):
        need = self.backend.lib.mzx_search_arena_bytes(self.handle(num_trees))
        if self._arena is None or self._arena.numel() < need:
            big = self.backend.lib.mzx_search_arena_bytes(self.handle(self.max_trees)) if num_trees <= self.max_trees else need
            self._arena = self.backend.zeros((max(need, big),), torch.uint8)
        return self._arena

    def export_trees(self, num_trees):
        """
        Canonical-order copy of the trees of the last ``run`` (diagnose tooling / parity tests):
        dict of numpy arrays visit [B][N], value_sum, reward, to_play, parent, child [B][N][A],
        prior, minmax [B][2], n_nodes [B].  With the fused kernel this needs mode flag 2 (or max_carried_nodes > 0: such
        an engine's searches always leave their trees in the arena).
        """
        be, lib, B, N, A = self.backend, self.backend.lib, num_trees, self.num_nodes, self.A
        t = dict(
            visit=be.zeros((B, N), torch.int32), value_sum=be.zeros((B, N), torch.float64),
            reward=be.zeros((B, N), torch.float64), to_play=be.zeros((B, N), torch.int32),
            parent=be.zeros((B, N), torch.int32), child=be.zeros((B, N, A), torch.int32),
            prior=be.zeros((B, N, A), torch.float64), minmax=be.zeros((B, 2), torch.float64),
            n_nodes=be.zeros((B,), torch.int32),
        )
        d = _lib.TreeDump(*[be.ptr(t[k]) for k in ("visit", "value_sum", "reward", "to_play", "parent", "child",
                                                   "prior", "minmax", "n_nodes")])
        lib.check(lib.mzx_search_dump(self.handle(B), ctypes.byref(d), be.ptr(self.arena(B)), be.stream()))
        return {k: v.cpu().numpy() for k, v in t.items()}

    def arena_offsets(self, num_trees):
        out = (ctypes.c_int64 * 8)()
        self.backend.lib.check(self.backend.lib.mzx_search_arena_offsets(self.handle(num_trees), ctypes.byref(out)))
        return dict(zip(("tables", "trees", "hidden", "workspace", "tree_bytes", "workspace_bytes", "total"), out))

    def _buf(self, name, shape, dtype):
        key = (name, tuple(shape), dtype)
        if key not in self._buffers:
            self._buffers[key] = self.backend.empty(shape, dtype)
        return self._buffers[key]

    def make_io(self, B, observations, legal, to_play, noise, tape):
        """Upload one move's inputs; returns (io struct, output tensors)."""
        be = self.backend
        dev = lambda a, dt: torch.as_tensor(a).to(dt).contiguous().to(be.device, non_blocking=True)
        t_obs = dev(observations, torch.float32)
        t_legal = dev(legal, torch.int32)
        t_tp = dev(to_play, torch.int32)
        t_noise = None if noise is None else dev(noise, torch.float64)
        t_tape = dev(tape.view(numpy.int32) if isinstance(tape, numpy.ndarray) else tape, torch.int32)
        out = dict(
            visits=self._buf("visits", (B, self.A), torch.int32), root_value=self._buf("rv", (B,), torch.float64),
            predicted=self._buf("rpv", (B,), torch.float64), info=self._buf("info", (B, 4), torch.int32),
        )
        io = _lib.SearchIO(be.ptr(t_obs), be.ptr(t_legal), be.ptr(t_tp), be.ptr(t_noise), be.ptr(t_tape),
                           be.ptr(out["visits"]), be.ptr(out["root_value"]), be.ptr(out["predicted"]),
                           be.ptr(out["info"]))
        keep = (t_obs, t_legal, t_tp, t_noise, t_tape)
        return io, out, keep

    def run_from_roots(self, roots, to_play, add_exploration_noise, rngs=None, streams=None, counter=None):
        """
        MCTS.run(..., override_root_with=root) (self_play.py:275-277) for B roots the caller expanded itself
        (``Node.expand`` after a ``recurrent_inference``, diagnose_model.py:57-74): the roots' hidden states,
        child priors and rewards replace initial_inference.  Roots that already carry visits are not supported.
        """
        legal, priors, rewards, hidden = [], numpy.zeros((len(roots), self.A), numpy.float64), [], []
        for i, root in enumerate(roots):
            if not root.expanded() or root.hidden_state is None:
                raise ValueError("override_root_with must be an expanded Node with a hidden_state")
            if root.visit_count or any(c.visit_count or c.expanded() for c in root.children.values()):
                raise NotImplementedError("override_root_with: only freshly expanded roots (no visits yet) are supported")
            if root.to_play != to_play[i]:
                raise NotImplementedError("override_root_with: root.to_play must equal the to_play argument")
            acts = list(root.children.keys())
            legal.append(acts)
            priors[i, : len(acts)] = [root.children[a].prior for a in acts]
            rewards.append(float(root.reward))
            hidden.append(root.hidden_state.detach().reshape(1, -1))
        override = dict(
            hidden=torch.cat(hidden).to(self.backend.device, torch.float32).contiguous(),
            priors=torch.as_tensor(priors).to(self.backend.device),
            reward=torch.as_tensor(numpy.asarray(rewards, numpy.float64)).to(self.backend.device),
        )
        if override["hidden"].shape[1] != self.model.hidden_size:
            raise ValueError("override_root_with: hidden_state does not match the network's encoded state")
        return self.run(None, legal, to_play, add_exploration_noise, rngs, _override=override, streams=streams, counter=counter)

    def node_graph(self, num_trees, i, root_actions, _trees=None):
        """
        Tree i of the last ``run`` as reference ``Node`` objects (self_play.py:433-476): children dicts keyed
        by action, visit_count / value_sum / prior / reward / to_play / hidden_state ([1, *hidden_shape]
        device tensor) per node -- what diagnose_model.py:145-192 walks.  Needs the per-operator engine
        (mode 0), whose arena holds every node's hidden state in canonical order.
        """
        t = self.export_trees(num_trees) if _trees is None else _trees     # (_trees: one export for many trees)
        off = self.arena_offsets(num_trees)
        N, A, Hf = self.num_nodes, self.A, self.model.hidden_size
        hid = self.arena(num_trees)[off["hidden"]: off["hidden"] + num_trees * N * Hf * 4].view(torch.float32)
        hid = hid.view(num_trees, N, Hf)[i].clone()
        n_nodes = int(t["n_nodes"][i])
        nodes = [None] * n_nodes

        def build(n, prior):
            node = Node(prior)
            node.canonical_index = n       # creation order (run_from_trees keeps it when the graph comes back)
            node.visit_count = int(t["visit"][i, n])
            node.value_sum = float(t["value_sum"][i, n])
            node.to_play = int(t["to_play"][i, n])
            node.reward = float(t["reward"][i, n])
            node.hidden_state = hid[n].view((1,) + tuple(self.model.hidden_shape))
            nodes[n] = node
            return node

        root = build(0, 0)
        order = [0]
        while order:
            n = order.pop()
            actions = list(root_actions) if n == 0 else list(self.config.action_space)
            for slot, a in enumerate(actions):
                c = int(t["child"][i, n, slot])
                prior = float(t["prior"][i, n, slot])
                if c >= 0:
                    nodes[n].children[a] = build(c, prior)
                    order.append(c)
                else:
                    nodes[n].children[a] = Node(prior)
        return root

    # ---- continued searches: MCTS.run(..., override_root_with=node) on nodes that already carry visits and descendants
    def _note_searched(self, B, root_actions, visits):
        """The trees of the last search of handle(B) are in the arena, complete: a continue_search may start from them."""
        self._carry = dict(B=B, root_actions=[list(a) for a in root_actions], visits=numpy.array(visits, copy=True))

    def arena_used_externally(self):
        """A caller ran ``mzx_search_run`` on ``handle`` / ``arena`` itself (``DeviceGameStore.reanalyse_search``): the trees
        of this engine's last ``run`` are gone, so a ``continue_search`` must not start from them."""
        self._carry = None

    def _require_capacity(self):
        if not self.max_carried_nodes:
            raise ValueError("continued searches need BatchedMCTS(..., max_carried_nodes=...) > 0")

    def _draw_ids(self, B, rngs, streams, counter):
        """(streams [B] int32, counter) of a call that draws on the device; None for a call on host streams."""
        if rngs is not None:
            if streams is not None or counter is not None:
                raise ValueError("streams= / counter= belong to device draws (rngs=None)")
            return None
        if not self.device_draws:
            raise ValueError("rngs=None needs device draws: config.device_draws or BatchedMCTS(..., device_draws=True)")
        if self.A > draws.MAX_ACTIONS:
            raise NotImplementedError(f"device draws take at most {draws.MAX_ACTIONS} actions")
        streams = numpy.arange(B, dtype=numpy.int32) if streams is None else numpy.ascontiguousarray(streams, dtype=numpy.int32)
        if streams.shape != (B,):
            raise ValueError("streams: one entry per tree")
        if counter is None:
            counter, self.draw_counter = self.draw_counter, self.draw_counter + 1
        return streams, int(counter)

    def _root_draws(self, root_n, add_exploration_noise, rngs, ids=None):
        """Dirichlet noise over the root's children, then the tie-break tape, from each tree's stream (as ``run``); with
        ``ids`` one library call (``mzx_selfplay_draws``) whose arrays stay on the device."""
        B, A, alpha = len(root_n), self.A, self.config.root_dirichlet_alpha
        if ids is not None:
            noise, tape = draws.root_draws(self.backend, self.draw_seed, ids[1], B, A, TAPE_WORDS, alpha=alpha,
                                           n=numpy.asarray(root_n, numpy.int32), streams=ids[0], noise=bool(add_exploration_noise))
            return noise, tape, None
        assert len(rngs) == B
        noise = numpy.zeros((B, A), numpy.float64) if add_exploration_noise else None
        tape = numpy.zeros((B, TAPE_WORDS), numpy.uint32)
        states = []
        for i in range(B):
            if add_exploration_noise:
                noise[i, : root_n[i]] = rngs[i].dirichlet([alpha] * int(root_n[i]))
            states.append(rngs[i].get_state())
            tape[i] = rngs[i].randint(0, 2 ** 32, size=TAPE_WORDS, dtype=numpy.uint32)
        return noise, tape, states

    def _run_continued(self, B, root_actions, to_play, noise, tape, states, rngs):
        """mzx_search_run_continued on the carried trees of the arena; the result record of ``run``."""
        be, lib, A = self.backend, self.backend.lib, self.A
        dev = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.as_tensor(numpy.ascontiguousarray(a)).to(dt).to(be.device)
        t_tp = dev(numpy.asarray(to_play, numpy.int32), torch.int32)
        t_noise = None if noise is None else dev(noise, torch.float64)
        t_tape = dev(tape if isinstance(tape, torch.Tensor) else tape.view(numpy.int32), torch.int32)
        out = dict(visits=be.zeros((B, A), torch.int32), root_value=be.zeros((B,), torch.float64),
                   predicted=be.zeros((B,), torch.float64), info=be.zeros((B, 4), torch.int32))
        io = _lib.SearchIO(None, None, be.ptr(t_tp), be.ptr(t_noise), be.ptr(t_tape), be.ptr(out["visits"]),
                           be.ptr(out["root_value"]), be.ptr(out["predicted"]), be.ptr(out["info"]))
        arena = self._arena
        lib.check(lib.mzx_search_run_continued(self.handle(B), ctypes.byref(io), be.ptr(arena), arena.numel(), be.stream()))
        res = {k: v.cpu().numpy() for k, v in out.items()}
        info = res["info"]
        for i in range(B if states is not None else 0):      # rewind, then consume exactly what the device consumed
            rngs[i].set_state(states[i])
            if info[i, 2]:
                rngs[i].randint(0, 2 ** 32, size=int(info[i, 2]), dtype=numpy.uint32)
        if (info[:, 1] != 0).any():
            self._carry = None
            bad = numpy.nonzero(info[:, 1])[0][:8]
            raise _lib.MzxError(f"continued search flagged trees {bad} (flags {set(info[:, 1])}): 1 = tie-break tape "
                                f"exhausted ({TAPE_WORDS} words; continued searches are not re-run), 4 = not an expanded child")
        result = SearchResult(res["visits"], res["root_value"], [None] * B, info, [list(a) for a in root_actions])
        self._note_searched(B, root_actions, res["visits"])
        return result

    def continue_search(self, actions, to_play, add_exploration_noise, rngs=None, streams=None, counter=None):
        """
        MCTS.run(model, None, _, to_play_i, add_exploration_noise, override_root_with=old_root_i.children[actions[i]])
        (self_play.py:260-361) for the B trees the last ``run`` / ``continue_search`` / ``run_from_trees`` of this engine
        left on the device; ``actions[i] = -1`` searches old root i itself again.  The chosen subtree is carried on the
        device (``mzx_search_advance``): visits, values, priors and hidden states stay, ``num_simulations`` more
        simulations follow (Dirichlet noise over the carried root's children, fresh MinMaxStats).  Returns a
        ``SearchResult`` (``root_predicted_values`` are None, as in the reference); ``export_trees`` / ``node_graph``
        read the continued trees.  rngs: B numpy RandomState-like objects; None (device draws): noise and tape come
        from one ``mzx_selfplay_draws`` call under (``draw_seed``, ``streams``, ``counter``) and never visit the host
        (what stays per tree on the host is list bookkeeping: the action check and the root action lists of the result).
        """
        self._require_capacity()
        B = len(actions)
        c = self._carry
        if c is None or c["B"] != B:
            raise ValueError("continue_search: no searched trees of this shard size to continue (run them first)")
        A = self.A
        acts = numpy.asarray(actions, numpy.int32).reshape(B)
        root_actions = []
        for i, a in enumerate(acts.tolist()):
            if a < 0:
                root_actions.append(c["root_actions"][i])
                continue
            if a not in c["root_actions"][i] or c["visits"][i, a] == 0:
                raise ValueError(f"continue_search: action {a} of tree {i} is not an expanded child of its root")
            root_actions.append(list(range(A)))
        root_n = [len(r) for r in root_actions]
        noise, tape, states = self._root_draws(root_n, add_exploration_noise, rngs, self._draw_ids(B, rngs, streams, counter))
        be = self.backend
        if self._arena_alt is None or self._arena_alt.numel() != self._arena.numel():
            self._arena_alt = be.zeros((self._arena.numel(),), torch.uint8)
        t_act = torch.as_tensor(acts).to(be.device)
        self._carry = None
        lib = be.lib
        lib.check(lib.mzx_search_advance(self.handle(B), be.ptr(t_act), be.ptr(self._arena), be.ptr(self._arena_alt),
                                         be.stream()))
        self._arena, self._arena_alt = self._arena_alt, self._arena
        return self._run_continued(B, root_actions, to_play, noise, tape, states, rngs)

    def run_from_trees(self, roots, to_play, add_exploration_noise, rngs=None, streams=None, counter=None):
        """
        MCTS.run(..., override_root_with=root) (self_play.py:260-361) for B expanded reference ``Node`` graphs that may
        already carry visits and expanded descendants: the graphs are flattened on the host (hidden states from
        ``node.hidden_state``), loaded (``mzx_search_load``) and searched ``num_simulations`` more times; each given
        root is then updated in place with the searched tree, as ``MCTS.run`` does for a fresh override.  Node order:
        the ``canonical_index`` ``node_graph`` records, else depth first in action order (the statistics do not depend
        on it).  Returns the ``SearchResult``.
        """
        self._require_capacity()
        B, A, M, Hf = len(roots), self.A, self.num_nodes, self.model.hidden_size
        arr = dict(visit=numpy.zeros((B, M), numpy.int32), value_sum=numpy.zeros((B, M)), reward=numpy.zeros((B, M)),
                   to_play=numpy.full((B, M), -1, numpy.int32), parent=numpy.full((B, M), -1, numpy.int32),
                   child=numpy.full((B, M, A), -1, numpy.int32), prior=numpy.zeros((B, M, A)),
                   hidden=numpy.zeros((B, M, Hf), numpy.float32), n_nodes=numpy.zeros(B, numpy.int32),
                   root_actions=numpy.full((B, A), -1, numpy.int32))
        root_actions = []
        for i, root in enumerate(roots):
            if not root.expanded() or root.hidden_state is None:
                raise ValueError("run_from_trees: every root must be an expanded Node with a hidden_state")
            if root.to_play != to_play[i]:
                raise ValueError("run_from_trees: root.to_play must equal the to_play argument")
            nodes = self._flatten(root)
            if len(nodes) + self.num_simulations + 1 > M:
                raise ValueError(f"run_from_trees: tree {i} has {len(nodes)} nodes; the engine holds "
                                 f"{M - self.num_simulations - 1} carried nodes (max_carried_nodes)")
            index = {id(n): k for k, n in enumerate(nodes)}
            acts = list(root.children.keys())
            root_actions.append(acts)
            arr["root_actions"][i, : len(acts)] = acts
            arr["n_nodes"][i] = len(nodes)
            for k, n in enumerate(nodes):
                arr["visit"][i, k], arr["value_sum"][i, k] = n.visit_count, n.value_sum
                arr["reward"][i, k], arr["to_play"][i, k] = n.reward, n.to_play
                arr["hidden"][i, k] = n.hidden_state.detach().reshape(-1).to("cpu", torch.float32).numpy()
                for slot, (a, ch) in enumerate(n.children.items()):
                    s = slot if k == 0 else a
                    arr["prior"][i, k, s] = ch.prior
                    if ch.expanded():
                        arr["child"][i, k, s] = index[id(ch)]
                        arr["parent"][i, index[id(ch)]] = k
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        h = _lib.TreeLoad(M, *[ptr(arr[k]) for k in ("visit", "value_sum", "reward", "to_play", "parent", "child", "prior",
                                                      "hidden", "n_nodes", "root_actions")])
        be = self.backend
        arena = self.arena(B)
        self._carry = None
        be.lib.check(be.lib.mzx_search_load(self.handle(B), ctypes.byref(h), be.ptr(arena), be.stream()))
        noise, tape, states = self._root_draws([len(r) for r in root_actions], add_exploration_noise, rngs,
                                               self._draw_ids(B, rngs, streams, counter))
        res = self._run_continued(B, root_actions, to_play, noise, tape, states, rngs)
        trees = self.export_trees(B)
        for i, root in enumerate(roots):      # the reference searches the given objects in place
            searched = self.node_graph(B, i, root_actions[i], _trees=trees)
            searched.hidden_state = root.hidden_state
            root.__dict__.update(searched.__dict__)
        return res

    def _flatten(self, root):
        """Expanded nodes of a Node graph, parents before children (see run_from_trees)."""
        nodes, stack = [], [root]
        while stack:
            n = stack.pop()
            if not n.expanded():
                continue
            if n.hidden_state is None:
                raise ValueError("run_from_trees: every expanded node needs its hidden_state")
            nodes.append(n)
            stack.extend(reversed(list(n.children.values())))
        if all(hasattr(n, "canonical_index") for n in nodes):
            nodes.sort(key=lambda n: n.canonical_index)
            if nodes[0] is not root:
                raise ValueError("run_from_trees: canonical_index of the root must be the smallest")
        return nodes

    def _staging(self, B, tape_words, obs_floats, with_noise, device_draws=False):
        """
        Persistent I/O of one (B, tape) geometry: ONE pinned host block + ONE device block for a move's inputs
        (observations | noise | legal | to_play | tape; 8-byte fields first) and one of each for its outputs
        (root value | predicted root value | visit counts | info) -- a move costs one upload, one launch, one
        download and one stream synchronisation instead of five uploads and four blocking downloads.
        ``device_draws``: noise and tape are device scratch outside the uploaded block (``draw_noise`` / ``draw_tape``);
        the inputs carry the temperatures, the outputs the chosen actions.
        """
        key = ("staging", B, tape_words, obs_floats, bool(with_noise)) + (("device_draws",) if device_draws else ())
        st = self._buffers.get(key)
        if st is not None:
            return st
        A, be = self.A, self.backend
        on_gpu = be.device.type == "cuda"

        def carve(fields):
            off, table = 0, {}
            for name, dtype, count in fields:
                nbytes = numpy.dtype(dtype).itemsize * count
                table[name] = (off, dtype, count)
                off += (nbytes + 15) & ~15
            return table, max(off, 16)

        if device_draws:
            fin, n_in = carve([("temperature", numpy.float64, B), ("obs", numpy.float32, B * obs_floats),
                               ("legal", numpy.int32, B * A), ("to_play", numpy.int32, B)])
            fout, n_out = carve([("root_value", numpy.float64, B), ("predicted", numpy.float64, B), ("action", numpy.int64, B),
                                 ("visits", numpy.int32, B * A), ("info", numpy.int32, B * 4)])
        else:
            fin, n_in = carve([("noise", numpy.float64, B * A if with_noise else 0), ("obs", numpy.float32, B * obs_floats),
                               ("legal", numpy.int32, B * A), ("to_play", numpy.int32, B), ("tape", numpy.uint32, B * tape_words)])
            fout, n_out = carve([("root_value", numpy.float64, B), ("predicted", numpy.float64, B),
                                 ("visits", numpy.int32, B * A), ("info", numpy.int32, B * 4)])
        h_in = torch.empty(n_in, dtype=torch.uint8, pin_memory=on_gpu)
        h_out = torch.empty(n_out, dtype=torch.uint8, pin_memory=on_gpu)
        d_in = be.empty((n_in,), torch.uint8) if on_gpu else h_in
        d_out = be.zeros((n_out,), torch.uint8) if on_gpu else h_out
        views = lambda block, table: {k: block.numpy()[o:o + numpy.dtype(dt).itemsize * c].view(dt)
                                      for k, (o, dt, c) in table.items()}
        st = dict(h_in=h_in, h_out=h_out, d_in=d_in, d_out=d_out, vin=views(h_in, fin), vout=views(h_out, fout),
                  pin={k: d_in.data_ptr() + o for k, (o, _, _) in fin.items()},
                  pout={k: d_out.data_ptr() + o for k, (o, _, _) in fout.items()}, on_gpu=on_gpu)
        if device_draws:
            st["draw_noise"] = be.zeros((B, A), torch.float64) if with_noise else None
            st["draw_tape"] = be.zeros((B, tape_words), torch.int32)
            st["draw_streams"] = be.zeros((B,), torch.int32)
        self._buffers[key] = st
        return st

    def _launch(self, B, obs, legal, to_play, noise, tape, tape_words, override):
        """One mzx_search_run / mzx_search_run_from_roots over B roots; host copies of the outputs."""
        lib, A = self.backend.lib, self.A
        obs_dev = obs if isinstance(obs, torch.Tensor) else None      # already stacked on the device (FrameStore)
        obs_floats = 0 if obs_dev is not None else int(obs.size // B)
        st = self._staging(B, tape_words, obs_floats, noise is not None)
        vin = st["vin"]
        if obs_dev is None:
            vin["obs"][:] = obs.reshape(-1)
        if noise is not None:
            vin["noise"][:] = noise.reshape(-1)
        vin["legal"][:] = legal.reshape(-1)
        vin["to_play"][:] = to_play
        vin["tape"][:] = tape.reshape(-1).view(numpy.uint32)
        if st["on_gpu"]:
            st["d_in"].copy_(st["h_in"], non_blocking=True)
        c_vp, pin, pout = ctypes.c_void_p, st["pin"], st["pout"]
        io = _lib.SearchIO(c_vp(obs_dev.data_ptr()) if obs_dev is not None else c_vp(pin["obs"]), c_vp(pin["legal"]),
                           c_vp(pin["to_play"]), c_vp(pin["noise"]) if noise is not None else c_vp(0), c_vp(pin["tape"]),
                           c_vp(pout["visits"]), c_vp(pout["root_value"]), c_vp(pout["predicted"]), c_vp(pout["info"]))
        arena = self.arena(B)
        handle = self.handle(B, tape_words)
        if override is not None:
            ptr = self.backend.ptr
            lib.check(lib.mzx_search_run_from_roots(handle, ctypes.byref(io), ptr(override["hidden"]),
                                                    ptr(override["priors"]), ptr(override["reward"]), ptr(arena),
                                                    arena.numel(), self.backend.stream()))
        else:
            lib.check(lib.mzx_search_run(handle, ctypes.byref(io), self.backend.ptr(arena), arena.numel(),
                                         self.backend.stream()))
        if st["on_gpu"]:
            st["h_out"].copy_(st["d_out"], non_blocking=True)
            torch.cuda.current_stream(self.backend.device).synchronize()
        vout = st["vout"]
        return (vout["visits"].reshape(B, A).copy(), vout["root_value"].copy(), vout["predicted"].copy(),
                vout["info"].reshape(B, 4).copy())

    def _fused_move(self, B, obs, legal, to_play, with_noise, asynchronous, call, bank=None, bank_idx=None):
        """
        What the two one-call moves share (``_move_search``: bank draws; ``_move_search_device``: ``bank`` None, noise and
        tape are device scratch): the pinned staging block, the ``Move`` struct (its fixed part filled once per geometry),
        the observation read from the device or from the host, the library call ``call(st, mv, n_legal, arena)`` -- its
        "Legal actions ..." failures raise AssertionError as self_play.py:296-301 does -- and the event behind an
        ``asynchronous`` call, which returns once the download is queued (MZX_MOVE_NO_SYNC; the staging block of this
        (B, tape) geometry is in use until then: one search in flight per engine).  Returns the move's ``_MoveOutputs``.
        """
        lib, A, be = self.backend.lib, self.A, self.backend
        obs_dev = obs if isinstance(obs, torch.Tensor) else None
        obs_floats = 0 if obs_dev is not None else int(obs.size // B)
        st = self._staging(B, TAPE_WORDS, obs_floats, with_noise, device_draws=bank is None)
        pin, pout, c_vp = st["pin"], st["pout"], ctypes.c_void_p
        mv = st.get("move")
        if mv is None:
            mv = st["move"] = _lib.Move()
            mv.num_games, mv.action_space_size, mv.tape_words = B, A, TAPE_WORDS
            mv.h_in, mv.d_in, mv.in_bytes = st["h_in"].data_ptr(), st["d_in"].data_ptr(), st["h_in"].numel()
            mv.h_out, mv.d_out, mv.out_bytes = st["h_out"].data_ptr(), st["d_out"].data_ptr(), st["h_out"].numel()
            if bank is None:
                noise, tape = be.ptr(st["draw_noise"]), be.ptr(st["draw_tape"])
            else:
                noise, tape = c_vp(pin["noise"]) if with_noise else c_vp(0), c_vp(pin["tape"])
            mv.io = _lib.SearchIO(c_vp(pin["obs"]), c_vp(pin["legal"]), c_vp(pin["to_play"]), noise, tape, c_vp(pout["visits"]),
                                  c_vp(pout["root_value"]), c_vp(pout["predicted"]), c_vp(pout["info"]))
        asynchronous = bool(asynchronous) and st["on_gpu"]
        if bank is not None:
            mv.num_threads = bank.threads
        mv.flags = _lib.MOVE_NO_SYNC if asynchronous else 0
        mv.streams = None if bank is None else bank_idx.ctypes.data
        mv.legal_actions, mv.to_play = legal.ctypes.data, to_play.ctypes.data
        mv.dirichlet_alpha, mv.add_exploration_noise = float(self.config.root_dirichlet_alpha), int(with_noise)
        if obs_dev is not None:
            mv.observation, mv.observation_floats = None, 0
            mv.io.d_observation = obs_dev.data_ptr()
        else:
            mv.observation, mv.observation_floats = obs.ctypes.data, obs_floats
        n_legal = numpy.empty(B, numpy.int32)
        rc = call(st, mv, n_legal, self.arena(B))
        if rc != 0:
            message = lib.mzx_last_error().decode()
            if message.startswith("Legal actions"):       # self_play.py:296-301 raise AssertionError
                raise AssertionError(message)
            lib.check(rc)
        done = None
        if asynchronous:
            done = st.get("event")
            if done is None:
                done = st["event"] = torch.cuda.Event()
            done.record(torch.cuda.current_stream(be.device))

        # (keep: the library read these during the call; the caller may reuse them after)
        return _MoveOutputs(st, (B, A), n_legal, done, with_noise and bank is not None, (obs, legal, to_play, bank_idx))

    def _move_search(self, B, obs, legal, to_play, bank, bank_idx, with_noise, asynchronous=False):
        """
        ``mzx_selfplay_search``: root draws of the bank straight into the pinned staging block, ONE upload, the search,
        ONE download, the stream synchronisation -- the statements of ``StreamBank.root_draws`` + ``_launch`` behind one
        call.  Returns what ``_fused_move`` returns.
        """
        lib, be = self.backend.lib, self.backend

        def call(st, mv, n_legal, arena):
            return lib.mzx_selfplay_search(self.handle(B, TAPE_WORDS), bank.handle, ctypes.byref(mv), n_legal.ctypes.data,
                                           be.ptr(arena), arena.numel(), be.stream())
        return self._fused_move(B, obs, legal, to_play, with_noise, asynchronous, call, bank, bank_idx)

    def _power_table(self, temps):
        """Device copies of ``draws.power_table`` over every visit count a search of this engine can report."""
        key = tuple(numpy.unique(temps[(temps != 0) & ~numpy.isinf(temps)]).tolist())
        entry = self._buffers.get(("pow", key))
        if entry is None:
            table, distinct = draws.power_table(numpy.array(key, numpy.float64), self.num_nodes + 1)
            dev = lambda a: None if a is None else torch.as_tensor(a).to(self.backend.device)
            entry = self._buffers[("pow", key)] = (dev(table), dev(distinct) if len(key) else None, table, distinct)
        return entry

    def _move_search_device(self, B, obs, legal, to_play, ids, with_noise, temperature, asynchronous=False):
        """
        ``mzx_selfplay_move_device``: the legal rows validated and staged, ONE upload, the draws, the search, the action
        choice (``temperature`` [B], or None: none), ONE download -- one library call, no host stream, no per-game loop.
        Returns what ``_fused_move`` returns; its ``actions`` attribute hands out the chosen actions.
        """
        lib, A, be, c_vp = self.backend.lib, self.A, self.backend, ctypes.c_void_p
        streams, counter = ids

        def call(st, mv, n_legal, arena):
            d = _lib.Draws(seed=self.draw_seed & (2 ** 64 - 1), counter=counter & (2 ** 64 - 1), num_games=B, action_space_size=A,
                           tape_words=TAPE_WORDS, dirichlet_alpha=float(self.config.root_dirichlet_alpha))
            if numpy.array_equal(streams, streams[0] + numpy.arange(B, dtype=numpy.int32)):
                d.first_stream = int(streams[0])
            else:
                st["draw_streams"].copy_(torch.as_tensor(streams))
                d.d_streams = be.ptr(st["draw_streams"])
            sel = None
            if temperature is not None:
                st["vin"]["temperature"][:] = temperature
                table, distinct, _, _ = self._power_table(temperature)
                sel = _lib.DrawsSelect(d_temperature=c_vp(st["pin"]["temperature"]), d_pow_table=be.ptr(table),
                                       d_table_temperatures=be.ptr(distinct), table_stride=0 if table is None else table.shape[1],
                                       num_temperatures=0 if table is None else table.shape[0], d_action=c_vp(st["pout"]["action"]))
            return lib.mzx_selfplay_move_device(self.handle(B, TAPE_WORDS), ctypes.byref(mv), ctypes.byref(d),
                                                None if sel is None else ctypes.byref(sel), n_legal.ctypes.data, be.ptr(arena),
                                                arena.numel(), be.stream())
        outputs = self._fused_move(B, obs, legal, to_play, with_noise, asynchronous, call)
        outputs.select, outputs.device_noise = temperature is not None, outputs.staging["draw_noise"]
        return outputs

    def run(self, observations, legal_actions, to_play, add_exploration_noise, rngs=None, _override=None, _defer_advance=False,
            _asynchronous=False, streams=None, counter=None, temperature=None):
        """
        observations: B stacked observations; legal_actions: B lists; to_play: B ints;
        rngs: B numpy RandomState-like objects (dirichlet / randint / get_state / set_state), or a pair
        ``(StreamBank, stream indices)`` -- the native bank serves all B games, and the whole host side of the
        move (draws, staging, upload, search, download) is ONE call into the library (``mzx_selfplay_search``).
        ``_defer_advance``: leave the consumption of the tie-break words to ``SelfPlay._select_actions_bank``
        (``mzx_selfplay_select`` does it in the same pass as the action draw); ``result.pending_words`` holds them.
        ``_asynchronous`` (bank searches): returns a ``PendingSearch`` as soon as the search is queued on the device;
        its ``result()`` waits and completes the call -- the host steps another group of games in between.
        ``rngs=None`` (device draws): noise, tape and -- with ``temperature`` (a number or [B]) -- the action choice are
        drawn on the device under (``draw_seed``, ``streams``, ``counter``): ONE ``mzx_selfplay_move_device`` call;
        ``result.actions`` holds the chosen actions.
        """
        cfg, A = self.config, self.A
        B = len(legal_actions)
        bank = None
        ids = self._draw_ids(B, rngs, streams, counter)
        if temperature is not None:
            if ids is None:
                raise ValueError("temperature= belongs to device draws (rngs=None)")
            temperature = numpy.ascontiguousarray(numpy.broadcast_to(numpy.asarray(temperature, numpy.float64), (B,)))
        if isinstance(rngs, tuple):
            bank, bank_idx = rngs
            bank_idx = numpy.ascontiguousarray(bank_idx, dtype=numpy.int32)
            assert bank_idx.size == B
        elif ids is None:
            assert len(rngs) == B
        assert len(to_play) == B
        legal = numpy.full((B, A), -1, numpy.int32)
        n_legal = numpy.empty(B, numpy.int32)
        action_set = set(cfg.action_space)
        fused = self.fused_move and bank is not None and _override is None     # the move's host side behind one library call
        device_fused = ids is not None and _override is None
        if isinstance(legal_actions, numpy.ndarray):   # batched protocol: [B][A] int32, lists padded with -1
            legal = numpy.ascontiguousarray(legal_actions, dtype=numpy.int32)
            assert legal.shape == (B, A), "legal_actions array must be [num_trees][len(action_space)]"
            if not (fused or device_fused):            # (mzx_selfplay_search / _move_device validate the rows themselves)
                n_legal = (legal >= 0).sum(1).astype(numpy.int32)
                assert (n_legal > 0).all(), "Legal actions should not be an empty array."
                assert (legal < A).all() and ((legal >= 0) == (numpy.arange(A)[None, :] < n_legal[:, None])).all(), \
                    "Legal actions should be a subset of the action space (padded with -1 at the end)."
            legal_actions = legal
        if not isinstance(legal_actions, numpy.ndarray) and B > 1 and legal_actions.count(legal_actions[0]) == B:
            # every game offers the same list (the common case): validate it once (self_play.py:296-301)
            acts = legal_actions[0]
            assert acts, f"Legal actions should not be an empty array. Got {acts}."
            assert set(acts).issubset(action_set), "Legal actions should be a subset of the action space."
            assert len(set(acts)) == len(acts), "Legal actions must not repeat."
            legal[:, : len(acts)] = acts
            n_legal[:] = len(acts)
            shared = [list(acts)] * B
        else:
            shared = None
        for i, acts in enumerate(legal_actions if not isinstance(legal_actions, numpy.ndarray) and shared is None else ()):
            # self_play.py:296-301
            assert acts, f"Legal actions should not be an empty array. Got {acts}."
            assert set(acts).issubset(action_set), "Legal actions should be a subset of the action space."
            assert len(set(acts)) == len(acts), "Legal actions must not repeat."
            legal[i, : len(acts)] = acts
            n_legal[i] = len(acts)
        states = None
        if fused or device_fused:
            noise = tape = None
        elif ids is not None:                          # given roots: the draws by one library call, then the ordinary launch
            t_noise, t_tape = draws.root_draws(self.backend, self.draw_seed, ids[1], B, A, TAPE_WORDS, alpha=cfg.root_dirichlet_alpha,
                                               legal=legal, streams=ids[0], noise=bool(add_exploration_noise))
            noise = None if t_noise is None else t_noise.cpu().numpy()
            tape = t_tape.cpu().numpy().view(numpy.uint32)
        elif bank is not None:
            noise, tape = bank.root_draws(bank_idx, cfg.root_dirichlet_alpha, n_legal, A, TAPE_WORDS,
                                          with_noise=bool(add_exploration_noise))
        else:
            noise = numpy.zeros((B, A), numpy.float64) if add_exploration_noise else None
            tape = numpy.zeros((B, TAPE_WORDS), numpy.uint32)
            states = []
            for i in range(B):
                if add_exploration_noise:
                    noise[i, : n_legal[i]] = rngs[i].dirichlet([cfg.root_dirichlet_alpha] * int(n_legal[i]))
                states.append(rngs[i].get_state())
                tape[i] = rngs[i].randint(0, 2 ** 32, size=TAPE_WORDS, dtype=numpy.uint32)
        if _override is not None:
            obs = numpy.zeros((B, 1), numpy.float32)    # not read: the roots are given
        elif isinstance(observations, torch.Tensor):   # already stacked on the device (mzx.observations.FrameStore)
            assert observations.shape[0] == B
            obs = observations.reshape(B, -1)
        else:
            obs = numpy.ascontiguousarray(numpy.asarray(observations, dtype=numpy.float32).reshape(B, -1))
        to_play = numpy.ascontiguousarray(to_play, dtype=numpy.int32)
        outputs = None
        if fused:
            outputs = self._move_search(B, obs, legal, to_play, bank, bank_idx, bool(add_exploration_noise), _asynchronous)
        elif device_fused:
            outputs = self._move_search_device(B, obs, legal, to_play, ids, bool(add_exploration_noise), temperature, _asynchronous)
        job = types.SimpleNamespace(outputs=outputs, B=B, obs=obs, legal=legal, legal_actions=legal_actions, shared=shared,
                                    to_play=to_play, n_legal=n_legal, noise=noise, tape=tape, bank=bank,
                                    bank_idx=bank_idx if bank is not None else None, rngs=rngs, states=states, override=_override,
                                    defer_advance=_defer_advance, ids=ids, temperature=temperature)
        pending = PendingSearch(lambda: self._complete_run(job))
        return pending if _asynchronous else pending.result()

    def _complete_run(self, job):
        """The second half of ``run``: outputs of the (possibly still running) search, tape retries, the result record.
        ``job``: what ``run`` staged -- the inputs as the launch takes them, the draws or where they come from."""
        cfg, A = self.config, self.A
        B, n_legal, noise = job.B, job.n_legal, job.noise      # (the one-call moves hand n_legal and the noise out themselves)
        if job.outputs is not None:
            visits, root_values, predicted, info, n_legal, noise = job.outputs()
        else:
            visits, root_values, predicted, info = self._launch(B, job.obs, job.legal, job.to_play, noise, job.tape, TAPE_WORDS, job.override)
        # A tree that exhausted its tie-break tape (a network with equal priors ties at every level) is searched
        # again with a longer tape: same roots, same noise, the stream peeked further -- the reference never
        # fails here (numpy.random.choice at self_play.py:371 simply keeps drawing).
        words = TAPE_WORDS
        redone = numpy.zeros(B, bool)
        while (info[:, 1] & 1).any():
            words *= 8
            if words > (1 << 22):
                raise _lib.MzxError("tie-break tape: a search consumed more than 4M random words")
            redo = numpy.nonzero(info[:, 1] & 1)[0]
            redone[redo] = True
            self.tape_retries += len(redo)
            if job.ids is not None:      # a longer tape under the same (stream, counter) begins with the shorter one
                _, t_tape = draws.root_draws(self.backend, self.draw_seed, job.ids[1], len(redo), A, words, streams=job.ids[0][redo], noise=False)
                long_tape = t_tape.cpu().numpy().view(numpy.uint32)
                if noise is None and getattr(job.outputs, "device_noise", None) is not None:
                    noise = job.outputs.device_noise.cpu().numpy()      # (read before _launch below draws anything)
            elif job.bank is not None:
                _, long_tape = job.bank.root_draws(job.bank_idx[redo], cfg.root_dirichlet_alpha, n_legal[redo], A, words,
                                               with_noise=False)
            else:
                long_tape = numpy.zeros((len(redo), words), numpy.uint32)
                for k, i in enumerate(redo):
                    job.rngs[i].set_state(job.states[i])
                    long_tape[k] = job.rngs[i].randint(0, 2 ** 32, size=words, dtype=numpy.uint32)
            ov = None if job.override is None else {k: v[torch.as_tensor(redo, device=v.device)] for k, v in job.override.items()}
            sub_obs = job.obs[torch.as_tensor(redo, device=job.obs.device)] if isinstance(job.obs, torch.Tensor) else job.obs[redo]
            v2, r2, p2, i2 = self._launch(len(redo), sub_obs, job.legal[redo], job.to_play[redo],
                                          None if noise is None else noise[redo], long_tape, words, ov)
            visits[redo], root_values[redo], predicted[redo], info[redo] = v2, r2, p2, i2
        self._carry = None      # (the re-runs used the arena at other shard sizes: the trees of this run are gone)
        if words == TAPE_WORDS:
            self._note_searched(B, [list(job.legal[i, : int((job.legal[i] >= 0).sum())]) for i in range(B)], visits)
        result = SearchResult(visits, root_values, predicted, info,
                              job.legal_actions if isinstance(job.legal_actions, numpy.ndarray) else
                              (job.shared if job.shared is not None else [list(a) for a in job.legal_actions]))
        if job.shared is not None:
            result.shared_legal = job.shared[0]
        if (info[:, 1] != 0).any():
            raise _lib.MzxError(f"search flagged trees {numpy.nonzero(info[:, 1])[0][:8]} (flags {set(info[:, 1])}): "
                                "node arena exhausted")
        result.actions = None
        if job.ids is not None:
            result.legal_array, result.n_legal, result.streams = job.legal, n_legal, job.ids[0]
            if job.temperature is not None:
                result.actions = getattr(job.outputs, "actions", None)
                again = numpy.arange(B) if result.actions is None else numpy.nonzero(redone)[0]
                if again.size:       # the searches run again (and the given roots): the same select function over them
                    if result.actions is None:
                        result.actions = numpy.zeros(B, numpy.int64)
                    _, _, table, distinct = self._power_table(job.temperature)
                    result.actions[again] = draws.select(self.backend, self.draw_seed, job.ids[1], job.legal[again], visits[again],
                                                         job.temperature[again], table, distinct, streams=job.ids[0][again]).cpu().numpy()
        elif job.bank is not None:
            result.legal_array, result.n_legal, result.streams = job.legal, n_legal, job.bank_idx
            if job.defer_advance and self.fused_move:     # (the numpy action draw of the A/B switch does not advance)
                result.pending_words = numpy.ascontiguousarray(info[:, 2], dtype=numpy.int32)
            else:
                job.bank.advance(job.bank_idx, info[:, 2])   # consume exactly what the device consumed
        else:
            for i in range(B):  # rewind, then consume exactly what the device consumed
                job.rngs[i].set_state(job.states[i])
                if info[i, 2]:
                    job.rngs[i].randint(0, 2 ** 32, size=int(info[i, 2]), dtype=numpy.uint32)
        return result


class MCTS:
    """self_play.py:249-361 -- single-root form, same signature and return value."""

    def __init__(self, config):
        self.config = config

    def run(self, model, observation, legal_actions, to_play, add_exploration_noise, override_root_with=None):
        # the single-root facade returns the whole searched tree as Node objects, like the reference; it uses
        # the per-operator engine, whose arena keeps every node's hidden state
        engine = getattr(model, "_mcts_engine", None)
        if engine is None or engine.config is not self.config:
            engine = BatchedMCTS(self.config, model, 1, mode=0)
            model._mcts_engine = engine
        rng = [numpy.random.mtrand._rand]
        if override_root_with:
            res = engine.run_from_roots([override_root_with], [to_play], add_exploration_noise, rng)
            searched = engine.node_graph(1, 0, res.legal_actions[0])
            searched.hidden_state = override_root_with.hidden_state
            override_root_with.__dict__.update(searched.__dict__)   # the reference searches the given object in place
            root, predicted = override_root_with, None
        else:
            res = engine.run([observation], [list(legal_actions)], [to_play], add_exploration_noise, rng)
            root, predicted = engine.node_graph(1, 0, res.legal_actions[0]), float(res.root_predicted_values[0])
        extra_info = {
            "max_tree_depth": int(res.max_tree_depth[0]),
            "root_predicted_value": predicted,
        }
        return root, extra_info
