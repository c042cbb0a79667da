"""
TEST HELPER -- continued searches on the oracle's canonical-index ``Tree`` (oracle/mcts_oracle.py).

``carry(tree, cfg, action)`` is what ``MCTS.run(..., override_root_with=old_root.children[action])`` starts from
(/root/reference/self_play.py:260-361; ``action = -1``: the old root itself): the subtree under the chosen node,
renumbered in creation order (increasing old index, the new root at 0).  ``continue_search`` restates only the
``run_search`` loop from such a tree and reuses the oracle's ``_select_slot`` / ``_expand`` / ``_backpropagate``:
Dirichlet noise over the root's existing children (:467-476), fresh MinMaxStats, ``root_predicted_value`` None.

Also here: ``ReplayValues`` (deterministic network outputs shared by the oracle and the lock-step ABI) and
``LockstepCarry``, the lock-step driver of continued searches on any backend (tests/hostcheck or the GPU library).
"""
import ctypes
import math

import numpy
import torch

from mzx import _lib
from oracle import mcts_oracle as mo


def carry(tree, cfg, action):
    c = 0 if action < 0 else tree.child[0][tree.actions[0].index(action)]
    assert c >= 0, "the chosen child is not expanded"
    new = {}
    for n in range(len(tree.visit)):
        if n == c or (n > c and tree.parent[n] in new):
            new[n] = len(new)
    t = mo.Tree()
    for n in sorted(new):
        t.actions.append(list(tree.actions[n]))
        t.visit.append(tree.visit[n])
        t.value_sum.append(tree.value_sum[n])
        t.reward.append(tree.reward[n])
        t.to_play.append(tree.to_play[n])
        t.hidden.append(tree.hidden[n])
        t.prior.append(list(tree.prior[n]))
        t.child.append([new[x] if x >= 0 else -1 for x in tree.child[n]])
        t.parent.append(-1 if n == c else new[tree.parent[n]])
        t.parent_slot.append(-1 if n == c else tree.parent_slot[n])
    return t


def continue_search(cfg, evaluator, tree, to_play, add_exploration_noise, rng, num_simulations=None):
    """MCTS.run(model, None, _, to_play, add_exploration_noise, override_root_with=<root of tree>); mutates `tree`."""
    assert tree.to_play[0] == to_play
    tree.minimum, tree.maximum = float("inf"), -float("inf")      # MinMaxStats() per call, self_play.py:306
    tree.trace, tree.margins, tree.value_margins = [], [], []
    tree.max_depth, tree.tie_draws, tree.root_predicted_value = 0, 0, None
    root = 0
    if add_exploration_noise:
        noise = rng.dirichlet([cfg.root_dirichlet_alpha] * len(tree.actions[root]))
        frac = cfg.root_exploration_fraction
        tree.prior[root] = [p * (1 - frac) + n * frac for p, n in zip(tree.prior[root], noise)]
    sims = cfg.num_simulations if num_simulations is None else num_simulations
    for _ in range(sims):
        virtual_to_play = to_play
        node, path, depth = root, [root], 0
        tree._sim_margin = (float("inf"), 0)
        tree._sim_value_margin = float("inf")
        while True:
            depth += 1
            slot = mo._select_slot(tree, cfg, node, rng)
            if virtual_to_play + 1 < len(cfg.players):
                virtual_to_play = cfg.players[virtual_to_play + 1]
            else:
                virtual_to_play = cfg.players[0]
            nxt = tree.child[node][slot]
            if nxt < 0:
                break
            node = nxt
            path.append(node)
        parent = node
        action = tree.actions[parent][slot]
        leaf = mo._new_node(tree, parent, slot)
        tree.child[parent][slot] = leaf
        path.append(leaf)
        value, reward, priors, hidden = evaluator.recurrent(tree.hidden[parent], action, list(cfg.action_space))
        mo._expand(tree, leaf, cfg.action_space, virtual_to_play, reward, priors, hidden)
        mo._backpropagate(tree, cfg, path, value, virtual_to_play)
        tree.max_depth = max(tree.max_depth, depth)
        tree.trace.append((parent, int(action), depth))
    return tree


class ReplayValues:
    """Network outputs of tree i as a seeded sequence: expansion k gets (value, reward, priors) number k."""

    def __init__(self, seed, count, A, ties=False):
        r = numpy.random.RandomState(seed)
        self.values = r.uniform(-1, 1, count)
        self.rewards = r.uniform(-0.5, 0.5, count)
        p = r.uniform(0.05, 1.0, (count, A))
        if ties:      # equal priors: the unvisited children of a node tie, the tape decides
            p[:, :] = 1.0
        self.priors = p / p.sum(1, keepdims=True)
        self.k = 0

    def _next(self, actions):
        k = self.k
        self.k += 1
        return float(self.values[k]), float(self.rewards[k]), [float(x) for x in self.priors[k][: len(actions)]], None

    def initial(self, observation, actions):
        return self._next(actions)

    def recurrent(self, hidden, action, actions):
        return self._next(actions)


def tables(cfg, n):
    pbc = (ctypes.c_double * n)(*[math.log((k + cfg.pb_c_base + 1) / cfg.pb_c_base) + cfg.pb_c_init for k in range(n)])
    sq = (ctypes.c_double * n)(*[math.sqrt(k) for k in range(n)])
    return pbc, sq


class LockstepCarry:
    """
    The tree arithmetic of fresh and continued searches through the C ABI's lock-step calls (a handle without a network):
    begin / select / apply / finish for the first search, then mzx_search_advance + mzx_search_run_continued + select /
    apply / finish per continuation, the network outputs from ``ReplayValues``.
    """

    TAPE = 64

    def __init__(self, backend, cfg, B, S, max_nodes):
        self.be, self.lib, self.cfg, self.B, self.S, self.A = backend, backend.lib, cfg, B, S, len(cfg.action_space)
        self.N = max_nodes
        self._t0 = tables(cfg, S + 1)
        c = _lib.SearchConfig()
        c.num_trees, c.num_simulations, c.action_space_size = B, S, self.A
        c.num_players, c.support_size, c.tape_words = len(cfg.players), cfg.support_size, self.TAPE
        c.discount, c.root_exploration_fraction = float(cfg.discount), float(cfg.root_exploration_fraction)
        c.h_pb_c_table = ctypes.cast(self._t0[0], ctypes.POINTER(ctypes.c_double))
        c.h_sqrt_table = ctypes.cast(self._t0[1], ctypes.POINTER(ctypes.c_double))
        self.handle = ctypes.c_void_p()
        self.lib.check(self.lib.mzx_search_create(ctypes.byref(c), None, ctypes.byref(self.handle)))
        self._t1 = tables(cfg, max_nodes)
        self.lib.check(self.lib.mzx_search_set_capacity(self.handle, max_nodes, *self._t1))
        nbytes = self.lib.mzx_search_arena_bytes(self.handle)
        self.arenas = [backend.zeros((nbytes,), torch.uint8), backend.zeros((nbytes,), torch.uint8)]

    def close(self):
        self.lib.mzx_search_destroy(self.handle)

    def dev(self, a, dtype):
        return torch.as_tensor(numpy.ascontiguousarray(a)).to(dtype).to(self.be.device)

    def _draws(self, rngs, root_n, noise_on):
        B, A = self.B, self.A
        noise = numpy.zeros((B, A)) if noise_on else None
        tape = numpy.zeros((B, self.TAPE), numpy.uint32)
        states = []
        for i in range(B):
            if noise_on:
                noise[i, : root_n[i]] = rngs[i].dirichlet([self.cfg.root_dirichlet_alpha] * root_n[i])
            states.append(rngs[i].get_state())
            tape[i] = rngs[i].randint(0, 2 ** 32, size=self.TAPE, dtype=numpy.uint32)
        return noise, tape, states

    def _io(self, legal, to_play, noise, tape, out):
        be = self.be
        keep = [None if legal is None else self.dev(legal, torch.int32), self.dev(to_play, torch.int32),
                None if noise is None else self.dev(noise, torch.float64), self.dev(tape.view(numpy.int32), torch.int32)]
        io = _lib.SearchIO(None, be.ptr(keep[0]), be.ptr(keep[1]), be.ptr(keep[2]), be.ptr(keep[3]), be.ptr(out["visits"]),
                           be.ptr(out["root_value"]), be.ptr(out["predicted"]), be.ptr(out["info"]))
        return io, keep

    def _simulate(self, io, evals, arena):
        be, lib, B, A = self.be, self.lib, self.B, self.A
        sel = [be.zeros((B,), torch.int32) for _ in range(3)]
        st = be.stream()
        for _ in range(self.S):
            lib.check(lib.mzx_search_lockstep_select(self.handle, ctypes.byref(io), *[be.ptr(t) for t in sel], be.ptr(arena), st))
            v, r, p = numpy.zeros(B), numpy.zeros(B), numpy.zeros((B, A))
            for i, e in enumerate(evals):
                v[i], r[i], pr, _ = e.recurrent(None, None, list(self.cfg.action_space))
                p[i] = pr
            tv, tr, tp = self.dev(v, torch.float64), self.dev(r, torch.float64), self.dev(p, torch.float64)
            lib.check(lib.mzx_search_lockstep_apply(self.handle, be.ptr(tv), be.ptr(tr), be.ptr(tp), be.ptr(arena), st))

    def _finish(self, io, out, arena, rngs, states):
        self.lib.check(self.lib.mzx_search_finish(self.handle, ctypes.byref(io), self.be.ptr(arena), self.be.stream()))
        res = {k: v.cpu().numpy() for k, v in out.items()}
        for i in range(self.B):
            rngs[i].set_state(states[i])
            if res["info"][i, 2]:
                rngs[i].randint(0, 2 ** 32, size=int(res["info"][i, 2]), dtype=numpy.uint32)
        res.update(self.dump(arena))
        return res

    def _out(self):
        be, B, A = self.be, self.B, self.A
        return dict(visits=be.zeros((B, A), torch.int32), root_value=be.zeros((B,), torch.float64),
                    predicted=be.zeros((B,), torch.float64), info=be.zeros((B, 4), torch.int32))

    def fresh(self, legal, to_play, noise_on, rngs, evals):
        B, A = self.B, self.A
        lg = numpy.full((B, A), -1, numpy.int32)
        for i, acts in enumerate(legal):
            lg[i, : len(acts)] = acts
        noise, tape, states = self._draws(rngs, [len(a) for a in legal], noise_on)
        pri, rew = numpy.zeros((B, A)), numpy.zeros(B)
        for i, e in enumerate(evals):
            _, rew[i], p, _ = e.initial(None, legal[i])
            pri[i, : len(p)] = p
        out = self._out()
        io, keep = self._io(lg, to_play, noise, tape, out)
        arena = self.arenas[0]
        tp, tr = self.dev(pri, torch.float64), self.dev(rew, torch.float64)
        self.lib.check(self.lib.mzx_search_lockstep_begin(self.handle, ctypes.byref(io), self.be.ptr(tp), self.be.ptr(tr),
                                                          self.be.ptr(arena), arena.numel(), self.be.stream()))
        self._simulate(io, evals, arena)
        return self._finish(io, out, arena, rngs, states)

    def advance(self, actions):
        """mzx_search_advance from the current arena into the other one; returns the library's return code."""
        t = self.dev(numpy.asarray(actions, numpy.int32), torch.int32)
        rc = self.lib.mzx_search_advance(self.handle, self.be.ptr(t), self.be.ptr(self.arenas[0]), self.be.ptr(self.arenas[1]),
                                         self.be.stream())
        if rc == 0:
            self.arenas.reverse()
        return rc

    def cont(self, root_n, to_play, noise_on, rngs, evals):
        """mzx_search_run_continued (root preparation) + the simulations + finish; raises MzxError on a refused call."""
        noise, tape, states = self._draws(rngs, root_n, noise_on)
        out = self._out()
        io, keep = self._io(None, to_play, noise, tape, out)
        arena = self.arenas[0]
        try:
            self.lib.check(self.lib.mzx_search_run_continued(self.handle, ctypes.byref(io), self.be.ptr(arena), arena.numel(),
                                                             self.be.stream()))
        except _lib.MzxError:
            for i in range(self.B):
                rngs[i].set_state(states[i])
            raise
        self._simulate(io, evals, arena)
        return self._finish(io, out, arena, rngs, states)

    def dump(self, arena):
        be, B, N, A = self.be, self.B, self.N, self.A
        t = dict(visit=be.zeros((B, N), torch.int32), value_sum=be.zeros((B, N), torch.float64),
                 reward=be.zeros((B, N), torch.float64), to_play=be.zeros((B, N), torch.int32),
                 parent=be.zeros((B, N), torch.int32), child=be.zeros((B, N, A), torch.int32),
                 prior=be.zeros((B, N, A), torch.float64), minmax=be.zeros((B, 2), torch.float64),
                 n_nodes=be.zeros((B,), torch.int32))
        d = _lib.TreeDump(*[be.ptr(t[k]) for k in ("visit", "value_sum", "reward", "to_play", "parent", "child", "prior",
                                                   "minmax", "n_nodes")])
        self.lib.check(self.lib.mzx_search_dump(self.handle, ctypes.byref(d), be.ptr(arena), be.stream()))
        return {k: v.cpu().numpy() for k, v in t.items()}


def bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


def assert_tree_equal(got, i, tree, A, flags=0):
    """Tree i of a lock-step / engine dump against an oracle Tree, bit for bit (statistics, links, priors, min-max);
    `flags`: the status word the tree must report (4 = TF_BAD_CARRY: the advance kept the old root)."""
    n = len(tree.visit)
    assert got["n_nodes"][i] == n, (i, got["n_nodes"][i], n)
    assert numpy.array_equal(got["visit"][i, :n], tree.visit), i
    assert numpy.array_equal(bits(got["value_sum"][i, :n]), bits(tree.value_sum)), i
    assert numpy.array_equal(bits(got["reward"][i, :n]), bits(tree.reward)), i
    assert numpy.array_equal(got["to_play"][i, :n], tree.to_play), i
    assert numpy.array_equal(got["parent"][i, :n], tree.parent), i
    for k in range(n):
        m = len(tree.actions[k])
        assert numpy.array_equal(got["child"][i, k, :m], tree.child[k]), (i, k)
        assert numpy.array_equal(bits(got["prior"][i, k, :m]), bits(tree.prior[k])), (i, k)
    assert numpy.array_equal(bits(got["minmax"][i]), bits([tree.minimum, tree.maximum])), i
    want = numpy.zeros(A, numpy.int32)
    for s, a in enumerate(tree.actions[0]):
        c = tree.child[0][s]
        want[a] = tree.visit[c] if c >= 0 else 0
    if "visits" in got:
        assert numpy.array_equal(got["visits"][i], want), i
        assert got["root_value"][i] == tree.node_value(0), i
        assert got["info"][i, 0] == tree.max_depth and got["info"][i, 1] == flags, i
