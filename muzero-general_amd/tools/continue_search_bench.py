"""
Continued searches (BatchedMCTS.continue_search): the time of one tree_advance_kernel launch and the simulations per
second of a continued search, next to a fresh ``run`` of the same size on the same engine (handles with spare node
capacity take the route a fresh search of the handle takes: fc2_search_kernel, rt_search_kernel, the streamed row route
or the per-operator path) and next to a fresh ``run`` of the default engine.  Wall times include the host side of
BatchedMCTS; ``continue_stream_ms`` is the device stream's time from the mzx_search_run_continued call to the end of its
last kernel (the root preparation and the simulations; the carried node counts' read-back included).  ``*_route`` is
mzx_search_route's out[0] (0 per-operator, 2 streamed rows, 3 rt_search_kernel, 4 fc2_search_kernel).  One JSON line
per workload.

    python muzero-general_amd/tools/continue_search_bench.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mzx import configs, models, self_play, synthetic  # noqa: E402

WORKLOADS = (("C2 cartpole FC", "cartpole", 4096, 50), ("connect4", "connect4", 1024, 200))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def route(engine, B):
    lib = engine.backend.lib
    out = (lib.mzx_search_route.argtypes[1]._type_)()
    lib.check(lib.mzx_search_route(engine.handle(B), out))
    return int(out[0])


class StreamTimed:
    """Events on the current stream around every call of one library entry point."""

    def __init__(self, lib, name):
        self.lib, self.name, self.fn, self.ms = lib, name, getattr(lib, name), []

    def __enter__(self):
        def call(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self.fn(*args)
            e1.record()
            self.pending.append((e0, e1))
            return rc
        self.pending = []
        setattr(self.lib, self.name, call)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.fn)
        torch.cuda.synchronize()
        self.ms += [a.elapsed_time(b) for a, b in self.pending]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for label, game, B, S in WORKLOADS:
        cfg = configs.BY_NAME[game](num_simulations=S)
        net = models.MuZeroNetwork(cfg)
        net.set_weights(synthetic.fill_state_dict(net.state_dict(), 0))
        obs = synthetic.observations(B, net.input_shape, seed=1)
        legal = [list(cfg.action_space)] * B
        rngs = lambda: [numpy.random.RandomState(7 + i) for i in range(B)]
        row = dict(workload=label, trees=B, sims=S)
        default = self_play.BatchedMCTS(cfg, net, B)
        default.run(list(obs), legal, [0] * B, True, rngs())
        t = min(timed(lambda: default.run(list(obs), legal, [0] * B, True, rngs()))[1] for _ in range(args.reps))
        row["run_default_sims_per_s"] = B * S / t
        row["run_default_kernel"] = default.kernel_name(B)
        row["run_default_route"] = route(default, B)
        del default
        engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=S + 1)
        P = len(cfg.players)
        runs, conts, advances, streams = [], [], [], []
        for _ in range(args.reps):
            st = rngs()
            res, t_run = timed(lambda: engine.run(list(obs), legal, [0] * B, True, st))
            runs.append(t_run)
            acts = [int(numpy.argmax(res.visit_counts[i])) for i in range(B)]
            with StreamTimed(engine.backend.lib, "mzx_search_run_continued") as tm:
                _, t_cont = timed(lambda: engine.continue_search(acts, [1 % P] * B, True, st))
            conts.append(t_cont)
            streams += tm.ms
            # one tree_advance_kernel launch alone, between the same two arenas (the trees just continued -> the other)
            h, lib, be = engine.handle(B), engine.backend.lib, engine.backend
            t_act = torch.as_tensor(numpy.asarray(acts, numpy.int32) * 0 - 1).to(be.device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.check(lib.mzx_search_advance(h, be.ptr(t_act), be.ptr(engine._arena), be.ptr(engine._arena_alt), be.stream()))
            e1.record()
            torch.cuda.synchronize()
            advances.append(e0.elapsed_time(e1) * 1e-3)
            engine._arena, engine._arena_alt = engine._arena_alt, engine._arena
            engine._carry = None
        row["run_spare_capacity_sims_per_s"] = B * S / min(runs)
        row["run_spare_capacity_route"] = route(engine, B)
        row["continue_sims_per_s"] = B * S / min(conts)
        row["continue_stream_ms"] = min(streams)
        row["continue_stream_sims_per_s"] = B * S / (1e-3 * min(streams))
        row["continue_kernel"] = engine.kernel_name(B)
        row["continue_route"] = route(engine, B)
        row["advance_ms_old_root"] = 1e3 * min(advances)
        off = engine.arena_offsets(B)
        row["arena_bytes"] = int(off["total"])
        print(json.dumps(row), flush=True)
        del engine
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
