"""
Reanalyse with fresh searches over a device-resident replay store (mzx.replay.DeviceGameStore), on the GPU: the SWEEP
(DeviceGameStore.reanalyse_search: per chunk of positions mzx_replay_positions, the observation gather,
mzx_replay_search_inputs, mzx_search_run, mzx_replay_search_write; then one mzx_replay_values and one download of a counter)
against the HOST-DRIVEN loop a user writes without it (per game: store.stacked, BatchedMCTS.run with per-tree host streams,
the GameHistory rebuilt from the result, update_game_history -- which uploads root values only) and against the SAME
engine's search alone (mzx_search_run on one chunk's inputs already in HBM) at the same trees x simulations, in one process.

    python muzero-general_amd/tools/reanalyse_search_bench.py [--out profiles/reanalyse_search_bench.log] [--quick]

Two shapes: CartPole (fully connected) 4096 trees x 50 simulations over 1024 games x 32 positions, and connect4 1024 trees x
200 simulations over 256 games of 7 .. 42 positions.  Per shape one JSON line (printed, and written to the log):
  sweep_ms, sweep_positions_per_s        one sweep over every resident game (chunk_positions, chunks, skipped)
  search_positions_per_s                 mzx_search_run alone, full chunks back to back
  sweep_share_of_search                  sweep rate / search-alone rate
  loop_positions_per_s, loop_games       the host-driven loop over the first loop_games games
  sweep_over_loop                        ratio of the two rates
Host clock around work that ends in a device synchronise; medians of timed blocks after a warm-up.  The stock buffer is a
small stand-in so that the tool needs nothing outside the repository.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "muzero-general_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mzx import _lib, configs, models, replay, self_play, synthetic  # noqa: E402
from mzx.search import TAPE_WORDS  # noqa: E402
from reanalyse_sweep_bench import Stock, make_games  # noqa: E402


def median_ms(fn, blocks):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def run(be, name, cfg, lengths, dtype, trees, simulations, loop_games, blocks):
    lib = be.lib
    games = make_games(cfg, lengths, dtype)
    total = int(sum(lengths))
    store = replay.DeviceGameStore(cfg, be, total + len(lengths))
    buffer = replay.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, cfg, stock=Stock, device_store=store)
    for g in games:
        buffer.save_game(g)
    model = models.MuZeroNetwork(cfg)
    model.set_weights(synthetic.fill_state_dict(model.state_dict(), 0))
    engine = self_play.BatchedMCTS(cfg, model, trees, num_simulations=simulations)
    report = {}

    def sweep():
        report.update(store.reanalyse_search(engine))

    sweep_ms = median_ms(sweep, blocks)

    # the search alone: one full chunk's inputs, built by the sweep's own kernels, searched back to back
    A, n = store.A, min(trees, total)
    ids = list(store.games)
    entries = [store.games[g] for g in ids]
    up = lambda a: torch.from_numpy(a).to(be.device)
    length = numpy.array([T for _, T in entries], dtype=numpy.int64)
    d = [up(numpy.array([b for b, _ in entries], dtype=numpy.int64)), up(length.astype(numpy.int32)),
         up(numpy.concatenate([[0], numpy.cumsum(length)[:-1]]).astype(numpy.int64))]
    s_base, s_len, s_pos = be.empty((n,), torch.int64), be.empty((n,), torch.int32), be.empty((n,), torch.int32)
    lib.check(lib.mzx_replay_positions(*(be.ptr(t) for t in d), len(ids), total, 0, n, be.ptr(s_base), be.ptr(s_len), be.ptr(s_pos),
                                       be.stream()))
    obs = store.gather(s_base, s_len, s_pos, targets=False)[0]
    to_play, flags = be.empty((n,), torch.int32), be.empty((n,), torch.int32)
    legal, tape = be.empty((n, A), torch.int32), be.empty((n, TAPE_WORDS), torch.int32)
    lib.check(lib.mzx_replay_search_inputs(ctypes.byref(store.pool), None, be.ptr(s_base), be.ptr(s_pos), n, TAPE_WORDS, 0, 0, 0,
                                           be.ptr(to_play), be.ptr(legal), be.ptr(tape), be.ptr(flags), be.stream()))
    out = [be.empty((n, A), torch.int32), be.empty((n,), torch.float64), be.empty((n,), torch.float64), be.empty((n, 4), torch.int32)]
    io = _lib.SearchIO(be.ptr(obs), be.ptr(legal), be.ptr(to_play), None, be.ptr(tape), *(be.ptr(t) for t in out))
    arena = engine.arena(n)
    repeats = max(1, -(-total // n))

    def search_alone():
        for _ in range(repeats):
            lib.check(lib.mzx_search_run(engine.handle(n, TAPE_WORDS), ctypes.byref(io), be.ptr(arena), arena.numel(), be.stream()))

    search_ms = median_ms(search_alone, blocks)
    kernel = engine.kernel_name(n)

    # the host-driven loop over the first games: download-free gather, host draws, search, rebuild, update
    loop_ids = [g for g in ids if store.games[g][1]][:loop_games]
    loop_positions = sum(store.games[g][1] for g in loop_ids)
    rngs = [numpy.random.RandomState(i) for i in range(int(max(lengths)))]
    legal_list = list(cfg.action_space)

    def loop():
        for g in loop_ids:
            gh = buffer.buffer[g]
            T = len(gh.root_values)
            result = engine.run(store.stacked(g), [legal_list] * T, gh.to_play_history[:T], False, rngs[:T])
            visits = result.visit_counts
            gh.child_visits = (visits / visits.sum(1, keepdims=True)).tolist()
            gh.root_values = result.root_values.tolist()
            buffer.update_game_history(g, gh)

    loop_ms = median_ms(loop, max(1, blocks // 2))
    sweep_rate, search_rate, loop_rate = total / sweep_ms * 1e3, n * repeats / search_ms * 1e3, loop_positions / loop_ms * 1e3
    return {
        "shape": name, "network": cfg.network, "trees": trees, "simulations": simulations, "games": len(lengths),
        "positions": total, "chunk_positions": min(trees, total), "chunks": report["chunks"], "skipped": report["skipped"],
        "search_kernel": kernel, "sweep_ms": round(sweep_ms, 3), "sweep_positions_per_s": round(sweep_rate, 1),
        "sweep_simulations_per_s": round(sweep_rate * simulations, 1), "search_positions_per_s": round(search_rate, 1),
        "sweep_share_of_search": round(sweep_rate / search_rate, 4), "loop_games": len(loop_ids),
        "loop_positions": loop_positions, "loop_ms": round(loop_ms, 3), "loop_positions_per_s": round(loop_rate, 1),
        "sweep_over_loop": round(sweep_rate / loop_rate, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanalyse_search_bench.log"))
    ap.add_argument("--quick", action="store_true", help="fewer timed blocks (a rehearsal)")
    ap.add_argument("--only", default=None, help="one shape by name")
    args = ap.parse_args()
    be = _lib.default_backend()
    blocks = 3 if args.quick else 5
    fields = dict(td_steps=10, num_unroll_steps=5, PER=False, PER_alpha=0.5, batch_size=128, replay_buffer_size=10 ** 6)
    rs = numpy.random.RandomState(4)
    legs = [
        # name, config, positions per game, frame dtype, trees, simulations, games of the host loop
        ("cartpole", configs.cartpole(**fields), [32] * 1024, numpy.float32, 4096, 50, 64),
        ("connect4", configs.connect4(**fields), [int(T) for T in rs.randint(7, 43, size=256)], numpy.int32, 1024, 200, 16),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        head = (f"# reanalyse_search_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; host clock, every timed block "
                f"ends in a device synchronise, medians of {blocks} blocks; sweep = DeviceGameStore.reanalyse_search over every "
                "resident game, search = mzx_search_run alone on one chunk's inputs, loop = stacked + BatchedMCTS.run + rebuild + "
                "update_game_history per game over the first loop_games games")
        print(head)
        log.write(head + "\n")
        for name, cfg, lengths, dtype, trees, simulations, loop_games in legs:
            if args.only and args.only != name:
                continue
            line = json.dumps(run(be, name, cfg, lengths, dtype, trees, simulations, loop_games, blocks))
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
