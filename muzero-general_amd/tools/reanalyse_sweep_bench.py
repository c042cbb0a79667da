"""
Reanalyse over a device-resident replay store (mzx.replay.DeviceGameStore), on the GPU: the SWEEP
(DeviceGameStore.reanalyse: per chunk of positions mzx_replay_positions, the observation gather, one initial_inference,
mzx_replay_reanalyse_write; then one mzx_replay_values and one download) against the existing PER-GAME loop body
(Reanalyse.reanalyse_game + ReplayBuffer.update_game_history for every game: gather, network, decode, a blocking download,
an upload and a values launch per game) over the same games, in the same process, under the same weights.

    python muzero-general_amd/tools/reanalyse_sweep_bench.py [--out profiles/reanalyse_sweep_bench.log] [--quick]

Three geometries: CartPole (fully connected, 1024 games x 32 positions), connect4 (1024 games of 7 .. 42 positions) and
games/atari.py (3 x 96 x 96 frames, 32 stacked observations, the network as shipped; 8 games x 200 positions, the store of
tools/device_replay_bench.py).  Per geometry one JSON line (printed, and written to the log):
  sweep_ms, sweep_positions_per_s        one sweep over every resident game, default chunk (chunk_positions, chunks)
  loop_ms, loop_positions_per_s          the per-game loop over the same games
  sweep_over_loop                        ratio of the two rates
  network_ms                             initial_inference alone on one chunk's observations already in HBM, summed over the
                                         sweep's chunks (HIP events): what both paths spend in the network at best
  max_abs_difference                     largest |sweep - loop| decoded value (the paths batch the network differently)
Host clock around work that ends in a device synchronise (both paths end in a download); medians of timed blocks after
a warm-up, the two paths alternating block by block.  The stock buffer is a small stand-in so that the tool needs nothing outside the repository.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "muzero-general_amd"))
from mzx import _lib, configs, models, replay, self_play, synthetic  # noqa: E402


class Stock:
    """Storage of a replay buffer (what mzx.replay.ReplayBuffer composes with)."""

    def __init__(self, initial_checkpoint, initial_buffer, config):
        self.config, self.buffer = config, dict(initial_buffer)
        self.num_played_games = self.num_played_steps = self.total_samples = 0

    def save_game(self, game_history, shared_storage=None):
        self.buffer[self.num_played_games] = game_history
        self.num_played_games += 1
        self.num_played_steps += len(game_history.root_values)
        self.total_samples += len(game_history.root_values)

    def update_game_history(self, game_id, game_history):
        if next(iter(self.buffer)) <= game_id:
            self.buffer[game_id] = game_history


def make_games(cfg, lengths, dtype):
    rs = numpy.random.RandomState(0)
    shape, A, players = tuple(cfg.observation_shape), len(cfg.action_space), len(cfg.players)
    out = []
    for T in lengths:
        gh = self_play.GameHistory()
        gh.action_history = [0] + [int(a) for a in rs.randint(0, A, size=T)]
        gh.reward_history = [0] + [float(r) for r in rs.standard_normal(T)]
        gh.to_play_history = [i % players for i in range(T + 1)]
        gh.root_values = [float(v) for v in rs.standard_normal(T)]
        gh.child_visits = [[1 / A] * A for _ in range(T)]
        if numpy.issubdtype(dtype, numpy.integer):
            gh.observation_history = list(rs.randint(-1, 2, size=(T + 1,) + shape).astype(dtype))
        else:
            gh.observation_history = list(rs.rand(T + 1, *shape).astype(dtype))
        out.append(gh)
    return out


def host_clock(fns, blocks):
    """Median ms of each function: one warm-up call each, then timed blocks that ALTERNATE between them."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(blocks):
        for fn, row in zip(fns, times):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            row.append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(row) for row in times]


def run(be, name, cfg, lengths, dtype, quick):
    games = make_games(cfg, lengths, dtype)
    total = int(sum(lengths))
    store = replay.DeviceGameStore(cfg, be, total + len(lengths))
    buffer = replay.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, cfg, stock=Stock, device_store=store)
    for g in games:
        buffer.save_game(g)
    weights = synthetic.fill_state_dict(models.MuZeroNetwork(cfg).state_dict(), 0)
    worker = replay.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, cfg, device_store=store)
    swept = {}

    def sweep():
        swept.update(store.reanalyse(worker.model))

    looped = {}

    def loop():
        for game_id, gh in buffer.buffer.items():
            looped[game_id] = gh.reanalysed_predicted_root_values = worker.reanalyse_game(gh, game_id)
            buffer.update_game_history(game_id, gh)

    sweep_ms, loop_ms = host_clock((sweep, loop), 3 if quick else 7)
    worst = max(float(numpy.abs(swept[g] - looped[g].reshape(-1)).max()) for g in swept if len(swept[g]))
    # the network alone, per chunk of the sweep: observations already in HBM, HIP events
    chunk = min(store.reanalyse_chunk_positions(), total)
    sizes = [min(chunk, total - lo) for lo in range(0, total, chunk)]
    network_ms = 0.0
    for n in sorted(set(sizes)):
        obs = torch.rand((n,) + store.sample_shape, device=be.device)
        worker.model.initial_inference(obs)
        iters = 2 if quick else 5
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            worker.model.initial_inference(obs)
        stop.record()
        torch.cuda.synchronize()
        network_ms += start.elapsed_time(stop) / iters * sizes.count(n)
        del obs
    return {
        "geometry": name, "network": cfg.network, "observation_shape": list(cfg.observation_shape),
        "stacked_observations": cfg.stacked_observations, "games": len(lengths), "positions": total,
        "positions_per_game_min": int(min(lengths)), "positions_per_game_max": int(max(lengths)),
        "chunk_positions": chunk, "chunks": len(sizes),
        "sweep_ms": round(sweep_ms, 3), "sweep_positions_per_s": round(total / sweep_ms * 1e3, 1),
        "loop_ms": round(loop_ms, 3), "loop_positions_per_s": round(total / loop_ms * 1e3, 1),
        "sweep_over_loop": round(loop_ms / sweep_ms, 2), "network_ms": round(network_ms, 3),
        "max_abs_difference": worst,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanalyse_sweep_bench.log"))
    ap.add_argument("--quick", action="store_true", help="fewer timed blocks (a rehearsal)")
    ap.add_argument("--only", default=None, help="one geometry by name")
    args = ap.parse_args()
    be = _lib.default_backend()
    replay_fields = dict(td_steps=10, num_unroll_steps=5, PER=False, PER_alpha=0.5, batch_size=128, replay_buffer_size=10 ** 6)
    rs = numpy.random.RandomState(4)
    legs = [
        # name, config, positions per game, frame dtype
        ("cartpole", configs.cartpole(**replay_fields), [32] * 1024, numpy.float32),
        ("connect4", configs.connect4(**replay_fields), [int(T) for T in rs.randint(7, 43, size=1024)], numpy.int32),
        ("atari", configs.atari(**replay_fields), [200] * 8, numpy.float32),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        head = (f"# reanalyse_sweep_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; host clock incl. the final "
                f"download, medians of {3 if args.quick else 7} timed blocks that alternate between the two paths; sweep = DeviceGameStore.reanalyse over every resident game, loop = "
                "reanalyse_game + update_game_history per game (the existing worker's loop body) over the same games")
        print(head)
        log.write(head + "\n")
        for name, cfg, lengths, dtype in legs:
            if args.only and args.only != name:
                continue
            line = json.dumps(run(be, name, cfg, lengths, dtype, args.quick))
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
