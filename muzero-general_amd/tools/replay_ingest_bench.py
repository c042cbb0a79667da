"""
The hand-off of a shard's finished games into a device replay store (sampler and PER on), game by game and in bulk, on the
GPU, over the SAME synthetic ``ShardGames``: CartPole geometry (1 x 1 x 4, 2 actions) with 4096 games of mixed lengths,
Connect4 (3 x 6 x 7, 7 actions) with 1024 games, and the games/atari.py frame geometry (3 x 96 x 96, 18 actions) with 4 games.

    python muzero-general_amd/tools/replay_ingest_bench.py [--out profiles/replay_ingest_bench.log] [--quick]

Per shape one JSON line (printed, and written to the log):
  per_game_ms     ``for game in hand_off: buffer.save_game(game)``: the path every hand-off took before save_games existed
      (ReplayBuffer.save_game -> DeviceGameStore.add_many of one game).
  save_games_ms   ``buffer.save_games(hand_off)``: the stock bookkeeping and the row allocation per game, then one ingest.
  *_library_calls the mzx_replay_* calls one hand-off makes (values + sampler refresh per game; ingest per staged chunk);
      ingest_launches = 3 per ingest call.  The per-game path issues on top of its two calls six to eight uploads and a
      three-statement slot flush per game; the bulk path one upload per ingest call.
Host clock around a call that ends in a device synchronise; medians over timed blocks after a warm-up block.  Every block
gets a fresh buffer, store and set of views (built outside the clock; the records carry their priorities, as
``collect(priorities_for=...)`` leaves them).  The records are synthetic (``_ShardRecord`` + ``ShardGameHistory.make_many``)
and the stock buffer is a small stand-in, so the tool needs no self-play and nothing outside the repository.
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
from mzx import _lib, configs, replay  # noqa: E402
from mzx.history import ShardGameHistory, ShardGames, _ShardRecord  # noqa: E402


class Stock:
    """Storage and counters of a replay buffer (what mzx.replay.ReplayBuffer composes with)."""

    def __init__(self, initial_checkpoint, initial_buffer, config):
        self.config, self.buffer = config, dict(initial_buffer)
        self.num_played_games = self.num_played_steps = self.total_samples = 0

    def save_game(self, game_history, shared_storage=None):
        self.buffer[self.num_played_games] = game_history
        self.num_played_games += 1
        self.num_played_steps += len(game_history.root_values)
        self.total_samples += len(game_history.root_values)


SHAPES = {      # name -> (observation shape, actions, players, [(games, T), ...] one record each)
    "cartpole": ((1, 1, 4), 2, 1, [(256, T) for T in range(10, 42, 2)]),
    "connect4": ((3, 6, 7), 7, 2, [(128, T) for T in range(21, 43, 3)]),
    "atari": ((3, 96, 96), 18, 1, [(4, 200)]),
}


def make_config(shape, A, players):
    cfg = configs.cartpole(td_steps=10, num_unroll_steps=5, PER=True, PER_alpha=0.5, batch_size=128, replay_buffer_size=10 ** 6,
                           stacked_observations=0, seed=0)
    cfg.observation_shape, cfg.action_space, cfg.players = shape, list(range(A)), list(range(players))
    return cfg


def make_records(cfg, backend, lengths):
    shape, A, P = tuple(cfg.observation_shape), len(cfg.action_space), len(cfg.players)
    rs = numpy.random.RandomState(0)
    out = []
    for k, T in lengths:
        obs = rs.standard_normal((k, T + 1) + shape).astype(numpy.float32)
        acts = rs.randint(0, A, size=(k, T + 1)).astype(numpy.int64)
        rews = rs.standard_normal((k, T + 1))
        tps = numpy.tile((numpy.arange(T + 1) % P).astype(numpy.int64), (k, 1))
        vis = (rs.randint(0, 20, size=(k, T, A)) + 1).astype(numpy.int32)
        vals = rs.standard_normal((k, T))
        totals = vis.sum(2).astype(numpy.int64)
        record = _ShardRecord(A, obs, acts, rews, tps, vis, vals, totals, vis / totals[:, :, None], numpy.ones(k, bool), None)
        record.priorities, record.game_priority = replay.device_priorities(backend, vals, tps, rews, cfg)
        out.append((record, k, T))
    return out


def hand_off(records):
    """Fresh views of the records, interleaved as games that finish in turn, with the grouping ``collect`` attaches."""
    grouped, keyed = [], []
    for r, (record, k, T) in enumerate(records):
        record._lists = {}
        views = ShardGameHistory.make_many(record, k, T)
        grouped.append((record, T, views))
        keyed += [(j, r, h) for j, h in enumerate(views)]
    out = ShardGames([h for _, _, h in sorted(keyed, key=lambda e: e[:2])])
    out.records = grouped
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_ingest_bench.log"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    backend = _lib.default_backend()
    lib = backend.lib
    counts = {}
    for name in ("mzx_replay_values", "mzx_replay_sampler_refresh", "mzx_replay_ingest"):
        def counted(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a)
        setattr(lib, name, counted)
    blocks = 2 if args.quick else 5
    lines = []
    for shape_name, (shape, A, players, lengths) in SHAPES.items():
        cfg = make_config(shape, A, players)
        records = make_records(cfg, backend, lengths)
        games = sum(k for _, k, _ in records)
        rows = sum(k * (T + 1) for _, k, T in records)
        result = dict(shape=shape_name, games=games, pool_rows=rows, observation=list(shape), actions=A,
                      staged_mbytes=round(rows * (4 * int(numpy.prod(shape)) + 24 + 5 * A + 12) / 2 ** 20, 1))
        for mode in ("per_game", "save_games"):
            times = []
            for block in range(blocks + 1):
                store = replay.DeviceGameStore(cfg, backend, rows + 8, max_games=games)
                buffer = replay.ReplayBuffer({}, {}, cfg, stock=Stock, device_store=store)
                out = hand_off(records)
                counts.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "per_game":
                    for game_history in out:
                        buffer.save_game(game_history)
                else:
                    buffer.save_games(out)
                torch.cuda.synchronize()
                if block:
                    times.append((time.perf_counter() - t0) * 1e3)
                assert len(store) == games
            result[mode + "_ms"] = round(statistics.median(times), 3)
            result[mode + "_library_calls"] = sum(counts.values())
            if mode == "save_games":
                result["ingest_launches"] = 3 * counts.get("mzx_replay_ingest", 0)
        result["speedup"] = round(result["per_game_ms"] / result["save_games_ms"], 2)
        result["save_games_msteps_per_s"] = round((rows - games) / result["save_games_ms"] / 1e3, 3)
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# replay_ingest_bench: {torch.cuda.get_device_name(0)}, medians of {blocks} blocks\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
