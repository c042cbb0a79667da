"""
The hand-off of a resident shard's finished games into the device replay store, through the host (as it stands) and on the
device (config.device_handoff), in ONE process on one GPU.  The legs take turns block by block (so that clock and thermal
drift hit them alike); medians of the timed blocks after two warm-up blocks, min - max per leg, the host clock around
calls that end in a synchronise.  One JSON line per leg and one per comparison, printed and written behind a header line
to ``--out`` (default: profiles/device_handoff_bench.log).

  leg A   resident rounds + ``collect`` + ``save_games`` as they stand: the finished games are gathered on the device,
          downloaded, wrapped, staged in pinned memory, uploaded and ingested.  THE YARDSTICK of this run.
  leg B   the same with ``device_handoff``: the games are packed into a piece on the device and ingested from there.
  shapes  C2: the natively stepped synthetic game, 4096 games x 50 simulations, one group, chunk 16; Connect4Native,
          1024 games x 200 simulations.
  block   ``--rounds`` rounds (default 20; max_moves is cut to it on C2 so that every block finishes a shard of games),
          then collect, then save_games, then a synchronise.  Per block: end-to-end steps/s INCLUDING the hand-off, the
          seconds in rounds / collect / save, the bytes the rounds calls downloaded and the mzx_replay_* calls of the
          hand-off.

A gain is claimed only where the medians differ by more than the larger of the two legs' own (max - min) / median spreads;
otherwise the comparison says "inside the spread".  The stock buffer is a small stand-in (storage and counters), so the
tool needs nothing outside the repository.

    python muzero-general_amd/tools/device_handoff_bench.py [--blocks 7] [--rounds 20] [--games 4096] [--sims 50]
                                                            [--c4-games 1024] [--c4-sims 200] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mzx import configs, games, models, replay, self_play, synthetic  # noqa: E402

REPLAY_CALLS = ("mzx_replay_ingest", "mzx_replay_priorities", "mzx_replay_values", "mzx_replay_sampler_refresh", "mzx_replay_export")


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


def summary(values):
    med = statistics.median(values)
    return dict(median=med, min=min(values), max=max(values), spread=(max(values) - min(values)) / med if med else 0.0)


def compare(name, base, leg):
    a, b = base["steps_per_s"], leg["steps_per_s"]
    ratio = b["median"] / a["median"]
    beyond = abs(ratio - 1.0) > max(a["spread"], b["spread"])
    return dict(comparison=name, ratio=round(ratio, 4), larger_spread=round(max(a["spread"], b["spread"]), 4),
                verdict=("faster" if ratio > 1 else "slower") if beyond else "inside the spread")


class Leg:
    def __init__(self, name, cfg, Game, net, B, rounds, blocks, counts, cut, **flags):
        c = copy.copy(cfg)
        if cut:
            c.max_moves = min(int(c.max_moves), rounds)
        c.device_draws, c.device_games = True, True
        c.PER, c.PER_alpha, c.td_steps, c.num_unroll_steps, c.batch_size, c.replay_buffer_size = True, 0.5, 10, 5, 128, 10 ** 9
        for k, v in flags.items():
            setattr(c, k, v)
        self.name, self.B, self.rounds, self.counts = name, B, rounds, counts
        self.sp = self_play.SelfPlay({"weights": net.get_weights()}, Game, c, 0, num_games=B, _backend=net.backend)
        rows = (blocks + 3) * B * rounds * 2 + 64          # every block's games stay resident: nothing is evicted on the clock
        store = replay.DeviceGameStore(c, net.backend, rows, max_games=(blocks + 3) * B * max(1, rounds))
        self.buffer = replay.ReplayBuffer({}, {}, c, stock=Stock, device_store=store, device_sampler=True)
        self.rows = []

    def block(self, timed):
        sp, shard = self.sp, None
        before = sp.stats["searches"]
        down0 = (sp.stats.get("resident") or [0] * 8)[4]
        self.counts.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        shard = sp._native_shard(1.0)
        upto = shard.rounds(1.0, None, 1 << 60, self.rounds)
        t1 = time.perf_counter()
        out, _ = shard.collect(upto, priorities_for=sp.config)
        t2 = time.perf_counter()
        self.buffer.save_games(out)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if timed:
            self.rows.append(dict(rate=(sp.stats["searches"] - before) / (t3 - t0), rounds=t1 - t0, collect=t2 - t1, save=t3 - t2,
                                  games=len(out), downloaded=sp.stats["resident"][4] - down0, calls=sum(self.counts.values())))

    def result(self):
        med = lambda key: statistics.median(r[key] for r in self.rows)
        out = dict(leg=self.name, games=self.B, rounds_per_block=self.rounds, slot_groups=len(self.sp._live["groups"]),
                   steps_per_s=summary([r["rate"] for r in self.rows]),
                   ms_per_block=dict(rounds=round(1e3 * med("rounds"), 3), collect=round(1e3 * med("collect"), 3),
                                     save=round(1e3 * med("save"), 3)),
                   games_per_hand_off=med("games"), bytes_downloaded_per_hand_off=int(med("downloaded")),
                   replay_calls_per_hand_off=med("calls"), bytes_in_pieces=self.sp.stats["resident"][7],
                   ingest_calls=self.buffer.device_store.ingest_calls)
        self.sp.close_game()
        return out


def run_legs(legs, blocks, emit):
    for _ in range(2):              # warm-up: allocations, kernel attributes, the first chunks, the first piece buffers
        for leg in legs:
            leg.block(False)
    for _ in range(blocks):
        for leg in legs:
            leg.block(True)
    results = [leg.result() for leg in legs]
    for r in results:
        emit(r)
    return {r["leg"]: r for r in results}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--c4-games", type=int, default=1024)
    ap.add_argument("--c4-sims", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_handoff_bench.log"))
    args = ap.parse_args()
    log = open(args.out, "w")
    log.write(f"# device_handoff_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one process, legs alternate block "
              f"by block, medians of {args.blocks} timed blocks after two warm-up blocks, host clock around calls that end in a "
              f"synchronise; the yardstick of every comparison is the host hand-off leg of this run\n")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    cfg = configs.cartpole(num_simulations=args.sims)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 0))
    lib, counts = net.backend.lib, {}
    for name in REPLAY_CALLS:
        def counted(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a)
        setattr(lib, name, counted)
    Game = games.make_native_synthetic_game(cfg.observation_shape, len(cfg.action_space), len(cfg.players))
    one = dict(self_play_pipeline=False, device_games_chunk=16)
    c2 = run_legs([
        Leg("c2 host hand-off", cfg, Game, net, args.games, args.rounds, args.blocks, counts, True, **one),
        Leg("c2 device hand-off", cfg, Game, net, args.games, args.rounds, args.blocks, counts, True, device_handoff=True, **one),
    ], args.blocks, emit)
    emit(compare("c2 device hand-off / c2 host hand-off", c2["c2 host hand-off"], c2["c2 device hand-off"]))
    cfg4 = configs.connect4(num_simulations=args.c4_sims)
    net4 = models.MuZeroNetwork(cfg4)
    net4.set_weights(synthetic.fill_state_dict(net4.state_dict(), 0))
    c4 = run_legs([
        Leg("connect4 host hand-off", cfg4, games.Connect4Native, net4, args.c4_games, args.rounds, args.blocks, counts, False,
            device_games_chunk=16),
        Leg("connect4 device hand-off", cfg4, games.Connect4Native, net4, args.c4_games, args.rounds, args.blocks, counts, False,
            device_games_chunk=16, device_handoff=True),
    ], args.blocks, emit)
    emit(compare("connect4 device hand-off / connect4 host hand-off", c4["connect4 host hand-off"], c4["connect4 device hand-off"]))
    log.close()


if __name__ == "__main__":
    main()
