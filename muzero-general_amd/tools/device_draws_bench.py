"""
Self-play draws on the device (config.device_draws; csrc/mzx_draws.h) against the host streams, in ONE process on one GPU:
medians of repeated timed blocks, the host clock around calls that end in a synchronise.  Three legs, one JSON line each:

  (a) native rounds     C2's natively stepped shard (4096 games x 50 simulations), SelfPlay.play_rounds = one
                        mzx_selfplay_rounds call per block: steps/s and the library's phase_seconds (ms per block), host
                        draws and device draws.
  (b) continued search  BatchedMCTS.continue_search wall time per call at 4096 x 50 (the old roots searched again), rngs =
                        4096 numpy RandomState objects against rngs=None.
  (c) launches alone    mzx_selfplay_draws and mzx_selfplay_select_device on their own (HIP events around one launch), at
                        C2's shape and at the widest action space the entries take (256 games x 4096 actions).

Every comparison is host draws against device draws of this run; "spread" is (max - min) / median of a leg's own blocks, and
"faster_beyond_spread" says whether the device leg's gain exceeds both spreads.  The lines are printed and written, behind
a header line, to ``--out`` (default: profiles/device_draws_bench.log of this tree).

    python muzero-general_amd/tools/device_draws_bench.py [--blocks 7] [--rounds 20] [--games 4096] [--sims 50] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mzx import configs, draws, games, models, self_play, synthetic  # noqa: E402


def summary(values):
    med = statistics.median(values)
    return dict(median=med, min=min(values), max=max(values), spread=(max(values) - min(values)) / med if med else 0.0)


def verdict(host, device, smaller_is_better):
    gain = (host["median"] / device["median"]) if smaller_is_better else (device["median"] / host["median"])
    return dict(device_over_host=round(gain, 4), faster_beyond_spread=bool(gain - 1.0 > max(host["spread"], device["spread"])))


def native_rounds_leg(cfg, net, B, rounds, blocks, device_draws):
    c = copy.copy(cfg)
    c.max_moves, c.device_draws = rounds, device_draws
    Game = games.make_native_synthetic_game(c.observation_shape, len(c.action_space), len(c.players))
    sp = self_play.SelfPlay({"weights": net.get_weights()}, Game, c, 0, num_games=B, _backend=net.backend)
    sp.play_rounds(1.0, None, min_games=1 << 60, max_rounds=2)          # warm-up: allocations, kernel attributes
    rates, phases = [], []
    for _ in range(blocks):
        sp.stats = {"searches": 0, "simulations": 0, "search_seconds": 0.0}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp.play_rounds(1.0, None, min_games=1 << 60, max_rounds=rounds)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rates.append(sp.stats["searches"] / wall)
        phases.append([1e3 * x for x in sp.stats["native_phase_seconds"]])
    groups = len(sp._live["groups"])
    sp.close_game()
    return dict(steps_per_s=summary(rates), slot_groups=groups,
                phase_ms_per_block=[round(statistics.median(p[k] for p in phases), 3) for k in range(7)])


def continue_leg(cfg, net, B, blocks, device_draws):
    S = cfg.num_simulations
    engine = self_play.BatchedMCTS(cfg, net, B, max_carried_nodes=S + 1, device_draws=device_draws)
    obs = synthetic.observations(B, net.input_shape, seed=1)
    legal = [list(cfg.action_space)] * B
    rngs = None if device_draws else [numpy.random.RandomState(7 + i) for i in range(B)]
    again = [-1] * B
    times = []
    for k in range(blocks + 1):          # (the first block warms up); a fresh search, untimed, then the continued one
        engine.run(list(obs), legal, [0] * B, True, rngs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.continue_search(again, [0] * B, True, rngs)
        torch.cuda.synchronize()
        if k:
            times.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_per_call=summary(times), sims_per_s=B * S / (1e-3 * statistics.median(times)))


def launches_leg(net, B, A, blocks, alpha, sims):
    be = net.backend
    legal = numpy.tile(numpy.arange(A, dtype=numpy.int32), (B, 1))
    visits = numpy.random.RandomState(1).multinomial(sims, [1.0 / A] * A, size=B).astype(numpy.int32)
    t_legal, t_visits = torch.as_tensor(legal).to(be.device), torch.as_tensor(visits).to(be.device)
    table, tt = draws.power_table([1.0], sims + 2)
    t_table, t_tt = torch.as_tensor(table).to(be.device), torch.as_tensor(tt).to(be.device)
    t_temps = torch.ones(B, dtype=torch.float64, device=be.device)
    out = {}
    for name, fn in (("draws_us", lambda k: draws.root_draws(be, 1, k, B, A, self_play.TAPE_WORDS, alpha=alpha, legal=t_legal)),
                     ("select_us", lambda k: draws.select(be, 1, k, t_legal, t_visits, t_temps, t_table, t_tt))):
        fn(0)
        times = []
        for k in range(blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn(k + 1)
            e1.record()
            torch.cuda.synchronize()
            times.append(1e3 * e0.elapsed_time(e1))
        out[name] = summary(times)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_draws_bench.log"))
    args = ap.parse_args()
    B = args.games
    log = open(args.out, "w")
    log.write(f"# device_draws_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one process, medians of "
              f"{args.blocks} timed blocks per leg, host clock around calls that end in a synchronise; host draws against device "
              f"draws of this run\n")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()
    cfg = configs.cartpole(num_simulations=args.sims)
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 0))
    host = native_rounds_leg(cfg, net, B, args.rounds, args.blocks, False)
    device = native_rounds_leg(cfg, net, B, args.rounds, args.blocks, True)
    emit(dict(leg="a native rounds", games=B, sims=args.sims, rounds_per_block=args.rounds, host_draws=host,
              device_draws=device, **verdict(host["steps_per_s"], device["steps_per_s"], False)))
    host = continue_leg(cfg, net, B, args.blocks, False)
    device = continue_leg(cfg, net, B, args.blocks, True)
    emit(dict(leg="b continue_search", trees=B, sims=args.sims, host_draws=host, device_draws=device,
              **verdict(host["ms_per_call"], device["ms_per_call"], True)))
    emit(dict(leg="c launches alone", games=B, actions=len(cfg.action_space), tape_words=self_play.TAPE_WORDS,
              **launches_leg(net, B, len(cfg.action_space), args.blocks, cfg.root_dirichlet_alpha, args.sims)))
    emit(dict(leg="c launches alone, widest action space", games=256, actions=draws.MAX_ACTIONS, tape_words=self_play.TAPE_WORDS,
              **launches_leg(net, 256, draws.MAX_ACTIONS, args.blocks, cfg.root_dirichlet_alpha, args.sims)))
    log.close()


if __name__ == "__main__":
    main()
