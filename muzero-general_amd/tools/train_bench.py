"""
One training step (Adam) of the shipped networks on the GPU, natively and through torch:

  torch_ms    the path before the native one: mzx.trainer.update_weights with the torch restatement of the network (the
              family's case module; residual networks in training mode) on the device -- torch's operators forward and
              backward, the fused loss head, torch Adam over the per-tensor parameters;
  native_ms   mzx.trainer.update_weights with a HipNetwork: mzx_train_fc_step / mzx_train_resnet_step, torch Adam on the
              flat parameter, for a residual network the statistics commit, refresh_derived;
  call_us     (fc) mzx_train_fc_step alone (mzx.trainer.train_fc_gradients: five launches), HIP events around a block.

    python muzero-general_amd/tools/train_bench.py --family fc|resnet|stem [--out FILE] [--quick] [--shape NAME]
    python muzero-general_amd/tools/train_bench.py --family chain [--out FILE] [--quick] [--shape NAME]   (whole steps: per-step loop
              with torch.optim.Adam | with mzx.optim.Adam | mzx.trainer.train_steps in chunks of 16; the optimizer launch alone)
    python muzero-general_amd/tools/train_bench.py --family fc --trace a|b|c --trace-steps N   (under rocprofv3 --kernel-trace --stats)
    python muzero-general_amd/tools/train_bench.py --family fc --launches DIR_N1 N1 DIR_N2 N2  (kernel dispatches per step from two traces)

  fc      CartPole's fully connected network, batch 128 x 11 steps                        -> profiles/fc_train_bench.log
  resnet  tic-tac-toe (64 x 21 steps) and connect4 (64 x 43 steps) as shipped             -> profiles/resnet_train_bench.log
  stem    the networks WITH a downsample stem, stem training on (config.train_downsample): breakout as shipped (16 x 6
          steps) and atari (256 channels x 16 blocks, 6 steps) at the largest power-of-two batch, up to its batch_size
          1024, whose scratch fits train_scratch_max_bytes                                -> profiles/resnet_stem_train_bench.log

The two legs run in one process and alternate block by block (host clock around calls that end in update_weights' one
download, i.e. a synchronise); medians over the blocks after a warm-up (fc: 9 blocks of 20; residual: 7 of 5, with the
minimum and maximum).  `launches` and `scratch_bytes` are what mzx_train_resnet_launches / _scratch_bytes report for the
native step.  A gain (either way) counts only beyond the larger of the two legs' spreads.  --trace runs one leg (a torch,
b native, c the call alone) for N steps and nothing else, so that two kernel traces of different N give the launches of
one step by difference (set-up launches cancel).
"""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "muzero-general_amd"), os.path.join(ROOT, "tests")]

FC_CASE = dict(name="cartpole_b128_k11", B=128, steps=11, obs=(1, 1, 4), stacked=0, enc=8, rep=[], dyn=[16], rew=[16], val=[16],
               pol=[16], A=2, S=10, per=True, alpha=0.5, vlw=0.25, seed=31)
FAMILIES = {      # shapes: name -> (batch, steps) as shipped; warm-up calls, (blocks, calls per block) full / --quick
    "fc": dict(cases="fc_train_cases", torch_net="FcNetwork", shapes={"cartpole": (128, 11)}, adam=dict(lr=0.02, weight_decay=1e-4),
               warm=3, blocks=(9, 20), quick=(3, 5), log="fc_train_bench.log",
               what="one training step of CartPole's network, batch 128 x 11 steps, Adam; torch_ms = update_weights with the torch "
                    "network, native_ms = update_weights with a HipNetwork (mzx_train_fc_step); medians of alternating timed "
                    "blocks, each call ends in one download; call_us = mzx_train_fc_step alone (events)"),
    "resnet": dict(cases="resnet_train_cases", torch_net="ResNetwork", shapes={"tictactoe": (64, 21), "connect4": (64, 43)},
                   adam=dict(lr=0.003, weight_decay=1e-4), warm=2, blocks=(7, 5), quick=(3, 2), log="resnet_train_bench.log",
                   what="one training step of the shipped residual networks, Adam; torch_ms = update_weights with the torch "
                        "network (training mode), native_ms = update_weights with a HipNetwork (mzx_train_resnet_step); medians "
                        "of alternating timed blocks [min, max], each call ends in one download"),
    "stem": dict(cases="resnet_stem_train_cases", torch_net="StemNetwork", shapes={"breakout": (16, 6), "atari": (1024, 6)},
                 adam=dict(lr=0.003, weight_decay=1e-4), warm=2, blocks=(7, 5), quick=(3, 2), log="resnet_stem_train_bench.log",
                 what="one training step of the shipped residual networks with a downsample stem, Adam; torch_ms = update_weights "
                      "with the torch network (training mode), native_ms = update_weights with a HipNetwork, stem training on "
                      "(mzx_train_resnet_step); medians of alternating timed blocks [min, max], each call ends in one download"),
    # whole training steps from a device replay store: (batch, unroll steps); see chain_measure / chain_optimizer_alone
    "chain": dict(shapes={"cartpole": (128, 10), "tictactoe": (64, 20), "connect4": (64, 42)}, adam=dict(lr=0.003, weight_decay=1e-4),
                  chunk=16, blocks=(7, 4), quick=(3, 1), log="train_chain_bench.log",
                  what="whole training steps (device sampler, gather, native step, Adam, priority feedback) in ms per step; "
                       "torch_adam = update_lr + train_step with torch.optim.Adam (the yardstick), native_adam = the same with "
                       "mzx.optim.Adam, chain = mzx.trainer.train_steps in chunks of 16; one process, legs alternate block by "
                       "block, medians of timed blocks [min, max], every block ends in ONE synchronise; then the optimizer launch "
                       "alone (HIP events) against torch's Adam over the same flat parameter"),
}


def shape_of(be, name):
    """(batch, steps) of a stem network: the shipped batch, halved until the native step's scratch fits train_scratch_max_bytes."""
    from mzx import configs, models, trainer

    B, steps = FAMILIES["stem"]["shapes"][name]
    probe = models.MuZeroNetwork(getattr(configs, name)(train_downsample=True), _backend=be)
    while B > 1:
        need = int(be.lib.mzx_train_resnet_scratch_bytes(probe.handle, B, steps))
        if 0 < need <= trainer.TRAIN_SCRATCH_MAX_BYTES:
            break
        B //= 2
    return B, steps


def legs(be, family, name):
    """({a: the torch step, b: the native step, c: the native gradient call alone}, the line's shape and extra keys)."""
    from mzx import configs, trainer

    fam = FAMILIES[family]
    cases = importlib.import_module(fam["cases"])
    if family == "fc":
        case, info = FC_CASE, {}
    else:
        B, steps = shape_of(be, name) if family == "stem" else fam["shapes"][name]
        case = cases.case_of_config(getattr(configs, name)(), B, steps, name=name)
    cfg = cases.config_of(case)
    batch = tuple(None if x is None else torch.from_numpy(x).to(be.device) for x in cases.batch(case))
    model = cases.load(getattr(cases, fam["torch_net"])(case), cases.weights(case)).to(be.device)
    if family != "fc":
        model.train()
    opt_torch = torch.optim.Adam(model.parameters(), **fam["adam"])
    net = cases.network(be, case)
    opt_native = torch.optim.Adam(net.parameters(), **fam["adam"])
    if family != "fc":
        info = dict(launches=int(be.lib.mzx_train_resnet_launches(net.handle, B, steps)),
                    scratch_bytes=int(be.lib.mzx_train_resnet_scratch_bytes(net.handle, B, steps)))
    gradients = trainer.train_fc_gradients if family == "fc" else trainer.train_resnet_gradients
    shape = case["name"] if family == "fc" else f"{name}_b{B}_k{steps}"
    return dict(a=lambda: trainer.update_weights(model, opt_torch, batch, cfg),
                b=lambda: trainer.update_weights(net, opt_native, batch, cfg),
                c=lambda: gradients(net, batch, cfg)), shape, info


def measure(be, family, name, quick):
    fam = FAMILIES[family]
    fns, shape, info = legs(be, family, name)
    blocks, iters = fam["quick"] if quick else fam["blocks"]
    times = dict(torch=[], native=[])
    for leg in "ab":
        for _ in range(fam["warm"]):
            fns[leg]()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for leg, ts in zip("ab", times.values()):
            t0 = time.perf_counter()
            for _ in range(iters):
                fns[leg]()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / iters)
    line = dict(shape=shape, optimizer="Adam")
    if family == "fc":
        line.update(torch_ms=round(statistics.median(times["torch"]), 4), native_ms=round(statistics.median(times["native"]), 4))
        line["torch_over_native"] = round(line["torch_ms"] / line["native_ms"], 2)
        fns["c"]()
        torch.cuda.synchronize()
        call = []
        for _ in range(blocks):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fns["c"]()
            stop.record()
            torch.cuda.synchronize()
            call.append(start.elapsed_time(stop) * 1e3 / iters)
        line["call_us"] = round(statistics.median(call), 2)
        return line
    line.update(blocks=blocks, steps_per_block=iters)
    for leg, ts in times.items():
        line[f"{leg}_ms"] = round(statistics.median(ts), 3)
        line[f"{leg}_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
    line["torch_over_native"] = round(line["torch_ms"] / line["native_ms"], 3)
    line.update(info)
    return line


def chain_setup(be, name, native):
    """(config, network, Adam, buffer with a device sampler) of a shipped configuration: 48 games of 8 .. 40 positions."""
    import numpy

    import replay_sampler_cases
    from mzx import configs, models, optim, replay, synthetic

    fam = FAMILIES["chain"]
    B, K = fam["shapes"][name]
    cfg = getattr(configs, name)(PER=True, PER_alpha=0.5, batch_size=B, num_unroll_steps=K, td_steps=10, discount=0.997, seed=7, value_loss_weight=0.25,
                                 replay_buffer_size=10 ** 6, lr_init=fam["adam"]["lr"], lr_decay_rate=0.9, lr_decay_steps=1000,
                                 weight_decay=fam["adam"]["weight_decay"], optimizer="Adam")
    rs = numpy.random.RandomState(5)
    lengths = [int(T) for T in rs.randint(8, 41, size=48)]
    store = replay.DeviceGameStore(cfg, be, sum(lengths) + len(lengths), max_games=64)
    buffer = replay.ReplayBuffer(dict(replay_sampler_cases.CHECKPOINT), {}, cfg, stock=replay_sampler_cases.FeedbackStock,
                                 device_store=store, device_sampler=True)
    for k, T in enumerate(lengths):
        buffer.save_game(replay_sampler_cases.game(cfg, T, 900 + k, priorities=0.1 + rs.random_sample(T)))
    net = models.MuZeroNetwork(cfg, _backend=be)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 11))
    make = optim.Adam if native else torch.optim.Adam
    return cfg, net, make(net.parameters(), **fam["adam"]), buffer


def chain_measure(be, name, quick):
    from mzx import trainer

    fam = FAMILIES["chain"]
    blocks, chunks = fam["quick"] if quick else fam["blocks"]
    chunk = fam["chunk"]
    setups = dict(torch_adam=chain_setup(be, name, False), native_adam=chain_setup(be, name, True), chain=chain_setup(be, name, True))
    at = dict.fromkeys(setups, 0)

    def block(leg):
        cfg, net, optimizer, buffer = setups[leg]
        for _ in range(chunks):
            if leg == "chain":
                trainer.train_steps(net, optimizer, buffer, cfg, chunk, at[leg])
            else:
                for i in range(chunk):
                    trainer.update_lr(optimizer, cfg, at[leg] + i)
                    trainer.train_step(net, optimizer, buffer, cfg)
            at[leg] += chunk

    times = {leg: [] for leg in setups}
    for leg in setups:
        block(leg)
    torch.cuda.synchronize()
    for _ in range(blocks):
        for leg, ts in times.items():
            t0 = time.perf_counter()
            block(leg)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / (chunks * chunk))
    B, K = fam["shapes"][name]
    line = dict(shape=f"{name}_b{B}_k{K}", optimizer="Adam", blocks=blocks, steps_per_block=chunks * chunk, chunk=chunk)
    for leg, ts in times.items():
        line[f"{leg}_ms"] = round(statistics.median(ts), 4)
        line[f"{leg}_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    line["torch_adam_over_chain"] = round(line["torch_adam_ms"] / line["chain_ms"], 3)
    line["torch_adam_over_native_adam"] = round(line["torch_adam_ms"] / line["native_adam_ms"], 3)
    flats = [setups[leg][1].flat_weights() for leg in ("native_adam", "chain")]
    line["chain_equals_native_adam_loop"] = bool(torch.equal(*flats))      # (the same steps from the same start: the same bits)
    return line


def chain_optimizer_alone(be, name, quick):
    """The optimizer launch alone over a shipped network's flat parameter: HIP events around runs of step() calls."""
    from mzx import configs, models, optim

    fam = FAMILIES["chain"]
    blocks, iters = (3, 20) if quick else (7, 100)
    net = models.MuZeroNetwork(getattr(configs, name)(), _backend=be)
    param = next(net.parameters())
    param.grad = torch.randn_like(net.flat_weights()) * 1e-3
    live = sum(count for _, count in optim.live_spans(net))
    line = dict(optimizer_alone=name, parameters=int(net.num_params), live=int(live))
    for leg, make in (("torch", torch.optim.Adam), ("native", optim.Adam)):
        optimizer = make(net.parameters(), **fam["adam"])
        for _ in range(3):
            optimizer.step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(blocks):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                optimizer.step()
            stop.record()
            torch.cuda.synchronize()
            ts.append(start.elapsed_time(stop) * 1e3 / iters)
        line[f"{leg}_us"] = round(statistics.median(ts), 2)
        line[f"{leg}_us_min_max"] = [round(min(ts), 2), round(max(ts), 2)]
    line["native_bytes_per_s"] = round(28 * live / (line["native_us"] * 1e-6), 0)
    line["native_fraction_of_8TBps"] = round(line["native_bytes_per_s"] / 8e12, 4)
    return line


def dispatches(directory):
    """{kernel name: calls} of a rocprofv3 --kernel-trace --stats output directory."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*_kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            out[r["Name"]] = out.get(r["Name"], 0) + int(r["Calls"])
    return out


def launches(dir1, n1, dir2, n2):
    d1, d2 = dispatches(dir1), dispatches(dir2)
    per_step = {k: (d2.get(k, 0) - d1.get(k, 0)) / (n2 - n1) for k in set(d1) | set(d2)}
    per_step = {k: v for k, v in per_step.items() if v}
    return dict(launches_per_step=round(sum(per_step.values()), 2), traces=[sum(d1.values()), sum(d2.values())], steps=[n1, n2],
                kernels={k[:100]: round(v, 2) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--shape", action="append")
    ap.add_argument("--trace", choices=["a", "b", "c"])
    ap.add_argument("--trace-steps", type=int, default=10)
    ap.add_argument("--launches", nargs=4, metavar=("DIR1", "N1", "DIR2", "N2"))
    args = ap.parse_args()
    fam = FAMILIES[args.family]
    names = args.shape or list(fam["shapes"])
    if set(names) - set(fam["shapes"]):
        ap.error(f"--shape of --family {args.family}: one of {sorted(fam['shapes'])}")
    if args.launches:
        print(json.dumps(launches(args.launches[0], int(args.launches[1]), args.launches[2], int(args.launches[3]))))
        return
    from mzx import _lib

    be = _lib.default_backend()
    if args.family == "chain" and args.trace:
        ap.error("--trace belongs to the step families")
    if args.trace:
        fn = legs(be, args.family, names[0])[0][args.trace]
        for _ in range(args.trace_steps):
            fn()
        torch.cuda.synchronize()
        return
    out = args.out or os.path.join(ROOT, "profiles", fam["log"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = [f"# {fam['log'][:-4]}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {fam['what']}"]
    print(lines[0], flush=True)
    if args.family == "chain":
        jobs = [(chain_measure, name) for name in names] + [(chain_optimizer_alone, name) for name in ("cartpole", "connect4", "atari")]
        for fn, name in jobs:
            lines.append(json.dumps(fn(be, name, args.quick)))
            print(lines[-1], flush=True)
            with open(out, "w") as log:
                log.write("\n".join(lines) + "\n")
        return
    for name in names:
        lines.append(json.dumps(measure(be, args.family, name, args.quick)))
        print(lines[-1], flush=True)
        with open(out, "w") as log:
            log.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
