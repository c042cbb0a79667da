"""
One training step of CartPole's fully connected network (batch 128, 11 steps, Adam) on the GPU:

  (a) torch_ms    the path before the native one: mzx.trainer.update_weights with the torch restatement of the network
                  (tests/fc_train_cases.FcNetwork) on the device -- torch's per-layer operators forward and backward, the
                  fused loss head, torch Adam over the per-tensor parameters;
  (b) native_ms   mzx.trainer.update_weights with a HipNetwork: mzx_train_fc_step, torch Adam on the flat parameter,
                  refresh_derived;
  (c) call_us     mzx_train_fc_step alone (mzx.trainer.train_fc_gradients: five launches), HIP events around a block.

    python muzero-general_amd/tools/fc_train_bench.py [--out profiles/fc_train_bench.log] [--quick]
    python muzero-general_amd/tools/fc_train_bench.py --trace a|b|c --trace-steps N     (under rocprofv3 --kernel-trace --stats)
    python muzero-general_amd/tools/fc_train_bench.py --launches DIR_N1 N1 DIR_N2 N2    (kernel dispatches per step from two traces)

(a) and (b) run in one process in alternating timed blocks (host clock around calls that end in update_weights' one
download, i.e. a synchronise); medians over the blocks after a warm-up.  --trace runs one leg for N steps and nothing else,
so that two kernel traces of different N give the launches of one step by difference (set-up launches cancel).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "muzero-general_amd"), os.path.join(ROOT, "tests")]

CASE = dict(name="cartpole_b128_k11", B=128, steps=11, obs=(1, 1, 4), stacked=0, enc=8, rep=[], dyn=[16], rew=[16], val=[16],
            pol=[16], A=2, S=10, per=True, alpha=0.5, vlw=0.25, seed=31)
ADAM = dict(lr=0.02, weight_decay=1e-4)


def legs(be):
    import fc_train_cases as cases
    from mzx import trainer

    cfg = cases.config_of(CASE)
    host = cases.batch(CASE)
    batch = tuple(None if x is None else torch.from_numpy(x).to(be.device) for x in host)
    model = cases.load(cases.FcNetwork(CASE), cases.weights(CASE)).to(be.device)
    opt_torch = torch.optim.Adam(model.parameters(), **ADAM)
    net = cases.network(be, CASE)
    opt_native = torch.optim.Adam(net.parameters(), **ADAM)
    return dict(a=lambda: trainer.update_weights(model, opt_torch, batch, cfg),
                b=lambda: trainer.update_weights(net, opt_native, batch, cfg),
                c=lambda: trainer.train_fc_gradients(net, batch, cfg))


def measure(be, quick):
    fns = legs(be)
    blocks, iters = (3, 5) if quick else (9, 20)
    times = dict(a=[], b=[])
    for name in times:
        for _ in range(3):
            fns[name]()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name in times:
            t0 = time.perf_counter()
            for _ in range(iters):
                fns[name]()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / iters)
    line = dict(shape=CASE["name"], optimizer="Adam", torch_ms=round(statistics.median(times["a"]), 4),
                native_ms=round(statistics.median(times["b"]), 4))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_train_bench.log"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--trace", choices=["a", "b", "c"])
    ap.add_argument("--trace-steps", type=int, default=10)
    ap.add_argument("--launches", nargs=4, metavar=("DIR1", "N1", "DIR2", "N2"))
    args = ap.parse_args()
    if args.launches:
        print(json.dumps(launches(args.launches[0], int(args.launches[1]), args.launches[2], int(args.launches[3]))))
        return
    from mzx import _lib

    be = _lib.default_backend()
    if args.trace:
        fn = legs(be)[args.trace]
        for _ in range(args.trace_steps):
            fn()
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = (f"# fc_train_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one training step of CartPole's "
            "network, batch 128 x 11 steps, Adam; torch_ms = update_weights with the torch network, native_ms = update_weights "
            "with a HipNetwork (mzx_train_fc_step); medians of alternating timed blocks, each call ends in one download; "
            "call_us = mzx_train_fc_step alone (events)")
    line = json.dumps(measure(be, args.quick))
    print(head + "\n" + line)
    with open(args.out, "w") as log:
        log.write(head + "\n" + line + "\n")


if __name__ == "__main__":
    main()
