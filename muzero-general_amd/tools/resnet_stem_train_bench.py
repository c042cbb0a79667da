"""
One training step (Adam) of the two shipped residual networks WITH a downsample stem on the GPU:

  breakout  games/breakout.py as shipped: batch_size 16 x (num_unroll_steps 5 + 1) steps;
  atari     games/atari.py as shipped (256 channels x 16 blocks, 73.5 M parameters), num_unroll_steps 5 + 1 steps, at the
            largest power-of-two batch (up to its batch_size 1024) whose scratch fits train_scratch_max_bytes.

  torch_ms    the path before the native one: mzx.trainer.update_weights with the torch restatement of the network
              (tests/resnet_stem_train_cases.StemNetwork, training mode) on the device;
  native_ms   mzx.trainer.update_weights with a HipNetwork whose stem training is switched on
              (config.train_downsample = True): mzx_train_resnet_step, torch Adam on the flat parameter, the statistics
              commit, refresh_derived.

    python muzero-general_amd/tools/resnet_stem_train_bench.py [--out profiles/resnet_stem_train_bench.log] [--quick] [--shape NAME]

Both legs run in one process and alternate block by block; medians of 7 blocks after a warm-up, with the minimum and
maximum.  `launches` and `scratch_bytes` are what mzx_train_resnet_launches / _scratch_bytes report for the native step.
A gain (either way) counts only beyond the larger of the two legs' spreads.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "muzero-general_amd"), os.path.join(ROOT, "tests")]

SHIPPED = {"breakout": (16, 6), "atari": (1024, 6)}      # batch_size, num_unroll_steps + 1 of the game files
ADAM = dict(lr=0.003, weight_decay=1e-4)


def shape_of(be, name):
    """(batch, steps): the shipped batch, halved until the native step's scratch fits train_scratch_max_bytes."""
    from mzx import configs, models, trainer

    B, steps = SHIPPED[name]
    probe = models.MuZeroNetwork(getattr(configs, name)(train_downsample=True), _backend=be)
    while B > 1:
        need = int(be.lib.mzx_train_resnet_scratch_bytes(probe.handle, B, steps))
        if 0 < need <= trainer.TRAIN_SCRATCH_MAX_BYTES:
            break
        B //= 2
    return B, steps


def legs(be, name, B, steps):
    import resnet_stem_train_cases as cases
    from mzx import configs, trainer

    case = cases.case_of_config(getattr(configs, name)(), B, steps, name=name)
    cfg = cases.config_of(case)
    batch = tuple(None if x is None else torch.from_numpy(x).to(be.device) for x in cases.batch(case))
    state = cases.weights(case)
    model = cases.load(cases.StemNetwork(case), state).to(be.device).train()
    opt_torch = torch.optim.Adam(model.parameters(), **ADAM)
    net = cases.network(be, case)
    opt_native = torch.optim.Adam(net.parameters(), **ADAM)
    info = dict(launches=int(be.lib.mzx_train_resnet_launches(net.handle, B, steps)),
                scratch_bytes=int(be.lib.mzx_train_resnet_scratch_bytes(net.handle, B, steps)))
    return dict(torch=lambda: trainer.update_weights(model, opt_torch, batch, cfg),
                native=lambda: trainer.update_weights(net, opt_native, batch, cfg)), info


def measure(be, name, quick):
    B, steps = shape_of(be, name)
    fns, info = legs(be, name, B, steps)
    blocks, iters = (3, 2) if quick else (7, 5)
    times = dict(torch=[], native=[])
    for leg in times:
        for _ in range(2):
            fns[leg]()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for leg in times:
            t0 = time.perf_counter()
            for _ in range(iters):
                fns[leg]()
            torch.cuda.synchronize()
            times[leg].append((time.perf_counter() - t0) * 1e3 / iters)
    line = dict(shape=f"{name}_b{B}_k{steps}", optimizer="Adam", blocks=blocks, steps_per_block=iters)
    for leg, ts in times.items():
        line[f"{leg}_ms"] = round(statistics.median(ts), 3)
        line[f"{leg}_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
    line["torch_over_native"] = round(line["torch_ms"] / line["native_ms"], 3)
    line.update(info)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_stem_train_bench.log"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--shape", choices=sorted(SHIPPED), action="append")
    args = ap.parse_args()
    from mzx import _lib

    be = _lib.default_backend()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = (f"# resnet_stem_train_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one training step of the "
            "shipped residual networks with a downsample stem, Adam; torch_ms = update_weights with the torch network (training "
            "mode), native_ms = update_weights with a HipNetwork, stem training on (mzx_train_resnet_step); medians of "
            "alternating timed blocks [min, max], each call ends in one download")
    lines = [head]
    print(head, flush=True)
    for name in args.shape or ["breakout", "atari"]:
        lines.append(json.dumps(measure(be, name, args.quick)))
        print(lines[-1], flush=True)
        with open(args.out, "w") as log:
            log.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
