"""
The loss head of a training step -- forward plus backward() of the loss part only, logits as leaf tensors -- on the GPU:

  (a) torch_ms   the reference's statements trainer.py:161-258 restated with torch operators on the device
                 (tests/trainer_loss_cases.torch_loss_head), INCLUDING its K + 1 blocking downloads for the priorities;
  (b) fused_ms   mzx.trainer.muzero_loss plus ONE download of the priorities.

    python muzero-general_amd/tools/trainer_loss_bench.py [--out profiles/trainer_loss_bench.log] [--quick] [--only-fused]

Both legs run in one process in alternating timed blocks (host clock around work that ends in a download, i.e. a
synchronise); medians over the blocks after a warm-up.  kernel_us is mzx_trainer_loss alone (HIP events around a block of
calls, both launches), kernel_GBps its logits read once + gradients written once: 2 * 4 * (K + 1) * B * (2 W + A) bytes.
--only-fused runs leg (b) alone (for a kernel trace).
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
import trainer_loss_cases as cases  # noqa: E402
from mzx import _lib, trainer  # noqa: E402

SHAPES = [dict(name="cartpole", B=128, steps=11, S=10, A=2), dict(name="connect4", B=1024, steps=6, S=10, A=7),
          dict(name="atari", B=1024, steps=6, S=300, A=18)]


def run(be, shape, quick, only_fused):
    case = dict(shape, per=True, alpha=0.5, vlw=0.25, seed=1)
    cfg = cases.config_of(case)
    x = {k: None if v is None else torch.from_numpy(v).to(be.device) for k, v in cases.inputs(case).items()}
    leaf = lambda a: [s.clone().requires_grad_() for s in a]

    def torch_leg():
        v, r, p = leaf(x["value"]), leaf(x["reward"]), leaf(x["policy"])
        loss, _, _, _, priorities = cases.torch_loss_head(v, r, p, x["target_value"], x["target_reward"], x["target_policy"],
                                                          x["weight"], x["gradient_scale"], cfg, download=True)
        loss.backward()
        return priorities

    def fused_leg():
        v, r, p = leaf(x["value"]), leaf(x["reward"]), leaf(x["policy"])
        loss, _, _, _, priorities = trainer.muzero_loss(v, r, p, x["target_value"], x["target_reward"], x["target_policy"],
                                                        x["weight"], x["gradient_scale"], cfg)
        loss.backward()
        return priorities.cpu().numpy()

    legs = [("fused_ms", fused_leg)] if only_fused else [("torch_ms", torch_leg), ("fused_ms", fused_leg)]
    blocks, iters = (3, 5) if quick else (9, 20)
    times = {name: [] for name, _ in legs}
    for name, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name, fn in legs:
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / iters)
    line = dict(shape, **{name: round(statistics.median(t), 4) for name, t in times.items()})
    if not only_fused:
        line["torch_over_fused"] = round(line["torch_ms"] / line["fused_ms"], 2)
    # the library call alone
    args = (be, x["value"], x["reward"], x["policy"], x["target_value"], x["target_reward"], x["target_policy"], x["weight"],
            x["gradient_scale"], case["S"], case["vlw"], case["alpha"], True)
    trainer._run(*args)
    torch.cuda.synchronize()
    kernel = []
    for _ in range(blocks):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            trainer._run(*args)
        stop.record()
        torch.cuda.synchronize()
        kernel.append(start.elapsed_time(stop) * 1e3 / iters)
    W = 2 * case["S"] + 1
    moved = 2 * 4 * case["steps"] * case["B"] * (2 * W + case["A"])
    us = statistics.median(kernel)
    line.update(call_us=round(us, 2), bytes=moved, call_GBps=round(moved / us / 1e3, 1), frac_of_8TBps=round(moved / us / 1e3 / 8000, 4))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_loss_bench.log"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    be = _lib.default_backend()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        head = (f"# trainer_loss_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; loss head forward + backward, "
                "logits as leaves; torch_ms = torch operators with K + 1 blocking downloads, fused_ms = mzx.trainer.muzero_loss + "
                "one download; medians of alternating timed blocks; call_us = mzx_trainer_loss alone (events; includes the "
                "allocation of its outputs)")
        print(head)
        log.write(head + "\n")
        for shape in SHAPES:
            line = json.dumps(run(be, shape, args.quick, args.only_fused))
            print(line, flush=True)
            log.write(line + "\n")


if __name__ == "__main__":
    main()
