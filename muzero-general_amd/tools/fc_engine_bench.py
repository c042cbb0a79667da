"""
A/B of the streamed engine for fully connected networks (net.fc_engine = "streamed", csrc/mzx_fc_streamed.hip) against the
per-operator path of the SAME handle in the SAME process (the yardstick), written to profiles/fc_engine_bench.log:

  * recurrent_inference at 4096 rows, hidden widths 64 / 256 / 512 (one hidden layer per MLP, 18 actions);
  * a search of 4096 trees x 50 simulations at width 256 (the row route around the engine against the per-operator path).

Legs alternate block by block; every figure is the median of 7 timed blocks with [min, max] (one warm-up block per leg is
dropped), timed with events on the stream.  The engine legs also report FLOP/s against the 157.3 TFLOP/s FP32 matrix peak
(mzx_net_flops: multiply-adds of the Linear layers only).  A gain is claimed only beyond the larger of the two legs' spreads.

    python muzero-general_amd/tools/fc_engine_bench.py [--blocks 7] [--calls 20]
"""
import argparse
import os
import statistics
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "muzero-general_amd"))
from mzx import configs, models, self_play  # noqa: E402

PEAK = 157.3e12
ENGINES = ("ops", "streamed")


def config(width, **kw):
    layers = {f"fc_{k}_layers": [width] for k in ("representation", "dynamics", "reward", "value", "policy")}
    return configs.cartpole(action_space=list(range(18)), **layers, **kw)


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def alternate(net, legs, blocks, calls):
    """ms per call of every leg: blocks + 1 rounds over the legs in turn, the first round dropped."""
    ms = {e: [] for e in ENGINES}
    for b in range(blocks + 1):
        for e in ENGINES:
            net.fc_engine = e
            t = timed(legs[e], calls)
            if b:
                ms[e].append(t)
    return ms


def report(out, label, ms, flops=None):
    med = {e: statistics.median(v) for e, v in ms.items()}
    spread = max(max(v) - min(v) for v in ms.values())
    for e in ENGINES:
        extra = ""
        if flops and e == "streamed":
            rate = flops / (med[e] * 1e-3)
            extra = f"  {rate / 1e12:.2f} TFLOP/s = {rate / PEAK:.3f} of the FP32 matrix peak"
        out.append(f"{label:<34} {e:<9} {med[e]:9.4f} ms [{min(ms[e]):.4f}, {max(ms[e]):.4f}]{extra}")
    gain = med["ops"] - med["streamed"]
    verdict = f"{med['ops'] / med['streamed']:.2f}x" if gain > spread else "no gain beyond the spread"
    out.append(f"{label:<34} ops - streamed = {gain:.4f} ms, larger spread {spread:.4f} ms: {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = [f"fc_engine_bench: {torch.cuda.get_device_name(0)}, {args.blocks} timed blocks per leg, legs alternating"]
    B = 4096
    for width in (64, 256, 512):
        torch.manual_seed(width)
        net = models.MuZeroNetwork(config(width))
        hidden = net.initial_inference(torch.rand(B, net.input_size))[3]
        act = (torch.arange(B) % 18).to(hidden.device)
        legs = {e: (lambda: net.recurrent_inference(hidden, act)) for e in ENGINES}
        flops = B * net.backend.lib.mzx_net_flops(net.handle, 1)
        report(out, f"recurrent_inference {B} x width {width}", alternate(net, legs, args.blocks, args.calls), flops)
    cfg = config(256, num_simulations=50)
    torch.manual_seed(1)
    net = models.MuZeroNetwork(cfg)
    obs = list(numpy.random.RandomState(0).rand(B, *cfg.observation_shape).astype(numpy.float32))
    legal = [list(cfg.action_space)] * B
    engines = {}
    for e in ENGINES:      # (a search engine per leg: the route is decided per handle and per call, the arenas are separate)
        net.fc_engine = e
        engines[e] = self_play.BatchedMCTS(cfg, net, B)
    legs = {e: (lambda e=e: engines[e].run(obs, legal, [0] * B, True, [numpy.random.RandomState(i) for i in range(B)]))
            for e in ENGINES}
    ms = alternate(net, legs, args.blocks, 1)
    report(out, f"search {B} x 50 at width 256 (host incl.)", ms)
    for e in ENGINES:
        out.append(f"  {e}: {engines[e].kernel_name(B)}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "fc_engine_bench.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
