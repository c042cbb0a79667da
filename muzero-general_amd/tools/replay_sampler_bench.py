"""
ReplayBuffer.get_batch and the priority feedback with and without the device-side sampler (mzx_replay_sample,
mzx_replay_update_priorities), on the GPU, at three shapes: CartPole (1 x 1 x 4) at batch 128, Connect4 (3 x 6 x 7) at batch
1024 and the games/atari.py geometry (3 x 96 x 96 frames, 32 stacked observations) at batch 1024.

    python muzero-general_amd/tools/replay_sampler_bench.py [--out profiles/replay_sampler_bench.log] [--quick]

Per shape one JSON line (printed, and written to the log):
  host_draw_get_batch_ms   get_batch of ReplayBuffer(device_store=...): the draws are numpy's, per sample, on the host; the
      gather runs on the device.  Host clock around a call that ends in a device synchronise.
  sampler_get_batch_ms     get_batch of ReplayBuffer(device_store=..., device_sampler=True), same clock.
  sampler_device_ms        the launches of that call alone (draw + gather), HIP events around blocks of calls.
  host_feedback_ms         packed.cpu() of the loss head's output followed by the stock update_priorities (a Python loop over
      the batch with one numpy.max per sample), host clock.
  device_feedback_ms / device_feedback_device_ms   the device scatter on the same priorities: host clock ending in a
      synchronise, and HIP events around blocks of calls.
Medians over timed blocks after a warm-up.  The stock buffer is a small stand-in so that the tool needs nothing outside
the repository.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "muzero-general_amd"))
from mzx import _lib, replay, self_play  # noqa: E402


class Stock:
    """Storage, game draw and priority feedback of a replay buffer (what mzx.replay.ReplayBuffer composes with)."""

    def __init__(self, initial_checkpoint, initial_buffer, config):
        self.config, self.buffer = config, dict(initial_buffer)
        self.num_played_games = self.num_played_steps = self.total_samples = 0

    def save_game(self, game_history, shared_storage=None):
        self.buffer[self.num_played_games] = game_history
        self.num_played_games += 1
        self.num_played_steps += len(game_history.root_values)
        self.total_samples += len(game_history.root_values)

    def sample_n_games(self, n_games, force_uniform=False):
        ids = list(self.buffer)
        probs = numpy.array([self.buffer[g].game_priority for g in ids], dtype="float32")
        probs /= probs.sum()
        chosen = numpy.random.choice(ids, n_games, p=probs)
        lookup = dict(zip(ids, probs))
        return [(g, self.buffer[g], lookup[g]) for g in chosen]

    def update_priorities(self, priorities, index_info):
        oldest = next(iter(self.buffer))
        for i in range(len(index_info)):
            game_id, pos = index_info[i]
            if oldest <= game_id:
                target = self.buffer[game_id].priorities
                end = min(pos + priorities.shape[1], len(target))
                target[pos:end] = priorities[i, :end - pos]
                self.buffer[game_id].game_priority = numpy.max(target)


def make_games(shape, A, n_games, T, dtype):
    rs = numpy.random.RandomState(0)
    out = []
    for _ in range(n_games):
        gh = self_play.GameHistory()
        gh.action_history = [0] + [int(a) for a in rs.randint(0, A, size=T)]
        gh.reward_history = [0] + [float(r) for r in rs.standard_normal(T)]
        gh.to_play_history = [0] * (T + 1)
        gh.root_values = [float(v) for v in rs.standard_normal(T)]
        gh.child_visits = [[1 / A] * A for _ in range(T)]
        gh.observation_history = list((rs.rand(T + 1, *shape) * 255).astype(dtype))
        out.append(gh)
    return out


def host_clock(fn, warmup, blocks):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def event_clock(fn, iters, blocks):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(blocks):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / iters)
    return statistics.median(times)


def run(be, name, shape, k, A, dtype, n_games, T, batch, quick):
    cfg = types.SimpleNamespace(PER=True, PER_alpha=0.5, seed=0, replay_buffer_size=10 ** 6, batch_size=batch,
                                num_unroll_steps=5, td_steps=10, discount=0.997, stacked_observations=k,
                                observation_shape=shape, action_space=list(range(A)), players=[0])
    checkpoint = {"num_played_games": 0, "num_played_steps": 0}
    buffers = {}
    for sampler in (False, True):
        store = replay.DeviceGameStore(cfg, be, n_games * (T + 1), max_games=n_games if sampler else None)
        buffers[sampler] = replay.ReplayBuffer(checkpoint, {}, cfg, stock=Stock, device_store=store, device_sampler=sampler)
        for g in make_games(shape, A, n_games, T, dtype):
            buffers[sampler].save_game(g)
    blocks = 3 if quick else 9
    iters = 5 if quick else 20
    numpy.random.seed(1)
    host_draw_ms = host_clock(buffers[False].get_batch, 2, blocks * 3)
    sampler_ms = host_clock(buffers[True].get_batch, 2, blocks * 3)
    sampler_device_ms = event_clock(buffers[True].get_batch, iters, blocks)
    # the feedback: the loss head's packed output (four losses, then the priorities) of one batch, both ways
    steps = cfg.num_unroll_steps + 1
    packed = torch.rand(4 + batch * steps, device=be.device)
    host_index = buffers[False].get_batch()[0]
    device_index = buffers[True].get_batch()[0]

    def host_feedback():
        host = packed.cpu().numpy()
        buffers[False].update_priorities(host[4:].reshape(batch, steps), host_index)

    def device_feedback():
        buffers[True].update_priorities(packed[4:].view(batch, steps), device_index)

    host_feedback_ms = host_clock(host_feedback, 2, blocks * 3)
    device_feedback_ms = host_clock(device_feedback, 2, blocks * 3)
    device_feedback_device_ms = event_clock(device_feedback, iters, blocks)
    return {
        "geometry": name, "observation_shape": list(shape), "stacked_observations": k, "batch": batch, "games": n_games,
        "positions_per_game": T, "host_draw_get_batch_ms": round(host_draw_ms, 3), "sampler_get_batch_ms": round(sampler_ms, 3),
        "sampler_device_ms": round(sampler_device_ms, 4), "get_batch_speedup": round(host_draw_ms / sampler_ms, 2),
        "host_feedback_ms": round(host_feedback_ms, 3), "device_feedback_ms": round(device_feedback_ms, 3),
        "device_feedback_device_ms": round(device_feedback_device_ms, 4),
        "feedback_speedup": round(host_feedback_ms / device_feedback_ms, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_sampler_bench.log"))
    ap.add_argument("--quick", action="store_true", help="fewer timed blocks (a rehearsal)")
    args = ap.parse_args()
    be = _lib.default_backend()
    legs = [
        # name, shape, k, A, frame dtype, games, positions per game, batch
        ("cartpole", (1, 1, 4), 0, 2, numpy.float32, 64, 500, 128),
        ("connect4", (3, 6, 7), 0, 7, numpy.int32, 256, 30, 1024),
        ("atari", (3, 96, 96), 32, 18, numpy.float32, 8, 200, 1024),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        head = (f"# replay_sampler_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; medians of timed blocks; "
                "get_batch with host draws against the device sampler, priority feedback through the host against the device scatter")
        print(head)
        log.write(head + "\n")
        for leg in legs:
            line = json.dumps(run(be, *leg, args.quick))
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
