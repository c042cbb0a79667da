"""
ReplayBuffer.get_batch with and without a device-resident store (mzx.replay.DeviceGameStore), on the GPU, at three
geometries: games/atari.py (3 x 96 x 96 frames, 32 stacked observations: 131 planes per sample; batch 128 and 1024),
Connect4 (3 x 6 x 7, nothing stacked) and CartPole (1 x 1 x 4).

    python muzero-general_amd/tools/device_replay_bench.py [--out profiles/device_replay_bench.log] [--quick]

Per geometry and batch size, one JSON line (printed, and appended to the log):
  host_get_batch_ms / host_batch_to_trainer_ms   the host path: get_batch, and get_batch + trainer_tensors (the upload
      the trainer does, trainer.py:140-153), host clock around work that ends in a device synchronise.  At the atari
      geometry the host leg runs a SMALLER batch (host_batch; one sample is 4.8 MB assembled by 32 numpy concatenations)
      and the line also gives the per-sample time scaled to the device leg's batch (host_get_batch_ms_scaled).
  device_get_batch_ms / device_batch_to_trainer_ms   the same two figures with the store.
  gather_ms, gather_written_GBps, gather_frac_of_8TBps   the observation gather alone (mzx_replay_batch with only the
      observation pointer), HIP events around blocks of launches; bytes = the output written.
  obs_stack_ms, obs_stack_written_GBps   mzx_obs_stack writing the same number of bytes (a FrameStore of `batch` games
      with a full ring), same process, same timer: the yardstick for the gather.
Medians over timed blocks after a warm-up.  The stock buffer is a small stand-in (uniform / PER game draw) so that the tool
needs nothing outside the repository.
"""
import argparse
import ctypes
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
from mzx import _lib, observations, replay, self_play  # noqa: E402


class Stock:
    """Storage + game draw of a replay buffer (what mzx.replay.ReplayBuffer composes with)."""

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


def run(be, name, shape, k, A, dtype, n_games, T, batch, host_batch, quick):
    cfg = types.SimpleNamespace(PER=True, PER_alpha=0.5, seed=0, replay_buffer_size=10 ** 6, batch_size=batch,
                                num_unroll_steps=5, td_steps=10, discount=0.997, stacked_observations=k,
                                observation_shape=shape, action_space=list(range(A)), players=[0])
    games = make_games(shape, A, n_games, T, dtype)
    checkpoint = {"num_played_games": 0, "num_played_steps": 0}
    host_cfg = types.SimpleNamespace(**{**vars(cfg), "batch_size": host_batch})
    plain = replay.ReplayBuffer(checkpoint, {}, host_cfg, stock=Stock)
    store = replay.DeviceGameStore(cfg, be, n_games * (T + 1))
    device = replay.ReplayBuffer(checkpoint, {}, cfg, stock=Stock, device_store=store)
    t0 = time.perf_counter()
    for g in games:
        device.save_game(g)
    torch.cuda.synchronize()
    ingest_ms = (time.perf_counter() - t0) * 1e3 / n_games
    for g in games:
        plain.save_game(g)
    blocks = 3 if quick else 7
    numpy.random.seed(1)
    host_ms = host_clock(plain.get_batch, 1, max(2, blocks // 2))
    host_full_ms = host_clock(lambda: replay.trainer_tensors(plain.get_batch()[1], be.device), 1, max(2, blocks // 2))
    device_ms = host_clock(device.get_batch, 2, blocks * 3)
    device_full_ms = host_clock(lambda: replay.trainer_tensors(device.get_batch()[1], be.device), 2, blocks * 3)
    # the gather alone: the samples of one drawn batch, only the observation pointer set
    index = device.get_batch()[0]
    base = torch.tensor([store.games[g][0] for g, _ in index], dtype=torch.int64, device=be.device)
    length = torch.tensor([store.games[g][1] for g, _ in index], dtype=torch.int32, device=be.device)
    pos = torch.tensor([p for _, p in index], dtype=torch.int32, device=be.device)
    out = be.empty((batch,) + store.sample_shape, torch.float32)
    io = _lib.ReplayBatchIO()
    io.d_base, io.d_len, io.d_pos, io.d_observation = base.data_ptr(), length.data_ptr(), pos.data_ptr(), out.data_ptr()
    io.num_samples, io.stacked_observations = batch, k
    lib, stream = be.lib, be.stream()
    iters = 5 if quick else 20
    gather_ms = event_clock(lambda: lib.check(lib.mzx_replay_batch(ctypes.byref(store.pool), ctypes.byref(io), stream)), iters, blocks)
    written = out.numel() * 4
    del out
    # the yardstick: mzx_obs_stack writing the same bytes (every stacked slot holds a real frame)
    frames = observations.FrameStore(cfg, batch, be)
    frames.frames.uniform_(0, 255)
    frames.actions.random_(0, A)
    frames.time = 2 * (k + 1)
    stack_ms = event_clock(frames.stacked, iters, blocks)
    line = {
        "geometry": name, "observation_shape": list(shape), "stacked_observations": k, "planes_per_sample": store.sample_shape[0],
        "batch": batch, "host_batch": host_batch, "games": n_games, "positions_per_game": T,
        "ingest_ms_per_game": round(ingest_ms, 3),
        "host_get_batch_ms": round(host_ms, 3), "host_batch_to_trainer_ms": round(host_full_ms, 3),
        "host_get_batch_ms_scaled": round(host_ms * batch / host_batch, 3),
        "host_batch_to_trainer_ms_scaled": round(host_full_ms * batch / host_batch, 3),
        "device_get_batch_ms": round(device_ms, 3), "device_batch_to_trainer_ms": round(device_full_ms, 3),
        "gather_written_bytes": written, "gather_ms": round(gather_ms, 4),
        "gather_written_GBps": round(written / gather_ms / 1e6, 1), "gather_frac_of_8TBps": round(written / gather_ms / 1e6 / 8000, 4),
        "obs_stack_ms": round(stack_ms, 4), "obs_stack_written_GBps": round(written / stack_ms / 1e6, 1),
        "gather_over_obs_stack": round(stack_ms / gather_ms, 3),
    }
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_replay_bench.log"))
    ap.add_argument("--quick", action="store_true", help="fewer timed blocks (a rehearsal)")
    args = ap.parse_args()
    be = _lib.default_backend()
    legs = [
        # name, shape, k, A, frame dtype, games, positions per game, batch, host batch
        ("atari", (3, 96, 96), 32, 18, numpy.float32, 8, 200, 128, 16),
        ("atari", (3, 96, 96), 32, 18, numpy.float32, 8, 200, 1024, 16),
        ("connect4", (3, 6, 7), 0, 7, numpy.int32, 256, 30, 1024, 1024),
        ("cartpole", (1, 1, 4), 0, 2, numpy.float32, 64, 500, 128, 128),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        head = (f"# device_replay_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; medians of timed blocks; "
                "at the atari geometry the host leg runs host_batch samples (one sample is 4.8 MB built by 32 numpy "
                "concatenations), *_scaled = per-sample time x batch")
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
