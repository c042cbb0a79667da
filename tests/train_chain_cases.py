"""
Whole training steps queued by one library call (mzx_train_chain, mzx.trainer.train_steps), for the serial build
(tests/test_train_chain.py) and the device (tests/test_gpu_train_chain.py): twin setups that start from the same store
contents, weights, optimizer state and ``_sample_calls``; one runs ``train_steps(n)``, the other the loop of its
definition (``update_lr`` + ``train_step`` per step); everything they leave is compared bit for bit.

The stores are built as tests/replay_sampler_cases.py builds its stores (``game``, ``FeedbackStock``): three games of 2, 6
and 4 positions, so that with batch 5 and up to three unroll steps sampled windows overlap and run past game ends in
every step.  lr_decay_steps = 3 with the chain starting at training step 2: the step counter crosses it inside the chain.
"""
import numpy
import pytest
import torch

import fc_train_cases
import replay_sampler_cases
import resnet_train_cases
import trainer_loss_cases
from mzx import models, optim, replay, trainer

LENGTHS = (2, 6, 4)
FIRST_TRAINING_STEP = 2
FIRST_SAMPLE_CALL = 8      # (the six draws from here on all have the property check_windows_overlap_and_pass_game_ends asserts)
NETWORKS = {
    "fc_b5_k4": (fc_train_cases, fc_train_cases.BY_NAME["b5_k4_stacked"]),
    "resnet_a_b2_k1": (resnet_train_cases, resnet_train_cases.BY_NAME["a_b2_k1"]),      # the smallest residual case
    "resnet_b_b3_k3": (resnet_train_cases, resnet_train_cases.BY_NAME["b_b3_k3"]),      # with dynamics applications
}
ROWS = [(name, per, n) for name in NETWORKS for per in (False, True) for n in (1, 5)]


def config_for(name, per, **kw):
    tables, case = NETWORKS[name]
    base = dict(PER=per, td_steps=3, discount=0.997, seed=7, replay_buffer_size=10 ** 6, lr_init=0.02, lr_decay_rate=0.8,
                lr_decay_steps=3, weight_decay=1e-4, momentum=0.9, optimizer="Adam")
    base.update(kw)
    return tables.config_of(case, **base)


def make_buffer(be, cfg, per, device_sampler=True):
    """The store and its buffer: three games, their priorities with PER, the call counter at FIRST_SAMPLE_CALL."""
    store = replay.DeviceGameStore(cfg, be, sum(LENGTHS) + len(LENGTHS), max_games=4)
    buffer = replay.ReplayBuffer(dict(replay_sampler_cases.CHECKPOINT), {}, cfg, stock=replay_sampler_cases.FeedbackStock,
                                 device_store=store, device_sampler=device_sampler)
    rs = numpy.random.RandomState(11)
    for k, T in enumerate(LENGTHS):
        buffer.save_game(replay_sampler_cases.game(cfg, T, 500 + k, priorities=0.1 + rs.random_sample(T) if per else None))
    buffer._sample_calls = FIRST_SAMPLE_CALL
    return buffer, store


def setup(be, name, per, kind="adam", warm=True, **kw):
    """(config, network, optimizer, buffer, store) with one warm-up ``train_step`` behind them (``warm``: the optimizer
    state and ``.grad`` exist, the priorities have been written once)."""
    tables, case = NETWORKS[name]
    cfg = config_for(name, per, **kw)
    buffer, store = make_buffer(be, cfg, per)
    net = tables.network(be, case)
    optimizer = (optim.Adam(net.parameters(), lr=cfg.lr_init, weight_decay=cfg.weight_decay) if kind == "adam" else
                 optim.SGD(net.parameters(), lr=cfg.lr_init, momentum=cfg.momentum, weight_decay=cfg.weight_decay))
    if warm:
        trainer.update_lr(optimizer, cfg, FIRST_TRAINING_STEP - 1)
        trainer.train_step(net, optimizer, buffer, cfg)
    return cfg, net, optimizer, buffer, store


def the_loop(net, optimizer, buffer, cfg, n, training_step):
    losses = []
    for i in range(n):
        trainer.update_lr(optimizer, cfg, training_step + i)
        losses.append(trainer.train_step(net, optimizer, buffer, cfg))
    return torch.stack(losses)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32) if t.is_floating_point() else t


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


def snapshot(net, optimizer, buffer, store):
    state = optimizer.state_dict()
    out = {"flat": net.flat_weights(), "derived": net._derived, "priorities": store.priorities, "slot_priority": store.slot_priority,
           "slot_sum": store.slot_sum, "grad": next(net.parameters()).grad}
    for key, value in state["state"].get(0, {}).items():
        out["state/" + key] = value if torch.is_tensor(value) else torch.tensor(value)
    scalars = {"lr": state["param_groups"][0]["lr"], "sample_calls": buffer._sample_calls,
               "tracked": {k: int(v) for k, v in net._num_batches_tracked.items()}}
    return {k: v.detach().clone() for k, v in out.items() if v is not None}, scalars      # (no .grad before the first step)


def check_row(be, name, per, n, kind="adam", warm=True):
    chained, looped = (setup(be, name, per, kind, warm) for _ in range(2))
    before, _ = snapshot(*chained[1:])
    start, _ = snapshot(*looped[1:])
    for key in before:
        same(before[key], start[key], "start " + key)
    cfg, net, optimizer, buffer, store = chained
    got = trainer.train_steps(net, optimizer, buffer, cfg, n, FIRST_TRAINING_STEP)
    assert got.shape == (n, 4) and got.dtype == torch.float32 and got.device.type == be.device.type
    cfg2, net2, optimizer2, buffer2, store2 = looped
    want = the_loop(net2, optimizer2, buffer2, cfg2, n, FIRST_TRAINING_STEP)
    same(got, want, "losses")
    assert torch.isfinite(got).all()
    after, scalars = snapshot(*chained[1:])
    after2, scalars2 = snapshot(*looped[1:])
    assert sorted(after) == sorted(after2)
    for key in after:
        same(after[key], after2[key], key)
    assert scalars == scalars2, (scalars, scalars2)
    assert scalars["sample_calls"] == FIRST_SAMPLE_CALL + int(warm) + n
    assert scalars["lr"] == cfg.lr_init * cfg.lr_decay_rate ** ((FIRST_TRAINING_STEP + n - 1) / cfg.lr_decay_steps)
    if kind == "adam":
        assert float(after["state/step"]) == int(warm) + n
    assert not torch.equal(after["flat"], before["flat"])
    if per:
        assert not torch.equal(after["priorities"], before["priorities"])
    else:
        same(after["priorities"], before["priorities"], "priorities without PER")
    if NETWORKS[name][0] is resnet_train_cases:
        assert scalars["tracked"] and all(v % (int(warm) + n) == 0 for v in scalars["tracked"].values())
        assert max(scalars["tracked"].values()) > 0


def check_windows_overlap_and_pass_game_ends(be):
    """What the docstring promises of the store as it starts: in every draw of the rows' range of call counters, with and
    without PER, two windows share a position and one runs past the end of its game."""
    for per in (True, False):
        cfg, net, optimizer, buffer, store = setup(be, "fc_b5_k4", per, warm=False)
        U = cfg.num_unroll_steps
        for call in range(FIRST_SAMPLE_CALL, FIRST_SAMPLE_CALL + 6):
            base, length, pos, tape, game_id, weight = store.sample(cfg.batch_size, cfg.seed, call, buffer.total_samples, per, U)
            base, length, pos = (t.cpu().numpy() for t in (base, length, pos))
            assert (pos + U > length).any(), call
            rows = [set(range(int(b + p), int(b + min(p + U + 1, T)))) for b, p, T in zip(base, pos, length)]
            assert any(rows[i] & rows[j] for i in range(len(rows)) for j in range(i)), call


REFUSALS = ["a torch optimizer", "a torch model", "no device sampler", "a refused network", "scratch above the ceiling", "n = 0"]


def check_refusal(be, what):
    """Every refusal raises by name before anything is queued: the weights, the priorities and the counters stay."""
    cfg, net, optimizer, buffer, store = setup(be, "fc_b5_k4", True)
    before, scalars = snapshot(net, optimizer, buffer, store)
    args = [net, optimizer, buffer, cfg, 2, FIRST_TRAINING_STEP]
    error, match = NotImplementedError, what
    if what == "a torch optimizer":
        args[1] = torch.optim.Adam(net.parameters(), lr=0.02)
        match = "torch optimizer"
    elif what == "a torch model":
        width = int(numpy.prod(store.sample_shape))
        args[0] = trainer_loss_cases.TinyModel(width, 8, cfg.support_size, len(cfg.action_space)).to(be.device)
        match = "torch model"
    elif what == "no device sampler":
        args[2] = replay.ReplayBuffer(dict(replay_sampler_cases.CHECKPOINT), {}, cfg, stock=replay_sampler_cases.FeedbackStock,
                                      device_store=store)
        match = "device sampler"
    elif what == "a refused network":
        wide = dict(fc_train_cases.BY_NAME["b2_k2_wide"], S=fc_train_cases.WIDE_UNSUPPORTED_S)
        args[0] = models.MuZeroNetwork(fc_train_cases.config_of(wide), _backend=be)
        args[1] = optim.Adam(args[0].parameters(), lr=0.02)
        match = "160 KiB LDS budget"
    elif what == "scratch above the ceiling":
        cfg.train_scratch_max_bytes = 64
        match = "train_scratch_max_bytes"
    else:
        args[4] = 0
        error, match = ValueError, "n = 0"
    with pytest.raises(error, match=match):
        trainer.train_steps(*args)
    after, scalars2 = snapshot(net, optimizer, buffer, store)
    for key in before:
        same(after[key], before[key], key)
    assert scalars == scalars2
