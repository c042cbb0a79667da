"""
``mzx.trainer.Trainer`` (trainer.py:13-123) for the serial build (tests/test_trainer_worker.py) and the device
(tests/test_gpu_trainer_worker.py): the worker loop over a ``LocalStorage`` against a twin per-step loop, on the network
and the store of tests/train_chain_cases.py (b5_k4_stacked, batch 5, three games of 2, 6 and 4 positions).
"""
import copy

import torch

import fc_train_cases
import train_chain_cases as chain
from mzx import models, optim, shared_storage, trainer

NAME = "fc_b5_k4"
LOGGED = ("training_step", "lr", "total_loss", "value_loss", "reward_loss", "policy_loss")      # trainer.py:98-107
PUBLISHED = ("weights", "optimizer_state")                                                      # trainer.py:88-95


class RecordingStorage(shared_storage.LocalStorage):
    """``LocalStorage`` that keeps every ``set_info`` call; ``terminate_after`` polls of "terminate" it answers True."""

    def __init__(self, terminate_after=None, **entries):
        super().__init__(**{"num_played_games": 1, "num_played_steps": 10 ** 9, "terminate": False, **entries})
        self.calls, self.polls, self.terminate_after, self.checkpoints = [], 0, terminate_after, 0

    def get_info(self, keys):
        if keys == "terminate" and self.terminate_after is not None:
            self.polls += 1
            return self.polls > self.terminate_after
        return super().get_info(keys)

    def set_info(self, keys, values=None):
        self.calls.append(copy.deepcopy(keys))
        super().set_info(keys, values)

    def save_checkpoint(self):
        self.checkpoints += 1


def config(per=True, **kw):
    base = dict(training_steps=7, checkpoint_interval=3, train_steps_chunk=4, training_delay=0, ratio=None, save_model=False,
                optimizer="Adam", train_on_gpu=True)
    base.update(kw)
    return chain.config_for(NAME, per, **base)


def checkpoint():
    tables, case = chain.NETWORKS[NAME]
    return {"weights": {k: torch.from_numpy(v) for k, v in tables.weights(case).items()}, "training_step": 0, "optimizer_state": None}


def worker(be, cfg, **buffer_kw):
    buffer, store = chain.make_buffer(be, cfg, cfg.PER, **buffer_kw)
    return trainer.Trainer(checkpoint(), cfg, _backend=be), buffer, store


def twin_loop(be, cfg, steps, at):
    """The per-step loop of the definition on a twin -> ({step: (weights, optimizer state)} for the steps of ``at``, the last
    step's four losses, the last lr, the twin)."""
    tables, case = chain.NETWORKS[NAME]
    buffer, store = chain.make_buffer(be, cfg, cfg.PER)
    net = tables.network(be, case)
    optimizer = optim.from_config(net, cfg)
    seen = {}
    for step in range(steps):
        trainer.update_lr(optimizer, cfg, step)
        losses = trainer.train_step(net, optimizer, buffer, cfg)
        if step + 1 in at:
            seen[step + 1] = (copy.deepcopy(net.get_weights()), trainer.optimizer_state(optimizer, net))
    return seen, [float(x) for x in losses.cpu().numpy()], optimizer.param_groups[0]["lr"], net


def same_nested(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            same_nested(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_nested(x, y, f"{where}[{i}]")
    elif torch.is_tensor(a):
        chain.same(a, b, where)
    else:
        assert a == b, (where, a, b)


def check_loop(be):
    """training_steps 7, checkpoint_interval 3, chunks of 4: chunks of 3, 3 and 1; publications at 3 and 6 equal the twin's
    state there bit for bit, in the reference's per-parameter layout; the last logged entries are the twin's."""
    cfg = config()
    me, buffer, store = worker(be, cfg)
    storage = RecordingStorage()
    me.continuous_update_weights(buffer, storage)
    assert me.training_step == 7 and me.route == "chain"
    assert isinstance(me.optimizer, optim.Adam)
    seen, losses, lr, twin = twin_loop(be, cfg, 7, (3, 6))
    published = [c for c in storage.calls if "weights" in c]
    logged = [c for c in storage.calls if "training_step" in c]
    assert [tuple(c) for c in published] == [PUBLISHED] * 2 and [tuple(c) for c in logged] == [LOGGED] * 3
    assert [c["training_step"] for c in logged] == [3, 6, 7]
    assert [tuple(c) for c in storage.calls] == [PUBLISHED, LOGGED, PUBLISHED, LOGGED, LOGGED]
    table = twin._tensors      # (fully connected: every tensor is a parameter)
    for call, step in zip(published, (3, 6)):
        weights, state = seen[step]
        same_nested(call["weights"], weights, f"weights at {step}")
        same_nested(call["optimizer_state"], state, f"optimizer_state at {step}")
        per_param = call["optimizer_state"]
        assert sorted(per_param["state"]) == list(range(len(table)))
        assert per_param["param_groups"][0]["params"] == list(range(len(table)))
        for i, (_, _, _, shape) in enumerate(table):
            assert list(per_param["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
            assert float(per_param["state"][i]["step"]) == step
            assert tuple(per_param["state"][i]["exp_avg"].shape) == tuple(shape) == tuple(per_param["state"][i]["exp_avg_sq"].shape)
    last = logged[-1]
    assert [last[k] for k in LOGGED[2:]] == losses and last["lr"] == lr == me.optimizer.param_groups[0]["lr"]
    chain.same(me.model.flat_weights(), twin.flat_weights(), "final weights")
    assert storage.checkpoints == 0
    return me


def check_reference_sequence(be):
    """train_steps_chunk = 1: the storage sees the reference's sequence of set_info calls (trainer.py:87-107: after every
    step the six logged entries, before them weights + optimizer_state when the step is a multiple of checkpoint_interval),
    and save_checkpoint with config.save_model."""
    cfg = config(train_steps_chunk=1, save_model=True)
    me, buffer, store = worker(be, cfg)
    storage = RecordingStorage()
    me.continuous_update_weights(buffer, storage)
    want = []
    for step in range(1, 8):
        if step % 3 == 0:
            want.append(PUBLISHED)
        want.append(LOGGED)
    assert [tuple(c) for c in storage.calls] == want
    assert [c["training_step"] for c in storage.calls if "training_step" in c] == list(range(1, 8))
    assert storage.checkpoints == 2 and me.training_step == 7


def check_ratio_wait(be, monkeypatch):
    """ratio set, few played steps: after the first chunk the loop waits (time.sleep, patched) until the storage says
    terminate; it leaves without training further."""
    sleeps = []
    monkeypatch.setattr(trainer.time, "sleep", sleeps.append)
    cfg = config(ratio=0.5, training_delay=0.25)
    me, buffer, store = worker(be, cfg)
    storage = RecordingStorage(terminate_after=4, num_played_steps=1)      # poll 1: the loop head; 2 .. 4: the wait; 5: True
    me.continuous_update_weights(buffer, storage)
    assert me.training_step == 3                                            # one chunk (to the checkpoint), no more
    assert sleeps == [0.25, 0.5, 0.5, 0.5]
    assert [c["training_step"] for c in storage.calls if "training_step" in c] == [3]


def check_terminate_first(be, monkeypatch):
    sleeps = []
    monkeypatch.setattr(trainer.time, "sleep", sleeps.append)
    cfg = config()
    me, buffer, store = worker(be, cfg)
    before = me.model.flat_weights().clone()
    storage = RecordingStorage(terminate_after=0)
    me.continuous_update_weights(buffer, storage)
    assert me.training_step == 0 and storage.calls == [] and me.route is None and not sleeps
    assert torch.equal(me.model.flat_weights(), before) and buffer._sample_calls == chain.FIRST_SAMPLE_CALL


def check_waits_for_a_game(be, monkeypatch):
    class Filling(RecordingStorage):
        def get_info(self, keys):
            if keys == "num_played_games":
                self.asked = getattr(self, "asked", 0) + 1
                return 0 if self.asked < 3 else 1
            return super().get_info(keys)

    sleeps = []
    monkeypatch.setattr(trainer.time, "sleep", sleeps.append)
    cfg = config(training_steps=1)
    me, buffer, store = worker(be, cfg)
    me.continuous_update_weights(buffer, Filling())
    assert sleeps == [0.1, 0.1] and me.training_step == 1


def check_torch_model_route(be):
    """A torch model (and its torch optimizer) takes the per-step route, and the worker says so."""
    import numpy
    import trainer_loss_cases
    cfg = config(training_steps=4)
    me, buffer, store = worker(be, cfg)
    width = int(numpy.prod(store.sample_shape))
    torch.manual_seed(5)
    me.model = trainer_loss_cases.TinyModel(width, 8, cfg.support_size, len(cfg.action_space)).to(be.device)
    me.model.get_weights = lambda: models.dict_to_cpu(me.model.state_dict())      # AbstractNetwork.get_weights (models.py:69-70)
    me.optimizer = torch.optim.SGD(me.model.parameters(), lr=cfg.lr_init)
    before = [p.detach().clone() for p in me.model.parameters()]
    storage = RecordingStorage()
    me.continuous_update_weights(buffer, storage)
    assert me.route == "step" and "torch model" in me.route_reason and me.training_step == 4
    assert buffer._sample_calls == chain.FIRST_SAMPLE_CALL + 4
    assert any(not torch.equal(a, b) for a, b in zip(before, me.model.parameters()))
    assert [c["training_step"] for c in storage.calls if "training_step" in c] == [3, 4]
    assert isinstance(storage.calls[0]["optimizer_state"], dict)


def check_host_buffer_route(be):
    """A buffer without the device sampler: get_batch / update_weights / update_priorities, step by step."""
    cfg = config(training_steps=2)
    me, buffer, store = worker(be, cfg, device_sampler=False)
    storage = RecordingStorage()
    me.continuous_update_weights(buffer, storage)
    assert me.route == "host" and "device sampler" in me.route_reason and me.training_step == 2
    assert [c["training_step"] for c in storage.calls if "training_step" in c] == [2]


def check_bound_forms_and_checkpoint(be):
    """``update_lr`` / ``update_weights`` are the module functions bound; a checkpoint with a reference-format optimizer
    state resumes where it was saved."""
    cfg = config(training_steps=3)
    me, buffer, store = worker(be, cfg)
    storage = RecordingStorage()
    me.continuous_update_weights(buffer, storage)
    saved = next(c for c in storage.calls if "weights" in c)
    resumed = trainer.Trainer({"weights": saved["weights"], "training_step": 3, "optimizer_state": saved["optimizer_state"]}, cfg,
                              _backend=be)
    assert resumed.training_step == 3
    chain.same(resumed.model.flat_weights(), me.model.flat_weights(), "resumed weights")
    same_nested(trainer.optimizer_state(resumed.optimizer, resumed.model), saved["optimizer_state"], "resumed optimizer state")
    resumed.update_lr()
    assert resumed.optimizer.param_groups[0]["lr"] == cfg.lr_init * cfg.lr_decay_rate ** (3 / cfg.lr_decay_steps)
    tables, case = chain.NETWORKS[NAME]
    out = resumed.update_weights(tables.batch(case))
    assert resumed.training_step == 4 and len(out) == 5 and out[0].shape == (case["B"], case["steps"])
    cfg.optimizer = "RMSprop"
    try:
        trainer.Trainer(checkpoint(), cfg, _backend=be)
    except NotImplementedError as e:
        assert "RMSprop is not implemented" in str(e)
    else:
        raise AssertionError("an unknown optimizer must raise")
    assert isinstance(resumed.model, models.HipNetwork) and fc_train_cases is tables
