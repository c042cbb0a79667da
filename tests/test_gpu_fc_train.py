"""
Training a fully connected network natively on the device (fc_train_forward_kernel, the loss head, fc_train_backward_kernel,
wave_kernel<4, FctWgradBody> behind mzx_train_fc_step; mzx.trainer with a HipNetwork) against tests/golden/fc_train.npz, with the
gates of tests/test_fc_train.py (fc_train_cases.check_case), and the whole step -- device sampler, native gradients, Adam,
priority feedback -- followed by a search on the trained buffer.
"""
import warnings

import numpy
import pytest
import torch

import fc_train_cases as cases
import replay_sampler_cases
import test_fc_train as host_tests
import train_cases_common as common
import trainer_loss_cases
from mzx import _lib, configs, models, replay, self_play, synthetic, trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return cases.golden(golden_dir)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c["name"])
def test_logits_losses_priorities_gradients(be, gold, case):
    net, got = cases.check_case(be, case, gold)
    assert next(net.parameters()).grad.is_cuda


@pytest.mark.parametrize("case", cases.LIVE_CASES, ids=lambda c: c["name"])
def test_live_case_against_the_restatement(be, case):
    cases.check_live(be, case)


def test_two_sgd_momentum_steps(be, gold):
    cases.check_sgd(be, cases.BY_NAME["b5_k4_stacked"], gold)


def test_adam_on_the_flat_parameter_is_adam_per_tensor(be):
    common.check_adam_bit_for_bit(be, cases, cases.BY_NAME["b5_k4_stacked"])


def test_optimizer_state_round_trip(be):
    host_tests.check_optimizer_state_round_trip(be, cases.BY_NAME["b5_k4_stacked"],
                                                lambda p: torch.optim.Adam(p, lr=0.02, weight_decay=1e-4))


@pytest.mark.parametrize("field,value", [("d_scratch", None), ("steps", 0), ("scratch_bytes", 64)],
                         ids=["d_scratch=None", "steps=0", "scratch_bytes=64"])
def test_abi_refusals(be, field, value):
    common.check_abi_refusal(be, "fc", cases, cases.CASES[1], field, value, device=be.device, sync=torch.cuda.synchronize,
                             others=[models.MuZeroNetwork(configs.tictactoe())])


def test_train_step_on_the_device_then_search(be):
    cfg = replay_sampler_cases.sampler_config(True, "fc", batch_size=24, stacked_observations=0)
    cfg.value_loss_weight = 0.25
    rs = numpy.random.RandomState(3)
    lengths = [int(T) for T in rs.randint(1, 20, size=12)]
    store = replay.DeviceGameStore(cfg, be, sum(lengths) + len(lengths), max_games=16)
    buffer = replay.ReplayBuffer(dict(replay_sampler_cases.CHECKPOINT), {}, cfg, stock=replay_sampler_cases.FeedbackStock,
                                 device_store=store, device_sampler=True)
    for k, T in enumerate(lengths):
        buffer.save_game(replay_sampler_cases.game(cfg, T, 500 + k))
    net = models.MuZeroNetwork(cfg)
    net.set_weights(synthetic.fill_state_dict(net.state_dict(), 11))
    assert net.train_fc_supported(cfg.batch_size, cfg.num_unroll_steps + 1)
    B = 8
    obs = synthetic.observations(B, cfg.observation_shape, seed=5)
    legal = [list(cfg.action_space)] * B

    def searched():
        engine = self_play.BatchedMCTS(cfg, net, B)
        res = engine.run(list(obs), legal, [0] * B, False, [numpy.random.RandomState(40 + i) for i in range(B)])
        return numpy.asarray(res.root_predicted_values, numpy.float64)

    before_search = searched()
    optimizer = torch.optim.Adam(net.parameters(), lr=0.05, weight_decay=1e-4)
    before = net.flat_weights().clone()
    priorities_before = store.priorities.clone()
    trainer.train_step(net, optimizer, buffer, cfg)            # (first step: buffers and optimizer state are created)
    torch.cuda.synchronize()
    packed = []
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2):
                packed.append(trainer.train_step(net, optimizer, buffer, cfg))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()], [str(w.message) for w in caught]
    torch.cuda.synchronize()
    for p in packed:
        assert torch.is_tensor(p) and p.shape == (4,) and p.is_cuda and torch.isfinite(p).all()
    after = net.flat_weights()
    assert torch.isfinite(after).all() and (after != before).float().mean().item() > 0.9      # Adam moves every weight
    assert not torch.equal(store.priorities, priorities_before)                                 # the feedback landed
    # a search on the same network object sees the trained weights: its root predictions are initial_inference's on the
    # updated buffer (the decoded-value gate), and moved away from those before training
    value_logits = net.initial_inference(torch.from_numpy(obs))[0]
    want = models.support_to_scalar(value_logits, cfg.support_size).cpu().numpy().reshape(-1).astype(numpy.float64)
    got = searched()
    print(f"root predictions: {numpy.abs(got - want).max():.3e} from initial_inference on the trained buffer, "
          f"{numpy.abs(got - before_search).max():.3e} from the search before training")
    assert numpy.abs(got - want).max() <= trainer_loss_cases.DECODED_SCALAR_GATE
    assert numpy.abs(got - before_search).max() > 10 * trainer_loss_cases.DECODED_SCALAR_GATE
