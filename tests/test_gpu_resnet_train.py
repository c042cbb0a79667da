"""
Training a residual network natively on the device (wave_kernel<4, RtnGemmBody<...>> on the FP32 matrix pipes, the
BatchNorm / normalisation wave bodies and the loss head behind mzx_train_resnet_step; mzx.trainer with a residual
HipNetwork) against tests/golden/resnet_train.npz with the gates of tests/test_resnet_train.py, the shipped tic-tac-toe
and connect4 networks against the torch restatement in binary64, and the whole step -- resident self-play rounds, device
hand-off, device sampler, native gradients, Adam, the statistics commit -- followed by a search on the trained buffer.
"""
import warnings

import numpy
import pytest
import torch

import device_handoff_cases
import resident_rounds_cases as rr
import resnet_train_cases as cases
import test_resnet_train as host_tests
import train_cases_common as common
import trainer_loss_cases
from mzx import _lib, configs, games, models, self_play, synthetic, trainer
from oracle import net_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return cases.golden(golden_dir)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c["name"])
def test_logits_losses_priorities_gradients_statistics(be, gold, case):
    net, got = cases.check_case(be, case, gold)
    assert next(net.parameters()).grad.is_cuda


@pytest.mark.parametrize("case", cases.LIVE_CASES, ids=lambda c: c["name"])
def test_live_case_against_the_restatement(be, case):
    """Shapes the fixture does not carry (a state plane of range between 0 and 1e-5), against the restatement in binary64."""
    cases.check_live(be, case)


def test_two_sgd_momentum_steps_weights_and_buffers(be, gold):
    cases.check_sgd(be, cases.BY_NAME["c_b5_k4_stacked"], gold)


def test_adam_on_the_flat_parameter_is_adam_per_tensor(be):
    common.check_adam_bit_for_bit(be, cases, cases.BY_NAME["c_b5_k4_stacked"])


def test_optimizer_state_round_trip(be):
    host_tests.check_optimizer_state_round_trip(be, cases.BY_NAME["c_b5_k4_stacked"],
                                                lambda p: torch.optim.Adam(p, lr=0.02, weight_decay=1e-4))


@pytest.mark.parametrize("game", ["tictactoe", "connect4"])
def test_shipped_networks_against_the_restatement_in_binary64(be, game):
    """B = 64, steps = 3 of the shipped network (connect4: the 64-channel shape the fixture is too small to carry), held
    to the torch restatement run here on the CPU in binary64, with the reference's float32 error measured the same way."""
    cfg = getattr(configs, game)()
    cases.check_live(be, cases.case_of_config(cfg, 64, 3, name=game))


@pytest.mark.parametrize("field,value", [("d_scratch", None), ("d_stats", None), ("steps", 0), ("scratch_bytes", 64)],
                         ids=["d_scratch=None", "d_stats=None", "steps=0", "scratch_bytes=64"])
def test_abi_refusals(be, field, value):
    common.check_abi_refusal(be, "resnet", cases, cases.BY_NAME["b_b3_k3"], field, value, device=be.device,
                             sync=torch.cuda.synchronize, others=[models.MuZeroNetwork(configs.breakout())])


def test_train_step_from_resident_rounds_then_search(be):
    cfg = device_handoff_cases.replay_cfg(rr.tictactoe_cfg(), True, value_loss_weight=0.25, batch_size=16)
    weights = rr._weights(be, cfg)
    run = device_handoff_cases.Run(be, games.TicTacToeNative, cfg, weights, 5, 7, True).play(rr.TICTACTOE_CALLS)
    assert len(run.games) >= 4
    net = models.MuZeroNetwork(cfg)
    net.set_weights(weights)
    assert net.train_resnet_supported(cfg.batch_size, cfg.num_unroll_steps + 1)
    B = 8
    obs = synthetic.observations(B, cfg.observation_shape, seed=5)
    legal = [list(cfg.action_space)] * B

    def searched():
        engine = self_play.BatchedMCTS(cfg, net, B)
        res = engine.run(list(obs), legal, [0] * B, False, [numpy.random.RandomState(40 + i) for i in range(B)])
        return numpy.asarray(res.root_predicted_values, numpy.float64)

    before_search = searched()
    optimizer = torch.optim.Adam(net.parameters(), lr=0.02, weight_decay=1e-4)
    before = net.flat_weights().clone()
    priorities_before = run.store.priorities.clone()
    trainer.train_step(net, optimizer, run.buffer, cfg)          # (first step: buffers and optimizer state are created)
    torch.cuda.synchronize()
    packed = []
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2):
                packed.append(trainer.train_step(net, optimizer, run.buffer, cfg))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()], [str(w.message) for w in caught]
    torch.cuda.synchronize()
    for p in packed:
        assert torch.is_tensor(p) and p.shape == (4,) and p.is_cuda and torch.isfinite(p).all()
    after = net.flat_weights()
    assert torch.isfinite(after).all() and (after != before).float().mean().item() > 0.9
    assert not torch.equal(run.store.priorities, priorities_before)                              # the feedback landed
    # the committed statistics were re-folded: the handle's inference is eval-mode inference of get_weights()
    state = net.get_weights()
    assert all(int(v) == 3 * (1 if k.startswith("representation") else cfg.num_unroll_steps if k.startswith("dynamics")
                              else cfg.num_unroll_steps + 1) for k, v in state.items() if k.endswith("num_batches_tracked"))
    oracle = net_oracle.make_oracle_network(cfg, state)
    want = oracle.initial_inference(torch.from_numpy(obs))
    got = net.initial_inference(torch.from_numpy(obs))
    for name, a, b in zip(("value", "reward", "policy", "state"), got, want):
        a, b = a.cpu().numpy().reshape(b.shape), b.numpy()
        finite = numpy.isfinite(b)
        assert numpy.array_equal(a[~finite], b[~finite]), name
        gap = float(numpy.abs(a[finite] - b[finite]).max())
        print(f"initial_inference {name} after three training steps: {gap:.3e} from eval-mode inference of get_weights()")
        assert gap <= 1e-4, name
    value_logits = got[0]
    want_root = models.support_to_scalar(value_logits, cfg.support_size).cpu().numpy().reshape(-1).astype(numpy.float64)
    got_root = searched()
    print(f"root predictions: {numpy.abs(got_root - want_root).max():.3e} from initial_inference on the trained buffer, "
          f"{numpy.abs(got_root - before_search).max():.3e} from the search before training")
    assert numpy.abs(got_root - want_root).max() <= trainer_loss_cases.DECODED_SCALAR_GATE
    assert numpy.abs(got_root - before_search).max() > 10 * trainer_loss_cases.DECODED_SCALAR_GATE
    run.close()
