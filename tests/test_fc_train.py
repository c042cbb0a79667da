"""
Training a fully connected network natively (mzx_train_fc_step, mzx.trainer.train_fc_gradients / update_weights with a
HipNetwork) on the serial test double of the ABI, against tests/golden/fc_train.npz -- the unmodified reference's own
step in float32 and binary64 (muzero-general_amd/tools/make_fc_train_golden.py) -- and, where the reference tree is
present, against it live.
"""
import ctypes

import numpy
import pytest
import torch

import fc_train_cases as cases
import hostcheck
import train_cases_common as common
from mzx import configs, models, trainer
from oracle import ref_shim


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return cases.golden(golden_dir)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c["name"])
def test_logits_losses_priorities_gradients(be, gold, case):
    cases.check_case(be, case, gold)


@pytest.mark.parametrize("case", cases.LIVE_CASES, ids=lambda c: c["name"])
def test_live_case_against_the_restatement(be, case):
    """Shapes the fixture does not carry (wider than a wavefront in every row loop), against the restatement in binary64."""
    cases.check_live(be, case)


def test_over64_with_hidden_layers_of_100_is_beyond_the_lds_budget(be):
    case = dict(cases.BY_NAME["b3_k3_over64"])
    assert cases.network(be, case).train_fc_supported(case["B"], case["steps"])
    for k in ("rep", "dyn", "rew", "val", "pol"):
        case[k] = [cases.OVER64_UNSUPPORTED_WIDTH]
    assert not cases.network(be, case).train_fc_supported(case["B"], case["steps"])


def test_two_sgd_momentum_steps(be, gold):
    cases.check_sgd(be, cases.BY_NAME["b5_k4_stacked"], gold)


def test_adam_on_the_flat_parameter_is_adam_per_tensor(be):
    common.check_adam_bit_for_bit(be, cases, cases.BY_NAME["b5_k4_stacked"])


def test_parameters_is_one_leaf_over_the_flat_buffer(be):
    net = cases.network(be, cases.CASES[2])
    params = list(net.parameters())
    assert len(params) == 1 and isinstance(params[0], torch.nn.Parameter) and params[0].is_leaf and params[0].requires_grad
    assert params[0].data_ptr() == net.flat_weights().data_ptr() and params[0].shape == (net.num_params,)
    assert not any(v.requires_grad for v in net.state_dict().values())


def check_optimizer_state_round_trip(be, case, make):
    return common.check_optimizer_state_round_trip(be, cases, case, make, lambda net: net._tensors)      # (no buffers: every tensor)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimizer_state_round_trip(be, kind):
    make = ((lambda p: torch.optim.SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4)) if kind == "sgd" else
            (lambda p: torch.optim.Adam(p, lr=0.02, weight_decay=1e-4)))
    check_optimizer_state_round_trip(be, cases.BY_NAME["b5_k4_stacked"], make)


def test_update_lr(be):
    net = cases.network(be, cases.CASES[0])
    optimizer = torch.optim.SGD(net.parameters(), lr=1.0)
    cfg = cases.config_of(cases.CASES[0], lr_init=0.02, lr_decay_rate=0.8, lr_decay_steps=1000)
    trainer.update_lr(optimizer, cfg, 2500)
    assert optimizer.param_groups[0]["lr"] == 0.02 * 0.8 ** (2500 / 1000)


def test_supported_shapes_and_the_limit(be):
    lib = be.lib
    for case in cases.CASES:
        net = cases.network(be, case)
        assert lib.mzx_train_fc_supported(net.handle, case["B"], case["steps"]) == 1 and net.train_fc_supported(case["B"], case["steps"])
        assert lib.mzx_train_fc_scratch_bytes(net.handle, case["B"], case["steps"]) > 0
        assert lib.mzx_train_fc_supported(net.handle, 0, 3) == 0 and lib.mzx_train_fc_supported(net.handle, 3, 0) == 0
    for game in (configs.cartpole(),):
        assert models.MuZeroNetwork(game, _backend=be).train_fc_supported(128, 11)
    wide = dict(cases.BY_NAME["b2_k2_wide"], S=cases.WIDE_UNSUPPORTED_S)      # one support bin pair past the LDS budget
    net = models.MuZeroNetwork(cases.config_of(wide), _backend=be)
    assert lib.mzx_train_fc_supported(net.handle, 2, 2) == 0 and lib.mzx_train_fc_scratch_bytes(net.handle, 2, 2) == 0
    with pytest.raises(NotImplementedError, match="160 KiB LDS budget"):
        trainer.update_weights(net, torch.optim.SGD(net.parameters(), lr=0.1), cases.batch(wide), cases.config_of(wide))
    residual = models.MuZeroNetwork(configs.tictactoe(), _backend=be)
    assert lib.mzx_train_fc_supported(residual.handle, 4, 3) == 0
    with pytest.raises(NotImplementedError, match="residual"):
        trainer.train_fc_gradients(residual, cases.batch(cases.CASES[1]), cases.config_of(cases.CASES[1]))
    assert lib.mzx_train_fc_supported(None, 4, 3) == 0


@pytest.mark.reference
def test_every_fully_connected_game_of_the_reference_is_supported(be):
    for name in ("cartpole", "gridworld", "lunarlander", "simple_grid"):
        cfg = ref_shim.muzero_config(name)
        assert cfg.network == "fullyconnected"
        net = models.MuZeroNetwork(cfg, _backend=be)
        assert net.train_fc_supported(cfg.batch_size, cfg.num_unroll_steps + 1), name


BAD = [(f, None) for f in common.REQUIRED] + [("batch", 0), ("batch", -1), ("steps", 0), ("steps", -2), ("scratch_bytes", 64),
                                              ("d_scratch", "misaligned")]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_abi_refusals(be, field, value):
    common.check_abi_refusal(be, "fc", cases, cases.CASES[1], field, value)


def test_abi_refuses_a_residual_network_and_null_arguments(be):
    case, keep = cases.CASES[1], []
    net = cases.network(be, case)
    residual = models.MuZeroNetwork(configs.tictactoe(), _backend=be)
    io, t = common.step_io(be, case, net, keep, "fc")
    assert be.lib.mzx_train_fc_step(residual.handle, ctypes.byref(io), None) == -1
    assert "residual" in be.lib.mzx_last_error().decode()
    assert be.lib.mzx_train_fc_step(None, ctypes.byref(io), None) == -1
    assert be.lib.mzx_train_fc_step(net.handle, None, None) == -1
    for key in common.OUTPUTS["fc"]:
        assert (t[key] == 7.0).all(), key


@pytest.mark.reference
@pytest.mark.parametrize("case", [c for c in cases.CASES if c["steps"] > 1], ids=lambda c: c["name"])   # (update_weights needs an unroll step)
def test_torch_restatement_is_the_reference(gold, case):
    """fc_train_cases.FcNetwork under trainer_loss_cases.torch_update_weights makes the gradients of the reference's
    Trainer.update_weights on models.MuZeroNetwork, bit for bit, on this host -- so the bench's baseline leg is the real
    thing.  Both sides are computed here and now (the fixture's float32 arrays come from the same statements on the host
    that wrote it; they are held to equality of values within float32 rounding of that host's BLAS, printed)."""
    import types

    import trainer_loss_cases

    ref_models, _ = ref_shim.load()
    import trainer as ref_trainer      # the reference's trainer.py, under the shim's ray stub
    theirs = ref_models.MuZeroNetwork(cases.config_of(case))
    theirs.set_weights({k: torch.from_numpy(v) for k, v in cases.weights(case).items()})
    ours = cases.load(cases.FcNetwork(case), cases.weights(case))
    assert list(ours.state_dict()) == list(theirs.state_dict())

    class NoOptimizer:
        zero_grad = step = lambda self: None

    me = types.SimpleNamespace(model=theirs, optimizer=NoOptimizer(), config=cases.config_of(case), training_step=0,
                               loss_function=ref_trainer.Trainer.loss_function)
    want = ref_trainer.Trainer.update_weights(me, cases.batch(case))
    got = trainer_loss_cases.torch_update_weights(ours, NoOptimizer(), cases.batch(case), cases.config_of(case))
    assert got[1] == want[1]
    for (key, a), b in zip(ours.named_parameters(), theirs.parameters()):
        assert numpy.array_equal(a.grad.numpy().view(numpy.int32), b.grad.numpy().view(numpy.int32)), key
        gap = numpy.abs(a.grad.numpy() - gold[f"{case['name']}/f32_grad/{key}"]).max()
        print(f"{case['name']} {key}: {gap:.3e} from the fixture's float32 gradient")
        assert gap <= 4 * cases.grad_gate(gold, case, key)[0]


@pytest.mark.reference
def test_optimizer_state_keys_are_the_reference_optimizers(be):
    case = cases.BY_NAME["b5_k4_stacked"]
    ref_models, _ = ref_shim.load()
    theirs = ref_models.MuZeroNetwork(cases.config_of(case))
    for kind in ("sgd", "adam"):
        make = ((lambda p: torch.optim.SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4)) if kind == "sgd" else
                (lambda p: torch.optim.Adam(p, lr=0.02, weight_decay=1e-4)))
        reference = make(theirs.parameters())
        for p in theirs.parameters():
            p.grad = torch.ones_like(p)
        reference.step()
        want = reference.state_dict()
        got = check_optimizer_state_round_trip(be, case, make)
        assert sorted(got["state"]) == sorted(want["state"])
        assert got["param_groups"][0].keys() == want["param_groups"][0].keys()
        assert got["param_groups"][0]["params"] == want["param_groups"][0]["params"]
        for i in want["state"]:
            assert list(got["state"][i]) == list(want["state"][i])
            for key, value in want["state"][i].items():
                mine = got["state"][i][key]
                assert torch.is_tensor(mine) == torch.is_tensor(value)
                if torch.is_tensor(value):
                    assert mine.shape == value.shape and mine.dtype == value.dtype, (i, key)
        reference.load_state_dict(got)          # and the reference's optimizer takes it
