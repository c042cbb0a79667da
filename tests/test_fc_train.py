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
from mzx import _lib, configs, models, trainer
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


def test_two_sgd_momentum_steps(be, gold):
    cases.check_sgd(be, cases.BY_NAME["b5_k4_stacked"], gold)


def check_adam_bit_for_bit(be, case):
    hp = dict(lr=0.02, weight_decay=1e-4)
    net = cases.network(be, case)
    before = net.flat_weights().clone()
    optimizer = torch.optim.Adam(net.parameters(), **hp)
    trainer.update_weights(net, optimizer, cases.batch(case), cases.config_of(case))
    grad = next(net.parameters()).grad
    want = cases.adam_reference_step(net, grad, before, **hp)
    got = net.flat_weights()
    assert not torch.equal(got, before)
    assert numpy.array_equal(got.cpu().numpy().view(numpy.int32), want.cpu().numpy().view(numpy.int32))


def test_adam_on_the_flat_parameter_is_adam_per_tensor(be):
    check_adam_bit_for_bit(be, cases.BY_NAME["b5_k4_stacked"])


def test_parameters_is_one_leaf_over_the_flat_buffer(be):
    net = cases.network(be, cases.CASES[2])
    params = list(net.parameters())
    assert len(params) == 1 and isinstance(params[0], torch.nn.Parameter) and params[0].is_leaf and params[0].requires_grad
    assert params[0].data_ptr() == net.flat_weights().data_ptr() and params[0].shape == (net.num_params,)
    assert not any(v.requires_grad for v in net.state_dict().values())


def check_optimizer_state_round_trip(be, case, make):
    net = cases.network(be, case)
    optimizer = make(net.parameters())
    for _ in range(2):
        trainer.update_weights(net, optimizer, cases.batch(case), cases.config_of(case))
    state = trainer.optimizer_state(optimizer, net)
    assert sorted(state["state"]) == list(range(len(net._tensors)))
    assert state["param_groups"][0]["params"] == list(range(len(net._tensors)))
    for i, (_, _, _, shape) in enumerate(net._tensors):
        for value in state["state"][i].values():
            assert not torch.is_tensor(value) or value.dim() == 0 or tuple(value.shape) == tuple(shape)
    twin_net = cases.network(be, case)
    twin = make(twin_net.parameters())
    trainer.load_optimizer_state(twin, twin_net, state)
    again = trainer.optimizer_state(twin, twin_net)
    assert again["param_groups"] == state["param_groups"] and sorted(again["state"]) == sorted(state["state"])
    for i in state["state"]:
        assert list(again["state"][i]) == list(state["state"][i])
        for key, value in state["state"][i].items():
            other = again["state"][i][key]
            assert torch.equal(value, other) if torch.is_tensor(value) else value == other, (i, key)
    return state


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


def _io(be, case, net, keep):
    """A complete mzx_train_fc_io over host tensors, outputs pre-filled with 7."""
    observation, action, tv, tr, tp, weight, scale = cases.batch(case)
    B, steps = case["B"], case["steps"]
    t = dict(observation=torch.from_numpy(observation).reshape(B, -1).contiguous(), action=torch.from_numpy(action).to(torch.int32),
             tv=torch.from_numpy(tv), tr=torch.from_numpy(tr), tp=torch.from_numpy(tp), scale=torch.from_numpy(scale),
             grad=torch.full((net.num_params,), 7.0), losses=torch.full((4,), 7.0), priorities=torch.full((B, steps), 7.0))
    nbytes = int(be.lib.mzx_train_fc_scratch_bytes(net.handle, B, steps))
    t["scratch"] = torch.full((max(nbytes, 16) // 4,), 7.0)
    keep.append(t)
    io = _lib.TrainFcIO()
    io.d_flat, io.d_observation, io.d_action = net.flat_weights().data_ptr(), t["observation"].data_ptr(), t["action"].data_ptr()
    io.d_target_value, io.d_target_reward, io.d_target_policy = t["tv"].data_ptr(), t["tr"].data_ptr(), t["tp"].data_ptr()
    io.d_gradient_scale = t["scale"].data_ptr()
    io.batch, io.steps, io.value_loss_weight, io.per_alpha = B, steps, case["vlw"], case["alpha"]
    io.d_grad_flat, io.d_losses, io.d_priorities = t["grad"].data_ptr(), t["losses"].data_ptr(), t["priorities"].data_ptr()
    io.d_scratch, io.scratch_bytes = t["scratch"].data_ptr(), nbytes
    return io, t


REQUIRED = ("d_flat", "d_observation", "d_action", "d_target_value", "d_target_reward", "d_target_policy", "d_gradient_scale",
            "d_grad_flat", "d_losses", "d_priorities", "d_scratch")
BAD = [(f, None) for f in REQUIRED] + [("batch", 0), ("batch", -1), ("steps", 0), ("steps", -2), ("scratch_bytes", 64)]


def check_refusals(be, field, value):
    case, keep = cases.CASES[1], []
    net = cases.network(be, case)
    io, t = _io(be, case, net, keep)
    setattr(io, field, value)
    assert be.lib.mzx_train_fc_step(net.handle, ctypes.byref(io), None) == -1        # MZX_ERR_INVALID
    assert be.lib.mzx_last_error()
    for key in ("grad", "losses", "priorities", "scratch"):                             # nothing was launched
        assert (t[key] == 7.0).all(), key
    return net, case, keep


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_abi_refusals(be, field, value):
    net, case, keep = check_refusals(be, field, value)
    io, t = _io(be, case, net, keep)                                    # (and the untouched struct is accepted)
    assert be.lib.mzx_train_fc_step(net.handle, ctypes.byref(io), None) == 0
    assert not (t["losses"] == 7.0).any() and not (t["grad"] == 7.0).any()


def test_abi_refuses_a_residual_network_and_null_arguments(be):
    case, keep = cases.CASES[1], []
    net = cases.network(be, case)
    residual = models.MuZeroNetwork(configs.tictactoe(), _backend=be)
    io, t = _io(be, case, net, keep)
    assert be.lib.mzx_train_fc_step(residual.handle, ctypes.byref(io), None) == -1
    assert "residual" in be.lib.mzx_last_error().decode()
    assert be.lib.mzx_train_fc_step(None, ctypes.byref(io), None) == -1
    assert be.lib.mzx_train_fc_step(net.handle, None, None) == -1
    for key in ("grad", "losses", "priorities", "scratch"):
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
