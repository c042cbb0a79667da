"""
The loss head of the trainer on the device (mzx_trainer_loss, mzx_scalar_to_support, mzx.trainer) against
tests/golden/trainer_loss.npz, with the gates of tests/test_trainer_loss.py (trainer_loss_cases.check_case).
"""
import numpy
import pytest
import torch

import trainer_loss_cases as cases
from mzx import _lib, trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return cases.golden(golden_dir)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c["name"])
def test_scalar_to_support_rows_bit_for_bit(be, gold, case):
    x = cases.inputs(case)
    for key in ("value", "reward"):
        rows = trainer.scalar_to_support(torch.from_numpy(x[f"target_{key}"]).to(be.device), case["S"])
        assert rows.is_cuda
        want = gold[f"{case['name']}/f32_support_{key}"]
        assert numpy.array_equal(rows.cpu().numpy().view(numpy.int32), want.view(numpy.int32))


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c["name"])
def test_loss_gradients_priorities(be, gold, case):
    x, got = cases.check_case(be, case, gold)
    again = cases.run_abi(be, case, x)                  # a second launch: identical bits in every output
    for key, value in got.items():
        assert numpy.array_equal(numpy.asarray(value).view(numpy.int32), numpy.asarray(again[key]).view(numpy.int32)), key
    plain = cases.run_abi(be, case, x, grads=False)     # evaluation only
    for key in ("loss", "value_loss", "reward_loss", "policy_loss", "priorities"):
        assert numpy.array_equal(numpy.asarray(plain[key]), numpy.asarray(got[key])), key


@pytest.mark.parametrize("case", cases.LIVE_CASES, ids=lambda c: c["name"])
def test_live_case_against_the_restatement(be, case):
    cases.check_live_case(be, case)


def test_muzero_loss_on_a_side_stream(be):
    case = cases.CASES[3]
    cfg = cases.config_of(case)
    x = cases.inputs(case)
    direct = cases.run_abi(be, case, x)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = {k: None if v is None else torch.from_numpy(v).to(be.device) for k, v in x.items()}
        v = t["value"].clone().requires_grad_()
        # the inputs are produced on the side stream right before the call: a launch on another stream would race them
        scaled = [(t["reward"] * 1.0), (t["policy"] + 0.0)]
        loss, _, _, _, priorities = trainer.muzero_loss(v, scaled[0], scaled[1], t["target_value"], t["target_reward"],
                                                        t["target_policy"], t["weight"], t["gradient_scale"], cfg)
        assert be.stream().value == side.cuda_stream
        loss.backward()
    side.synchronize()
    assert loss.item() == direct["loss"]
    assert numpy.array_equal(priorities.cpu().numpy(), direct["priorities"])
    assert numpy.array_equal(v.grad.cpu().numpy(), direct["grad_value"])


def test_update_weights_on_the_device(be):
    case = cases.CASES[2]
    cfg = cases.config_of(case)
    torch.manual_seed(5)
    ours = cases.TinyModel(6, 8, case["S"], case["A"]).to(be.device)
    theirs = cases.TinyModel(6, 8, case["S"], case["A"]).to(be.device)
    theirs.load_state_dict(ours.state_dict())
    opt_ours, opt_theirs = torch.optim.SGD(ours.parameters(), lr=1.0), torch.optim.SGD(theirs.parameters(), lr=1.0)
    batch = cases.training_batch(case)
    got = trainer.update_weights(ours, opt_ours, batch, cfg)
    want = cases.torch_update_weights(theirs, opt_theirs, batch, cfg)
    assert isinstance(got[0], numpy.ndarray) and got[0].dtype == numpy.float32 and got[0].shape == want[0].shape
    assert all(type(v) is float for v in got[1:])
    gate = 4 * cases.GRAD_ERROR_FLOOR * case["B"] * case["steps"]      # as in tests/test_trainer_loss.py
    for (name, a), b in zip(ours.named_parameters(), theirs.parameters()):
        err = (a - b).abs().max().item()
        print(f"{name}: {err:.3e} (gate {gate:.3e})")
        assert err <= gate, name
    assert numpy.abs(got[0] - want[0]).max() <= cases.DECODED_SCALAR_GATE ** cfg.PER_alpha
    assert numpy.allclose(got[1:], want[1:], rtol=1e-5, atol=cases.LOSS_ERROR_FLOOR)
