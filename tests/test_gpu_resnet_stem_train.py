"""
Training a residual network WITH a downsample stem natively on the device (wave_kernel<4, RtnGemmBody<MODE, true>> on the
FP32 matrix pipes, the pool element kernels, mzx_net_set_train_stem) against tests/golden/resnet_stem_train.npz with the
gates and helpers of tests/test_resnet_stem_train.py, and breakout as shipped -- 96 x 96 -> 6 x 6, 9216 stem positions per
sample pair, 18 weight-gradient chunks, the real 8 / 16 channels -- against the torch restatement in binary64.
"""
import numpy
import pytest
import torch

import resnet_stem_train_cases as cases
import test_resnet_stem_train as host_tests
from mzx import _lib, configs, trainer
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


def test_two_sgd_momentum_steps_weights_and_buffers(be, gold):
    """Two steps at the gates of ``check_sgd``.  They leave the second step little room (the reference's own float32 run of
    these two steps misses them on a few tensors): the step has to be more exact than a float32 network, which is why a
    stem network keeps its BatchNorm statistics and GEMM sums in binary64 (csrc/mzx_train_resnet.h)."""
    cases.check_sgd(be, cases.BY_NAME["sc_b5_k2_stacked"], gold)


def test_the_switch(be):
    host_tests.check_switch(be)


def test_scratch_limit_names_the_attribute(be):
    host_tests.test_scratch_limit_names_the_attribute(be)


@pytest.mark.parametrize("field,value", host_tests.BAD, ids=[f"{f}={v}" for f, v in host_tests.BAD])
def test_abi_refusals_with_the_switch_on(be, field, value):
    host_tests.check_abi_refusal(be, field, value, device=be.device, sync=torch.cuda.synchronize)


def test_breakout_as_shipped_against_the_restatement_in_binary64_then_three_adam_steps(be):
    """B = 4, steps = 3 of configs.breakout(train_downsample=True), held to the torch restatement run here on the CPU in
    binary64, the reference's float32 error measured the same way; then three update_weights steps with Adam, after which
    the handle's inference is eval-mode inference of get_weights()."""
    cfg = configs.breakout(train_downsample=True, PER=True, PER_alpha=0.5, value_loss_weight=0.25)
    case = cases.case_of_config(cfg, 4, 3, name="breakout")
    net, got = cases.check_live(be, case)
    assert be.lib.mzx_train_resnet_launches(net.handle, 4, 3) > 0
    optimizer = torch.optim.Adam(net.parameters(), lr=0.003, weight_decay=1e-4)
    before = net.flat_weights().clone()
    for _ in range(3):
        out = trainer.update_weights(net, optimizer, cases.batch(case), cases.config_of(case))
        assert numpy.isfinite(out[0]).all() and all(numpy.isfinite(v) for v in out[1:])
    state = net.get_weights()
    assert torch.isfinite(net.flat_weights()).all() and not torch.equal(net.flat_weights(), before)
    for key, value in state.items():
        if key.endswith("num_batches_tracked"):
            assert int(value) == cases.tracked_after(key, case, 3), (key, int(value))
        elif cases.is_bypassed(key):      # the optimizer never moves what the stem bypasses
            off, numel = next((o, n) for k, o, n, _ in net._tensors if k == key)
            assert torch.equal(value.reshape(-1), before[off:off + numel].cpu()), key
    observation = torch.from_numpy(cases.batch(case)[0])
    oracle = net_oracle.make_oracle_network(cfg, state)
    want = oracle.initial_inference(observation)
    have = net.initial_inference(observation)
    for name, a, b in zip(("value", "reward", "policy", "state"), have, want):
        a, b = a.cpu().numpy().reshape(b.shape), b.numpy()
        finite = numpy.isfinite(b)
        assert numpy.array_equal(a[~finite], b[~finite]), name
        gap = float(numpy.abs(a[finite] - b[finite]).max())
        print(f"initial_inference {name} after three Adam steps: {gap:.3e} from eval-mode inference of get_weights()")
        assert gap <= 1e-4, name
