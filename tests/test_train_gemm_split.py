"""
The split-BF16 arithmetic of the residual trainer's tiled GEMM route (mzx_net_set_train_matrix, csrc/mzx_train_gemm_split.h)
on the serial test double of the ABI: the switch, the counters, the reference gates, and the bits that must not move.
``network`` is shared with tests/test_gpu_train_gemm_split.py.
"""
import types

import numpy
import pytest

import fc_train_cases
import hostcheck
import resnet_train_cases as plain
from mzx import _lib, models
from test_train_gemm_tiled import check_same_bits


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


def split_tables(module, gemm="tiled_all", matrix="bf16x3"):
    """The case module with ``network()`` setting the two switches of the handle."""
    def network(be, case, **kw):
        net = module.network(be, case, **kw)
        net.train_gemm, net.train_matrix = gemm, matrix
        return net
    return types.SimpleNamespace(**{**vars(module), "network": network})


def test_the_switch(be):
    lib, case = be.lib, plain.BY_NAME["b_b3_k3"]
    net = plain.network(be, case)
    assert lib.mzx_net_train_matrix(net.handle) == 0 and net.train_matrix == "f32"
    for mode, name in enumerate(models.HipNetwork.TRAIN_MATRIX_MODES):
        assert lib.mzx_net_set_train_matrix(net.handle, mode) == 0
        assert lib.mzx_net_train_matrix(net.handle) == mode and net.train_matrix == name
    for bad in (-1, 2):
        assert lib.mzx_net_set_train_matrix(net.handle, bad) == -1 and b"mzx_net_set_train_matrix" in lib.mzx_last_error()
        assert net.train_matrix == "bf16x3"
    with pytest.raises(ValueError):
        net.train_matrix = "bf16"
    assert lib.mzx_net_set_train_matrix(None, 1) == -1 and lib.mzx_net_train_matrix(None) == 0
    fc = fc_train_cases.network(be, fc_train_cases.CASES[1])
    assert lib.mzx_net_set_train_matrix(fc.handle, 1) == -1 and lib.mzx_net_train_matrix(fc.handle) == 0
    with pytest.raises(_lib.MzxError):
        fc.train_matrix = "bf16x3"
    assert models.MuZeroNetwork(plain.config_of(case, train_matrix="bf16x3"), _backend=be).train_matrix == "bf16x3"
    assert models.MuZeroNetwork(plain.config_of(case), _backend=be).train_matrix == "f32"


def test_counters(be):
    lib, case = be.lib, plain.BY_NAME["b_b3_k3"]
    size = (case["B"], case["steps"])
    net = plain.network(be, case)
    base = (lib.mzx_train_resnet_launches(net.handle, *size), lib.mzx_train_resnet_scratch_bytes(net.handle, *size))
    for matrix in models.HipNetwork.TRAIN_MATRIX_MODES:      # the wave body never splits
        net.train_matrix = matrix
        assert lib.mzx_train_resnet_split_launches(net.handle, *size) == 0
    net.train_gemm = "tiled_all"
    assert 0 < lib.mzx_train_resnet_split_launches(net.handle, *size) == lib.mzx_train_resnet_tiled_launches(net.handle, *size)
    assert (lib.mzx_train_resnet_launches(net.handle, *size), lib.mzx_train_resnet_scratch_bytes(net.handle, *size)) == base
    assert lib.mzx_train_resnet_split_launches(net.handle, 0, 3) == 0 and lib.mzx_train_resnet_split_launches(None, 3, 3) == 0
    net.train_matrix = "f32"
    assert lib.mzx_train_resnet_split_launches(net.handle, *size) == 0 < lib.mzx_train_resnet_tiled_launches(net.handle, *size)


def test_split_meets_the_reference_gates_and_repeats_its_bits(be, golden_dir):
    # (check_case runs the step twice on one handle and compares every bit)
    net, _ = plain.check_case(be, plain.BY_NAME["b_b3_k3"], plain.golden(golden_dir), tables=split_tables(plain))
    assert (net.train_gemm, net.train_matrix) == ("tiled_all", "bf16x3")


def test_matrix_f32_keeps_the_default_bits(be):
    case = plain.BY_NAME["b_b3_k3"]
    check_same_bits(be, case, plain, plain.run_native(be, case, tables=split_tables(plain, matrix="f32")))
    # and the split step is another arithmetic: some bit of some gradient differs from the default handle's
    wave, split = plain.run_native(be, case), plain.run_native(be, case, tables=split_tables(plain))
    assert any(not numpy.array_equal(wave[k], split[k]) for k in wave if k.startswith("grad/"))
