"""
The LDS-tiled GEMM route of the residual trainer (mzx_net_set_train_gemm, csrc/mzx_train_gemm_tiled.h) on the serial test
double of the ABI: the switch, the launch-count invariants, and mode 2 reproducing mode 0's bits.  The helpers are shared
with tests/test_gpu_train_gemm_tiled.py.
"""
import types

import numpy
import pytest

import fc_train_cases
import hostcheck
import resnet_train_cases as plain
from mzx import _lib, models


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


def tiled_tables(module):
    """The case module with ``network()`` sending every GEMM of the step to the tiled body."""
    def network(be, case, **kw):
        net = module.network(be, case, **kw)
        net.train_gemm = "tiled_all"
        return net
    return types.SimpleNamespace(**{**vars(module), "network": network})


def check_same_bits(be, case, module, tiled):
    """Every array of ``run_native`` from the tiled_all handle's step against a default handle of the same weights."""
    wave = plain.run_native(be, case, tables=module)
    assert sorted(wave) == sorted(tiled)
    for key, value in wave.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(tiled[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key


def check_launch_counts(be, case, module):
    lib, size = be.lib, (case["B"], case["steps"])
    net = module.network(be, case)
    wave = (lib.mzx_train_resnet_launches(net.handle, *size), lib.mzx_train_resnet_scratch_bytes(net.handle, *size))
    assert wave[0] > 0 and wave[1] > 0 and lib.mzx_train_resnet_tiled_launches(net.handle, *size) == 0
    net.train_gemm = "tiled_all"
    assert 0 < lib.mzx_train_resnet_tiled_launches(net.handle, *size) < wave[0]
    assert (lib.mzx_train_resnet_launches(net.handle, *size), lib.mzx_train_resnet_scratch_bytes(net.handle, *size)) == wave
    net.train_gemm = "tiled"      # the rule's share lies between none and all; an unsupported size counts nothing
    assert 0 <= lib.mzx_train_resnet_tiled_launches(net.handle, *size) < wave[0]
    assert lib.mzx_train_resnet_tiled_launches(net.handle, 0, 3) == 0 and lib.mzx_train_resnet_tiled_launches(None, 4, 3) == 0


def test_the_switch(be):
    lib, case = be.lib, plain.BY_NAME["b_b3_k3"]
    net = plain.network(be, case)
    assert lib.mzx_net_train_gemm(net.handle) == 0 and net.train_gemm == "wave"
    for mode, name in enumerate(models.HipNetwork.TRAIN_GEMM_MODES):
        assert lib.mzx_net_set_train_gemm(net.handle, mode) == 0
        assert lib.mzx_net_train_gemm(net.handle) == mode and net.train_gemm == name
    for bad in (-1, 3):
        assert lib.mzx_net_set_train_gemm(net.handle, bad) == -1 and b"mzx_net_set_train_gemm" in lib.mzx_last_error()
        assert net.train_gemm == "tiled_all"
    with pytest.raises(ValueError):
        net.train_gemm = "lds"
    assert lib.mzx_net_set_train_gemm(None, 1) == -1 and lib.mzx_net_train_gemm(None) == 0
    fc = fc_train_cases.network(be, fc_train_cases.CASES[1])
    assert lib.mzx_net_set_train_gemm(fc.handle, 1) == -1 and lib.mzx_net_train_gemm(fc.handle) == 0
    with pytest.raises(_lib.MzxError):
        fc.train_gemm = "tiled"
    # config.train_gemm reaches the handle; without it the default is the wave body
    assert models.MuZeroNetwork(plain.config_of(case, train_gemm="tiled"), _backend=be).train_gemm == "tiled"
    assert models.MuZeroNetwork(plain.config_of(case), _backend=be).train_gemm == "wave"


def test_tiled_all_reproduces_the_wave_bits(be):
    case = plain.BY_NAME["b_b3_k3"]
    check_same_bits(be, case, plain, plain.run_native(be, case, tables=tiled_tables(plain)))


def test_launch_counts_do_not_depend_on_the_route(be):
    check_launch_counts(be, plain.BY_NAME["b_b3_k3"], plain)
