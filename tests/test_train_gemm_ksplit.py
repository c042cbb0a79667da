"""
The split-K GEMM route of the residual trainer (mzx_net_set_train_gemm_route modes 3 and 4, csrc/mzx_train_gemm_ksplit.h) on the
serial test double of the ABI, which restates the body's summation order (four per-wave sums over every fourth k-group, joined
(w0 + w1) + (w2 + w3)): the reference gates, the launch-count identities, and the default bits that must not move.
"""
import pytest

import hostcheck
import resnet_stem_train_cases as stem
import resnet_train_cases as plain
from mzx import models
from test_gpu_train_gemm_tiled import WIDE72
from test_train_gemm_split import split_tables
from test_train_gemm_tiled import check_same_bits


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


def test_the_route_switch(be):
    lib = be.lib
    net = plain.network(be, plain.BY_NAME["b_b3_k3"])
    assert models.HipNetwork.TRAIN_GEMM_ROUTES == ("wave", "tiled", "tiled_all", "ksplit", "ksplit_all")
    for mode, name in enumerate(models.HipNetwork.TRAIN_GEMM_ROUTES):
        assert lib.mzx_net_set_train_gemm_route(net.handle, mode) == 0
        assert lib.mzx_net_train_gemm(net.handle) == mode and net.train_gemm == name
    for bad in (-1, 5):
        assert lib.mzx_net_set_train_gemm_route(net.handle, bad) == -1 and b"mzx_net_set_train_gemm_route" in lib.mzx_last_error()
        assert net.train_gemm == "ksplit_all"
    assert lib.mzx_net_set_train_gemm_route(None, 3) == -1
    assert models.MuZeroNetwork(plain.config_of(plain.BY_NAME["b_b3_k3"], train_gemm="ksplit"), _backend=be).train_gemm == "ksplit"


# (plain: one fmaf chain per wave; stem: WIDE, the binary64 partials and join)
@pytest.mark.parametrize("module,name", [(plain, "b_b3_k3"), (stem, "sb_b3_k3")], ids=["b_b3_k3", "sb_b3_k3"])
def test_ksplit_all_meets_the_reference_gates_and_repeats_its_bits(be, golden_dir, module, name):
    # (check_case runs the step twice on one handle and compares every bit)
    tables = split_tables(module, gemm="ksplit_all", matrix="f32")
    net, _ = plain.check_case(be, module.BY_NAME[name], module.golden(golden_dir), tables=tables)
    assert net.train_gemm == "ksplit_all"
    assert be.lib.mzx_train_resnet_ksplit_launches(net.handle, module.BY_NAME[name]["B"], module.BY_NAME[name]["steps"]) > 0


@pytest.mark.parametrize("case", [plain.BY_NAME["b_b3_k3"], WIDE72], ids=["b_b3_k3", "wide72"])
def test_launch_count_identities(be, case):
    lib = be.lib
    size = (case["B"], case["steps"])
    net = plain.network(be, case)

    def counts(mode):
        net.train_gemm = mode
        return (lib.mzx_train_resnet_tiled_launches(net.handle, *size), lib.mzx_train_resnet_ksplit_launches(net.handle, *size),
                lib.mzx_train_resnet_launches(net.handle, *size), lib.mzx_train_resnet_scratch_bytes(net.handle, *size))

    wave, tiled, tiled_all, ksplit, ksplit_all = (counts(mode) for mode in models.HipNetwork.TRAIN_GEMM_ROUTES)
    gemms = tiled_all[0]
    assert wave[:2] == (0, 0) and tiled[1] == 0 and tiled_all[1] == 0 and 0 <= tiled[0] <= gemms > 0
    assert ksplit_all[:2] == (0, gemms)
    assert ksplit[0] == tiled[0] and ksplit[0] + ksplit[1] <= gemms
    assert {c[2:] for c in (tiled, tiled_all, ksplit, ksplit_all)} == {wave[2:]}
    assert lib.mzx_train_resnet_ksplit_launches(net.handle, 0, 3) == 0 and lib.mzx_train_resnet_ksplit_launches(None, 3, 3) == 0
    if case is WIDE72:      # 72 channels, 36 positions over both steps: the rule picks the prediction tower's GEMMs, not the heads'
        assert 0 < ksplit[1] < gemms
    else:      # 5 channels: no full 32 x 32 tile anywhere
        assert ksplit[1] == 0


@pytest.mark.parametrize("mode", ["ksplit", "ksplit_all"])
def test_a_default_handle_keeps_its_bits_after_the_mode_was_set_and_set_back(be, mode):
    case = plain.BY_NAME["b_b3_k3"]
    net = plain.network(be, case)
    net.train_gemm = mode
    plain.run_native(be, case, net)
    net.train_gemm = "wave"
    check_same_bits(be, case, plain, plain.run_native(be, case, net))
