"""
The split-K GEMMs of the residual trainer on the device (tile_kernel<256, RtnKsplitGemmBody<MODE, WIDE>>,
csrc/mzx_train_gemm_ksplit.h): a handle with train_gemm = "ksplit_all" passes the case modules' own gates against the binary64
references, unchanged, and repeats its bits.  The cases are those of tests/test_gpu_train_gemm_tiled.py; what each one is the
smallest shape for in THIS body (a workgroup per 32 x 32 tile, k-group g of 16 to wave g & 3, partials joined through LDS):
  b_b3_k3           27 positions and 5 channels in one partial tile; K = 54: three full groups and a ragged one of 6, wave 3 gets
                    only the ragged group; the head GEMMs have K < 64: waves without a group; the virtual action channel
  c_b5_k4_stacked   N = 20 ragged inside a tile; a non-square board; the add / mask epilogue through the reduction's store
  d_b70_k3          many M tiles, the last partial; 18 weight-gradient chunks, the last of 116 positions = 7 groups + 4: the
                    waves get 2, 2, 2, 2 groups with a ragged eighth; weight-gradient N = 180
  wide72            C = 72: three N tiles, the last with 8 columns; K = 648 = 40 groups + 8
  sb_b3_k3          WIDE: the binary64 partials and join; stride-2 convolutions
  cb_b3_k3_stacked  WIDE with the 6 x 6 stride-4 kernel
"""
import numpy
import pytest

import resnet_train_cases as plain
from mzx import _lib
from test_gpu_train_gemm_tiled import CASES, WIDE72
from test_train_gemm_split import split_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.mark.parametrize("module,case", CASES, ids=[c["name"] for _, c in CASES])
def test_ksplit_all_meets_the_reference_gates(be, golden_dir, module, case):
    tables = split_tables(module, gemm="ksplit_all", matrix="f32")
    if case is WIDE72:
        net, got = plain.check_live(be, case, tables=tables)
    else:
        net, got = plain.check_case(be, case, module.golden(golden_dir), tables=tables)
    assert net.train_gemm == "ksplit_all" and next(net.parameters()).grad.is_cuda
    assert be.lib.mzx_train_resnet_ksplit_launches(net.handle, case["B"], case["steps"]) > 0
    again = plain.run_native(be, case, net, tables)
    for key, value in got.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(again[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key
