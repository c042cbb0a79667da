"""
The split-BF16 tiled GEMMs of the residual trainer on the device (tile_kernel<256, RtnSplitGemmBody<MODE, WIDE>>,
csrc/mzx_train_gemm_split.h): a handle with train_gemm = "tiled_all" and train_matrix = "bf16x3" passes the case modules' own
gates against the binary64 references, unchanged, and repeats its bits.  The cases are those of
tests/test_gpu_train_gemm_tiled.py (see there what each one is the smallest shape for): the split body has the same tile,
the same slab of 32 k and the same chunks, so it is ragged where the tiled body is.
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
def test_split_meets_the_reference_gates(be, golden_dir, module, case):
    tables = split_tables(module)
    if case is WIDE72:
        net, got = plain.check_live(be, case, tables=tables)
    else:
        net, got = plain.check_case(be, case, module.golden(golden_dir), tables=tables)
    assert (net.train_gemm, net.train_matrix) == ("tiled_all", "bf16x3") and next(net.parameters()).grad.is_cuda
    assert be.lib.mzx_train_resnet_split_launches(net.handle, case["B"], case["steps"]) > 0
    again = plain.run_native(be, case, net, tables)
    for key, value in got.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(again[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key
