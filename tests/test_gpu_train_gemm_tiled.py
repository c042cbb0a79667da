"""
The LDS-tiled GEMMs of the residual trainer on the device (tile_kernel<256, RtnTileGemmBody<MODE, WIDE>>,
csrc/mzx_train_gemm_tiled.h): a handle with train_gemm = "tiled_all" passes the case modules' own gates against the binary64
reference, and every array of its step equals, bit for bit, the wave body's on a default handle of the same weights.

Each case is the smallest shape at which one mechanism of the tiled body can go wrong:
  b_b3_k3           27 positions and 5 channels in one partial workgroup tile; K = 54, neither a multiple of 32 nor of 16
                    (a ragged slab and a ragged quad); the virtual action channel
  c_b5_k4_stacked   N = 20 ragged inside a 64 tile; a non-square board; two blocks (the add / mask epilogue)
  d_b70_k3          8820 positions: many M workgroups, the last with 60 of 64 rows; 18 weight-gradient chunks, the last of
                    116 = 3 slabs + 20; weight-gradient N = 180 (three N tiles, the last ragged)
  wide72            C = 72 > 64: two N workgroup tiles forward and backward, two M tiles in the weight gradient, K = 648
  sb_b3_k3          WIDE with stride-2 3 x 3 convolutions and odd boards
  cb_b3_k3_stacked  WIDE with a 6 x 6 stride-4 kernel and 7 input planes
"""
import pytest

import resnet_stem_train_cases as stem
import resnet_train_cases as plain
import test_train_gemm_tiled as host_tests
from mzx import _lib

pytestmark = pytest.mark.gpu

WIDE72 = dict(name="wide72", B=2, steps=2, obs=(3, 3, 3), stacked=0, C=72, blocks=1, red=(2, 2, 2), rew=[4], val=[4], pol=[4],
              A=9, S=2, per=False, alpha=0.5, vlw=1.0, seed=35)
CASES = [(plain, plain.BY_NAME["b_b3_k3"]), (plain, plain.BY_NAME["c_b5_k4_stacked"]), (plain, plain.BY_NAME["d_b70_k3"]),
         (plain, WIDE72), (stem, stem.BY_NAME["sb_b3_k3"]), (stem, stem.BY_NAME["cb_b3_k3_stacked"])]


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.mark.parametrize("module,case", CASES, ids=[c["name"] for _, c in CASES])
def test_tiled_all_meets_the_reference_gates_with_the_wave_bits(be, golden_dir, module, case):
    tables = host_tests.tiled_tables(module)
    if case is WIDE72:
        net, got = plain.check_live(be, case, tables=tables)
    else:
        net, got = plain.check_case(be, case, module.golden(golden_dir), tables=tables)
    assert net.train_gemm == "tiled_all" and next(net.parameters()).grad.is_cuda
    host_tests.check_same_bits(be, case, module, got)
    host_tests.check_launch_counts(be, case, module)
