"""
The support decode on the MI355X (tests/decode_cases.py holds the rows, the references and the checks;
tests/test_decode_edges.py is the CPU twin of parts 1 and 3's per-operator path).

  1. The entries that take logits -- mzx_support_to_scalar, the replay / reanalyse value decode, mzx_trainer_loss's
     priorities -- on exact rows (restate(x) bit for bit, -0.0 at x = 0) and dense families (a gate computed from the
     reference side), at supports 0 .. 300: one launch per entry and block of rows.
  2. Every search kernel on prescribed head rows: all-zero networks whose value and reward heads return an edge row at every
     node (tree_edge_cases.network_weights, kind `heads`), ten searches of 4 ragged trees x 3 simulations per (route, support).
     Root predicted values, the reward of every node but the root and the value of every node visited once carry the bits
     of mzx_support_to_scalar -- and of the restatement on the exact rows -- and the root's reward is -0.0.  The supports sit
     either side of the bin counts where the row decodes change code path: F = 15 | 17 (a partly empty 16-lane row),
     31 | 33 (row_decode2 / row_decode2x2 against row_decode_wide and LdsNet::decode's second pass), 63 | 65.
     The kernel that ran is asserted by name in every case.
Each case prints one line: route, support, kernel, rows, worst figure against its gate.
"""
import pytest

from mzx import _lib, configs, search

import decode_cases as cases
import test_gpu_continue_shapes as shapes
import test_gpu_parity as parity
import test_gpu_streamed as streamed
import test_gpu_tower_search as tower

pytestmark = pytest.mark.gpu

FC2, RT, RZ = "mzx::fc2_search_kernel", "mzx::rt_search_kernel", "mzx::rz_search_kernel"
RZ_WAVE, RZ_TILE = "mzx::rz_wave_search_kernel", "mzx::rz_tile_search_kernel"
ROWS = "row_select_kernel"
ONE_THREAD = "one-thread-per-tree"
PER_OPERATOR = "one kernel per step of a simulation"


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.fixture(autouse=True)
def _long_tape():
    old = search.TAPE_WORDS
    search.TAPE_WORDS = 4096      # (zero policy heads tie at every level; an overflowing tree would be searched again)
    try:
        yield
    finally:
        search.TAPE_WORDS = old


# ----------------------------------------------------------------------------- 1. entries that take logits

@pytest.mark.parametrize("S", cases.SUPPORTS)
def test_decode_entries_on_the_device(backend, S):
    cases.check_entries(backend, S)


# ----------------------------------------------------------------------------- 2. every search kernel

def _is(name):
    return lambda kernel: kernel == name


def _rows(kernel):
    return ROWS in kernel and ONE_THREAD not in kernel


def _per_operator(kernel):
    return ONE_THREAD in kernel or kernel.startswith(PER_OPERATOR)


ROW_NET = streamed.WAVE_SELECT_CASES["wide200"][0]      # a small convolutional network on a 4 x 8 board, 200 actions
RZ_NET = parity.RESNET_CASES["gomoku"]                  # 16 channels x 2 blocks on 11 x 11: the LDS-resident engine takes it
RT_NET = tower.CASES["wide32"]                          # 64 channels, one block, 4 x 8

def _route(make, support, mode, kernel, tuning=None, net_mode=None, actions=None):
    return dict(make=make, support=support, mode=mode, want_kernel=kernel, tuning=tuning or {}, net_mode=net_mode, actions=actions)


ROUTES = {
    # SmallNetCartpole: row_decode2x2, support_inverse_transform_2 and the 64-bit DPP chain
    "fc2-smallnet-s10": _route(configs.cartpole, 10, 3, _is(FC2)),
    # LdsNet::decode; cartpole forced onto it by mode flag 4
    "fc2-lds-cartpole-s10": _route(configs.cartpole, 10, 7, _is(FC2)),
}
for _A in (4, 16):
    for _S in (7, 8, 15, 16, 31):      # (16 and 31: F = 33 and 63, LdsNet::decode's third and fourth pass over the row)
        ROUTES[f"fc2-lds-a{_A}-s{_S}"] = _route(shapes._lds16(_A), _S, 3, _is(FC2))
for _S in (7, 15, 16):
    # rz_wave_plan declines more than 32 bins (row_decode2 only): rz_search_kernel runs instead; the tile kernel takes them
    # with row_decode_wide
    ROUTES[f"rz-wave-4x4-s{_S}"] = _route(parity.SMALL_BOARD_CASES["wave-4x4"][0], _S, 3, _is(RZ_WAVE if _S < 16 else RZ))
    ROUTES[f"rz-tile-3x6-s{_S}"] = _route(parity.SMALL_BOARD_CASES["tile-3x6"][0], _S, 3, _is(RZ_TILE))
# rz / rt / the row route.  Their narrow instantiations (row_decode2) need at most 16 actions AND at most 32 bins
# (row_action_lanes); everything else is the wide form (row_decode_wide).  16 actions at supports 15 | 16 sit either side of
# that border; the networks' own action counts (121, 32, 200) run the wide form at every support.
for _S in (15, 16, 32):
    for _A in (16, None) if _S < 32 else (None,):
        tag = f"-a{_A}" if _A else ""
        ROUTES[f"rz{tag}-s{_S}"] = _route(RZ_NET, _S, 1, _is(RZ), {"wide_towers": 0}, actions=_A)
        ROUTES[f"rt{tag}-s{_S}"] = _route(RT_NET, _S, 1, _is(RT), {"rt_search": 1}, actions=_A)
        ROUTES[f"row-per-tree{tag}-s{_S}"] = _route(ROW_NET, _S, 1, _rows, {"rt_search": 0, "wave_select": 0}, 3, actions=_A)
        ROUTES[f"wave-per-tree{tag}-s{_S}"] = _route(ROW_NET, _S, 1, _rows, {"rt_search": 0, "wave_select": 1}, 3, actions=_A)
for _S in cases.SUPPORTS:
    ROUTES[f"per-operator-s{_S}"] = _route(shapes._lds16(4), _S, 0, _per_operator)


@pytest.mark.parametrize("route", list(ROUTES))
def test_decode_in_search_kernels(backend, route):
    cases.check_search(backend, route=route, **ROUTES[route])
