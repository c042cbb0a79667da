"""
CPU anchor of the tree edge cases (tests/tree_edge_cases.py): the per-operator tree operators (csrc/mzx_tree.h, compiled
serially by tests/hostcheck) through the lock-step ABI on GENERATED tables of network outputs, against the CPU oracle,
bit for bit -- action widths 1 .. 361 across every chunk border of the lane-parallel kernels, A-way root ties whose draws
reject tape words, pairs of equal maxima astride a border, walks through the last slot as deep as the search is long,
values of order 1e5, a search whose min-max bounds never separate, the visit tables used up to 800.
The GPU twin (and the tuned kernels against this path) is tests/test_gpu_tree_edges.py.
"""
import pytest

import hostcheck
import tree_edge_cases as edges


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


@pytest.mark.parametrize("name", [c["name"] for c in edges.LOCKSTEP_CASES])
def test_tree_edges_lockstep_bit_exact(backend, name):
    edges.check_lockstep(backend, edges.LOCKSTEP_BY_NAME[name], report=print)
