"""
The support decode -- soft-max, expectation, inverse value transform -- on the serial build (tests/hostcheck), at the rows
where a decode goes wrong without a 3e-4 gate noticing: exact rows (one-hot, pairs, four bins, both ends of the support,
x = 0), whose decode is the float32 restatement of the transform bit for bit, and dense families held to a gate computed
from the reference side (tests/decode_cases.py).  tests/test_gpu_decode_edges.py runs the same checks on the device and
adds every tuned search kernel.
"""
import numpy
import pytest

import decode_cases as cases
import hostcheck

import test_gpu_continue_shapes as shapes


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


def test_rows_are_what_they_claim():
    """The generators: the exact rows' soft-max is exactly 1 / n on the on bins in float32 and binary64 alike, x is on the
    quarter grid, both ends and zero are present; the edge rows are ten from support 2 on; the restatement is -0.0 at zero."""
    assert cases.bits(cases.restate([0.0]))[0] == 0x80000000
    for S in cases.SUPPORTS:
        rows, xs = cases.exact_rows(S)
        assert rows.dtype == xs.dtype == numpy.float32 and rows.shape == (len(xs), 2 * S + 1) and len(xs) <= cases.ROW_CAP + 8
        e = numpy.exp((rows - rows.max(1, keepdims=True)).astype(numpy.float32))
        assert set(numpy.unique(e)) <= {numpy.float32(0), numpy.float32(1)} and set(e.sum(1)) <= {1, 2, 4}
        x = (e / e.sum(1, keepdims=True) * numpy.arange(-S, S + 1, dtype=numpy.float32)).sum(1)
        assert numpy.array_equal(x, xs)
        assert {-S, 0, S} <= set(xs.tolist()) and (S == 0 or {-0.5, 0.5} <= set(xs.tolist()))
        half = len(xs) // 2
        assert numpy.array_equal(xs[:half], xs[half:]) and rows[:half].min() >= -200 and (S == 0 or rows[half:].min() == numpy.float32(-1e30))
        er, ex, names = cases.edge_rows(S)
        want = {0: [0], 1: [-1, 0, 1, 0.5, -0.5]}.get(S, [-S, -1, 0, 1, S, 0.5, -0.5, 0.25])
        assert er.shape == (len(want) + 2, 2 * S + 1) and [x for x in ex if x is not None] == want
        fam = cases.dense_rows(S)
        assert set(fam) == (set(cases.FAMILIES) if S else {"n3", "n20", "equal", "mirror"})


@pytest.mark.parametrize("S", cases.SUPPORTS)
def test_decode_entries(backend, S):
    """mzx_support_to_scalar: restate(x) bit for bit on the exact rows, -0.0 at x = 0, the gate on the dense rows; the
    replay / reanalyse decode and the trainer's priorities: mzx_support_to_scalar's bits on every row."""
    cases.check_entries(backend, S)


# ---- the per-operator path (mode 0) through the serial build: the decode inside a search

@pytest.mark.parametrize("S", cases.SUPPORTS)
def test_decode_in_per_operator_search(backend, S):
    cases.check_search(backend, shapes._lds16(4), S, 0, {}, "per-operator (serial build)",
                       lambda kernel: "one-thread-per-tree" in kernel or kernel.startswith("one kernel per step"), backend_arg=True)


# ---- the unmodified reference

@pytest.mark.reference
def test_reference_meets_the_gate():
    """models.support_to_scalar of the reference tree on the exact and dense rows against binary64, under the same gate.
    How many exact rows differ from the restatement in bits is printed, not asserted: torch is no bit reference."""
    import torch
    from oracle import ref_shim

    ref_models, _ = ref_shim.load()
    for S in cases.SUPPORTS:
        rows, xs = cases.exact_rows(S)
        got = ref_models.support_to_scalar(torch.from_numpy(numpy.array(rows)), S).numpy().reshape(-1)
        assert numpy.isfinite(got).all()
        err, g = cases.rel_error(got, cases.truth(rows, S)), cases.YARDSTICK_FACTOR * cases.e_transform(S)
        differ = int((cases.bits(got) != cases.bits(cases.restate(xs))).sum())
        print(f"decode_edges reference support {S} exact: error {err:.3e} gate {g:.3e}; {differ} of {len(xs)} rows differ from the restatement in bits")
        assert err <= g, (S, err, g)
        dense, _ = cases.dense_block(S)
        cases.check_dense(ref_models.support_to_scalar(torch.from_numpy(numpy.array(dense)), S).numpy(), S, "reference models.support_to_scalar")
