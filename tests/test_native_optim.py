"""
The native optimizer step (mzx_optim_step, csrc/mzx_optim.h) on the serial test double of the ABI: bit for bit against the
numpy float32 restatement of the definition in include/mzx.h over every flat length, span table and hyperparameter row of
tests/optim_cases.py; against torch within torch's own float32 error; every refusal.
"""
import ctypes

import numpy
import pytest

import hostcheck
import optim_cases as cases
from mzx import _lib


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


TABLES = ("whole", "alternating", "skipped_ends", "empty_spans", "reversed")


@pytest.mark.parametrize("row", cases.ADAM_ROWS, ids=lambda r: r["name"])
@pytest.mark.parametrize("n", cases.LENGTHS)
def test_adam_is_the_definition_bit_for_bit(be, n, row):
    for seed, table in enumerate(t for t in TABLES if t in cases.span_tables(n)):
        cases.check_adam_bits(be, n, table, row, seed)


@pytest.mark.parametrize("row", cases.SGD_ROWS, ids=lambda r: r["name"])
@pytest.mark.parametrize("n", cases.LENGTHS)
def test_sgd_is_the_definition_bit_for_bit(be, n, row):
    for seed, table in enumerate(t for t in TABLES if t in cases.span_tables(n)):
        cases.check_sgd_bits(be, n, table, row, seed)


def test_every_table_is_exercised():
    assert set(cases.span_tables(4099)) == set(TABLES)
    assert not cases.live_mask(4099, cases.span_tables(4099)["alternating"])[[1, 2, 6, 10]].any()


@pytest.mark.parametrize("n", [65, 1025])
def test_arrays_off_the_16_byte_grid_take_the_scalar_path(be, n):
    for table in ("whole", "alternating"):
        cases.check_adam_bits(be, n, table, cases.ADAM_ROWS[3], misaligned=True)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_nan_gradient_stays_in_its_element(be, kind):
    cases.check_nan_gradient(be, kind)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_four_steps_within_four_times_torchs_own_float32_error(be, kind):
    cases.check_against_torch(be, kind)


@pytest.mark.parametrize("what", cases.REFUSALS)
def test_refusals_write_nothing(be, what):
    cases.check_refusal(be, what)


def test_null_io_is_refused(be):
    assert be.lib.mzx_optim_step(None, None) == -1
    assert be.lib.mzx_optim_chunks(None, 1, 8, None, 0) == -1


def test_chunks_are_cut_at_absolute_multiples_of_the_chunk_size(be):
    spans = numpy.asarray([(1000, 2000), (5, 0), (3000, 1)], dtype=numpy.int64)
    out = numpy.zeros((8, 2), dtype=numpy.int64)
    count = be.lib.mzx_optim_chunks(spans.ctypes.data, 3, 4099, out.ctypes.data, 8)
    assert _lib.OPTIM_CHUNK == 1024 and count == 4
    assert out[:count].tolist() == [[1000, 24], [1024, 1024], [2048, 952], [3000, 1]]
    short = numpy.zeros((2, 2), dtype=numpy.int64)      # a short array: the count is returned, nothing is written past it
    assert be.lib.mzx_optim_chunks(spans.ctypes.data, 3, 4099, short.ctypes.data, 1) == 4
    assert short.tolist() == [[1000, 24], [0, 0]]


def test_io_struct_matches_the_header():
    assert ctypes.sizeof(_lib.OptimIO) == 4 * 2 + 8 + 4 * 8 + 8 + 2 * 8 + 2 * 4 + 9 * 8
