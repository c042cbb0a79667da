"""
The native optimizer step on the device (wave_kernel<4, OptimBody<...>> behind mzx_optim_step, csrc/mzx_optim.h): the
tables and checks of tests/test_native_optim.py (tests/optim_cases.py) -- bit for bit against the numpy float32
restatement of the definition, NaN in the skipped spans of every array, torch's own float32 error as the yardstick,
every refusal with nothing written.
"""
import pytest

import optim_cases as cases
import test_native_optim as host_tests
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_adam_is_the_definition_bit_for_bit(be, n):
    for row in cases.ADAM_ROWS:
        for seed, table in enumerate(t for t in host_tests.TABLES if t in cases.span_tables(n)):
            cases.check_adam_bits(be, n, table, row, seed)


@pytest.mark.parametrize("n", cases.LENGTHS)
def test_sgd_is_the_definition_bit_for_bit(be, n):
    for row in cases.SGD_ROWS:
        for seed, table in enumerate(t for t in host_tests.TABLES if t in cases.span_tables(n)):
            cases.check_sgd_bits(be, n, table, row, seed)


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
