"""
Every output bit of mzx_train_fc_step on the device, for the five fixture cases, against the `device` section of
tests/golden/fc_train_bits.json (recorded on an MI355X; see tests/test_fc_train_bits.py).
"""
import pytest

import test_fc_train_bits as host_tests
from mzx import _lib

pytestmark = pytest.mark.gpu

pinned = host_tests.pinned


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


@pytest.mark.parametrize("case,tables", host_tests.CASES, ids=[case["name"] for case, _ in host_tests.CASES])
def test_device_step_reproduces_the_pinned_bits(be, pinned, case, tables):
    host_tests.check_bits(be, case, tables, pinned["device"])
