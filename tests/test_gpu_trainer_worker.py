"""
mzx.trainer.Trainer on the device: the worker loop of tests/test_trainer_worker.py (tests/trainer_worker_cases.py) in
chunks against a twin per-step loop, and the per-step route of a torch model.
"""
import pytest

import trainer_worker_cases as cases
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return _lib.default_backend()


def test_the_loop_in_chunks_publishes_what_a_per_step_loop_holds(be):
    me = cases.check_loop(be)
    assert me.model.flat_weights().is_cuda


def test_a_torch_model_takes_the_per_step_route(be):
    cases.check_torch_model_route(be)
