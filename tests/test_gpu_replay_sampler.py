"""
Device-side prioritised sampling and priority feedback of the replay store on the MI355X (libmzx.so): the check functions
of tests/replay_sampler_cases.py -- the numpy oracle of the draw, bit for bit on dyadic priorities -- on the device
library.  Every case is a handful of launches on tiny buffers.
"""
import pytest

import replay_sampler_cases as cases
from mzx import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return _lib.default_backend()


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("slots", cases.SLOT_COUNTS)
def test_draws_bit_for_bit_on_the_device(backend, slots, per):
    cases.check_bit_exact(backend, slots, per)


def test_action_space_and_absorbing_tape_on_the_device(backend):
    cases.check_action_space(backend)


def test_boundaries_on_the_device(backend):
    cases.check_boundaries(backend)


def test_general_priorities_on_the_device(backend):
    cases.check_general(backend)


@pytest.mark.parametrize("case", cases.DEGENERATE)
def test_degenerate_priorities_on_the_device(backend, case):
    cases.check_degenerate(backend, case)


@pytest.mark.parametrize("steps", [1, 6])
def test_scatter_on_the_device(backend, steps):
    cases.check_scatter(backend, steps)


def test_store_upkeep_on_the_device(backend):
    cases.check_upkeep(backend)


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_end_to_end_on_the_device(backend, kind, per):
    cases.check_end_to_end(backend, kind, per)


def test_abi_refusals_on_the_device(backend):
    cases.check_abi_refusals(backend)
