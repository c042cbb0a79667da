"""
Device-side prioritised sampling and priority feedback of the replay store on the serial build of the functors
(tests/hostcheck): the check functions of tests/replay_sampler_cases.py, which tests/test_gpu_replay_sampler.py runs on the
device library.  The scatter is held to the unmodified reference method here (the reference tree stays in the build
container), and the restatement the device suite uses is held to it alongside.
"""
import copy
import types

import numpy
import pytest

import hostcheck
import replay_sampler_cases as cases
from oracle import ref_shim


@pytest.fixture(scope="module")
def backend():
    return hostcheck.backend()


def test_philox_known_answers():
    cases.check_known_answers()


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("slots", cases.SLOT_COUNTS)
def test_draws_bit_for_bit(backend, slots, per):
    cases.check_bit_exact(backend, slots, per)


def test_action_space_and_absorbing_tape(backend):
    cases.check_action_space(backend)


def test_boundaries(backend):
    cases.check_boundaries(backend)


def test_general_priorities(backend):
    cases.check_general(backend)


@pytest.mark.parametrize("case", cases.DEGENERATE)
def test_degenerate_priorities(backend, case):
    cases.check_degenerate(backend, case)


def test_distribution(backend):
    cases.check_distribution(backend)


def reference_update(buffer, priorities, index_info):
    ref_shim.load()
    import replay_buffer as ref_rb
    cls = getattr(getattr(ref_rb.ReplayBuffer, "__ray_metadata__", None), "modified_class", ref_rb.ReplayBuffer)
    cls.update_priorities(types.SimpleNamespace(buffer=buffer), priorities, index_info)


@pytest.mark.reference
@pytest.mark.parametrize("steps", [1, 6])
def test_scatter_against_the_reference(backend, steps):
    cases.check_scatter(backend, steps, reference_update)
    games, index, new = cases.scatter_case(cases.sampler_config(True), steps)
    ours, theirs = copy.deepcopy(games), copy.deepcopy(games)
    cases.restated_update_priorities(ours, new, index)
    reference_update(theirs, new, index)
    for g in games:
        assert numpy.array_equal(ours[g].priorities, theirs[g].priorities) and ours[g].game_priority == theirs[g].game_priority


@pytest.mark.parametrize("steps", [1, 6])
def test_scatter(backend, steps):
    cases.check_scatter(backend, steps)


def test_store_upkeep(backend):
    cases.check_upkeep(backend)


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("kind", ["fc", "resnet"])
def test_end_to_end(backend, kind, per):
    cases.check_end_to_end(backend, kind, per)


def test_abi_refusals(backend):
    cases.check_abi_refusals(backend)
