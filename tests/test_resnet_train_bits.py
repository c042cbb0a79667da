"""
Every output bit of mzx_train_resnet_step on the serial test double of the ABI, for the ten fixture cases of
resnet_train_cases and resnet_stem_train_cases, against the `serial` section of tests/golden/resnet_train_bits.json
(muzero-general_amd/tools/make_resnet_train_bits.py; the section names the commit it was recorded at).  A difference is a
changed sum or a changed contraction: find the expression, do not re-record.
"""
import importlib.util
import json
import os

import pytest

import hostcheck

_spec = importlib.util.spec_from_file_location("make_resnet_train_bits", os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "muzero-general_amd", "tools", "make_resnet_train_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

CASES = bits.fixture_cases()


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


@pytest.fixture(scope="module")
def pinned():
    with open(bits.FIXTURE) as f:
        return json.load(f)


def check_bits(be, case, tables, section):
    """The digests of the case's outputs are the section's; the assertion names the first output that differs."""
    want = section["cases"][case["name"]]
    assert sorted(want) == sorted(bits.PINNED)
    have = bits.digests(tables.run_native(be, case))
    differs = [key for key in bits.PINNED if have[key] != want[key]]
    assert not differs, f"{case['name']}: {differs[0]} differs from the bits recorded at {section['commit']} (all: {differs})"


def test_the_fixture_pins_every_case_on_both_builds(pinned):
    names = [case["name"] for case, _ in CASES]
    assert names == list(bits.PLAIN + bits.STEM) and len(names) == 10
    for backend in ("serial", "device"):
        assert sorted(pinned[backend]["cases"]) == sorted(names) and pinned[backend]["commit"]


@pytest.mark.parametrize("case,tables", CASES, ids=[case["name"] for case, _ in CASES])
def test_serial_step_reproduces_the_pinned_bits(be, pinned, case, tables):
    check_bits(be, case, tables, pinned["serial"])
