"""The *_workspace_bytes answers recorded in tests/golden/native_bits.json (no device needed): the query side of the pass
planner that the native encode, decode, pull-back and LPIPS share."""
import json
import os

import pytest

import native_bits_cases as NB

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_covers_every_configuration():
    assert GOLDEN["workspace_n"] == list(NB.WORKSPACE_N)
    assert sorted(GOLDEN["workspace_bytes"]) == sorted(f"{a}/{n}" for a, n in NB.ALL)


@pytest.mark.parametrize("area,name", NB.ALL, ids=[f"{a}-{n}" for a, n in NB.ALL])
def test_workspace_bytes_equal_the_recorded_ones(area, name):
    assert NB.workspace_answers(area, name) == GOLDEN["workspace_bytes"][f"{area}/{name}"]
