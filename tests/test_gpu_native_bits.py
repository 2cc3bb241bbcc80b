"""Every output bit of the native encode, decode, vanilla pull-back and LPIPS against tests/golden/native_bits.json, which
tools/gen_golden_native_bits.py wrote on the MI355X before their convolution core, pass planner and export helpers were
shared (native_bits_cases has the cases and why each size is there)."""
import json
import os

import pytest
import torch

import native_bits_cases as NB

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_bits.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("area,name", NB.ALL, ids=[f"{a}-{n}" for a, n in NB.ALL])
def test_bits_equal_the_recorded_ones(area, name):
    got = NB.run(area, name, torch.device("cuda", 0))
    recorded = {k: v for k, v in GOLDEN["cases"].items() if k.startswith(f"{area}/{name}/")}
    assert sorted(got) == sorted(recorded), "the fixture holds other cases: it belongs to another generator"
    for case, rec in recorded.items():
        assert got[case]["input"] == rec["input"], f"{case}: the input differs, the fixture belongs to another generator"
    for case, rec in recorded.items():
        assert got[case]["outputs"] == rec["outputs"], f"{case}: output bits differ from the recorded ones"
