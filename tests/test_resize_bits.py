"""The trilinear resize (csrc/tdx_resize.hip) computes the bits it computed before its host side was rewritten around one plan
per call and its three tiled kernels around one frame: every case of tests/resize_bits_cases.py must reproduce the digest in
tests/golden/resize_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the library of the commit
BEFORE that change.  One case per group stores the first elements of its outputs themselves, so a mismatch there is reported
in units of the last place."""

import json

import pytest

import resize_bits_cases as bits
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / bits.FIXTURE).read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(bits.GROUPS)
    for g in bits.GROUPS:
        assert sorted(EXPECTED[g]) == sorted(bits.names(g))
        assert [n for n, rec in EXPECTED[g].items() if "bits" in rec] == [bits.BITS[g]]
    # the first group's raw bits hold every element of the smallest case: 1 x 8, (1, 1, 1) -> (3, 4, 5) in float32
    assert [len(b) // 8 for b in EXPECTED["pairs"][bits.BITS["pairs"]]["bits"]] == [3 * 4 * 5 * 8, 8, 8]


def test_cases_reach_every_route():
    rows = [c for g in bits.GROUPS for c in bits.ROWS[g]]
    assert {c.fwd for c in rows} == {"pairs", "gather"} and {c.bwd for c in rows} == {2, 4, 6, 12, "generic"}
    assert {c.fwd_tile for c in rows if c.fwd == "pairs"} >= {(4, 8, 8), (2, 8, 8)}
    assert all({"f32", "bf16"} <= set(c.dtypes) for c in rows)


@pytest.mark.gpu
@pytest.mark.parametrize("group", bits.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(bits.run(group), EXPECTED[group], group)
