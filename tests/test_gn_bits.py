"""The streaming GroupNorm kernels of csrc/tdx_groupnorm.hip and the codec kernels that share their element with the two fused
tails compute the bits they computed before they were rewritten over one streaming skeleton: every case of tests/gn_cases.py
must reproduce the digest in tests/golden/gn_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the
library of the commit BEFORE that change.  At V = 5 the fixture holds the outputs themselves, so a mismatch there is reported
in units of the last place."""

import json

import pytest

import gn_cases as cases
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / cases.FIXTURE).read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(cases.GROUPS)


@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_shapes_reach_their_branches(shape):
    """The grid rule still puts each shape on the loop branches it was chosen for (blocks, stride, spare threads, and whether
    lanes run a full trip, the tail loop, or one after the other)."""
    B, C, G, V = shape
    assert cases.lane_paths(B, C, V) == cases.SHAPES[shape]


def test_fused_tails_run_at_their_partners_shapes():
    for B, D, with_c, G, V in cases.ENCODED:
        C = 2 * D if with_c else D
        assert cases.lane_paths(B, C, V)[3] == ({cases.TAIL} if V == 5 else {cases.TRIP, cases.TAIL})
    for B, C, G, V in cases.DECODE:
        L = C // 8
        assert L & (L - 1) == 0 and cases.lane_paths(B, C, V)[3] == {cases.TRIP, cases.TAIL}
    assert max(C for _, C, _, _ in cases.DECODE) == 512  # L = 64: the butterfly spans the wave


@pytest.mark.gpu
@pytest.mark.parametrize("group", cases.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(cases.run(group), EXPECTED[group], group)
