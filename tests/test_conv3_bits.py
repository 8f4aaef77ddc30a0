"""The brick kernels of the 3x3x3 forward / data gradient (csrc/tdx_conv3_mfma.hip, tdx_conv3_mfma_f32.hip,
tdx_conv3_mfma_split*.hip) and the remainder slabs of the ring kernel compute the bits they computed before they were moved
onto one brick view and one epilogue (csrc/tdx_conv3_brick.h, tdx_conv3_epilogue.h): every case of tests/conv3_cases.py must
reproduce the digest in tests/golden/conv3_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the
library of the commit BEFORE that change.  At each group's smallest shape the fixture holds a part of the outputs themselves, so
a mismatch there is reported in units of the last place."""

import json

import pytest

import conv3_cases as cases
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / cases.FIXTURE).read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(cases.GROUPS)
    for group, recs in EXPECTED.items():
        assert sum("bits" in r for r in recs.values()) <= 1, group  # the smallest shape only; none of the large grids


@pytest.mark.parametrize("shape", list(cases.SMALL))
def test_small_grids_reach_their_plans(shape):
    """The case table only: by the Python restatement of the planning rules (cases.plan16 / plan32, not the host code) each
    small grid has the permutation its comment names and no thin slabs."""
    B, grid = shape
    assert cases.plan16(grid) == cases.SMALL[shape]
    assert cases.plan32(B, grid, True) == (False, False, False)


def test_large_grids_reach_their_plans():
    """The case table only: the voxel and brick counts its comments quote, and what the restated rules make of them.  That
    the data gradient of these shapes runs on the brick kernels at all is asserted case by case (conv3_cases._conv_case)."""
    B, grid = cases.THIN16
    assert grid[0] * grid[1] * grid[2] == 69564 and cases.plan16(grid)[1] == (True, True, True)
    B, grid = cases.THIN32
    assert B * cases.bricks(grid, (0, 1, 2)) == 1275
    assert cases.plan32(B, grid, True) == (True, True, True) and cases.plan32(B, grid, False) == (False, False, False)
    B, grid = cases.BIG
    assert B * cases.bricks(grid, (0, 1, 2), (8, 8, 8)) == 1024  # the split launcher's threshold for 8 x 8 x 8 bricks
    for B, C1, C2, Co, grid, depth in cases.RING:  # the ring kernel leaves a remainder of 1-2 voxels on some axis
        assert any(1 <= e % b <= 2 for e, b in zip(grid, (8, 8, depth)))


@pytest.mark.gpu
@pytest.mark.parametrize("group", cases.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(cases.run(group), EXPECTED[group], group)
