"""The 1x1 convolution family (csrc/tdx_conv1*.hip) computes the bits it computed before its host side was rewritten around one
route, one plan per call and call records (csrc/tdx_conv1.h): every case of tests/conv1_bits_cases.py must reproduce the digest
in tests/golden/conv1_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the library of the commit
BEFORE that change.  One case per group stores the first elements of its outputs themselves, so a mismatch there is reported
in units of the last place.  The weight gradients are pinned under TDX_DETERMINISTIC=1 only: the atomic merge gives the bits
of its arrival order."""

import json

import pytest

import conv1_bits_cases as bits
import conv1_cases as cases
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / bits.FIXTURE).read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(bits.GROUPS)
    for g in bits.GROUPS:
        assert [n for n, rec in EXPECTED[g].items() if "bits" in rec] == [bits.BITS[g]]
    per_row = lambda table, names: {f"{n}/{d}" for n in names for d in cases.by_name(table, n).dtypes}
    assert set(EXPECTED["fwd"]) == per_row(cases.FWD, cases.FWD_INEXACT)
    assert set(EXPECTED["tail"]) == {f"{n}/{d}" for n in cases.TAIL_INEXACT for d in cases.H16}
    entries = ("tdx_conv1_bwd_weight/acc0", "tdx_conv1_bwd_weight_oc/acc0", "tdx_conv1_bwd_weight_oc/acc1")
    assert set(EXPECTED["wgrad"]) == {f"{r}/{e}" for r in per_row(cases.WGRAD, set(cases.WGRAD_INEXACT) | set(cases.NO_ARENA)) for e in entries}
    assert set(EXPECTED["wgrad_no_arena"]) == {f"{r}/{e}" for r in per_row(cases.WGRAD, cases.NO_ARENA) for e in entries}


@pytest.mark.gpu
@pytest.mark.parametrize("group", bits.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(bits.run(group), EXPECTED[group], group)
