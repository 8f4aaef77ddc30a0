"""The reverse-step, loss and Philox kernels of csrc/tdx_ddpm.hip compute the bits they computed before they were
rewritten over shared skeletons: every case of tests/reverse_step_cases.py must reproduce the digest in
tests/golden/reverse_step_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the
library of the commit BEFORE that change.  For the smallest shape the fixture holds the outputs themselves, so a mismatch
there is reported in units of the last place."""

import json

import pytest

import reverse_step_cases as cases
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / cases.FIXTURE).read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(cases.GROUPS)


@pytest.mark.gpu
@pytest.mark.parametrize("group", cases.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(cases.run(group), EXPECTED[group], group)
