"""The general 3-D convolution family (csrc/tdx_convg*.hip) computes the bits it computed before its geometry, index arithmetic
and epilogue were written once in csrc/tdx_convg.h: every case of tests/convg_cases.py must reproduce the digest in
tests/golden/convg_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the library of the commit
BEFORE that change.  One case per group stores the first elements of its outputs themselves, so a mismatch there is reported
in units of the last place.  The weight gradients run on integer operands and must also EQUAL the float64 gradients of F.conv3d on the CPU: that
check needs no fixture."""

import json

import pytest
import torch

import convg_cases as cases
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / cases.FIXTURE).read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(cases.GROUPS)
    assert all(any("bits" in rec for rec in EXPECTED[g].values()) for g in cases.GROUPS)


def _rows(test):
    return list(next(m for m in test.pytestmark if m.name == "parametrize" and m.args[0] == "case").args[1])


def test_cases_are_the_rows_of_the_tolerance_tests():
    import test_baseline_convs as T

    assert cases.MFMA_CONV == _rows(T.test_conv3d_matrix_core_kernels_vs_oracle)
    assert cases.MFMA_DECONV == _rows(T.test_conv_transpose3d_matrix_core_kernels_vs_oracle)
    assert cases.VECTOR == _rows(T.test_conv3d_general_vs_oracle)


@pytest.mark.parametrize("name", list(cases.WGRAD))
def test_wgrad_reference_sums_are_exact_in_fp32(name):
    """The premise of the wgrad group: every reference gradient is an integer below 2^24 (so is every partial sum: |x dy| <= 9
    and there are fewer than 2^24 / 9 rows), hence fp32 adds them exactly in any order."""
    _, _, row = cases.WGRAD[name]
    x, gy, _ = cases._wgrad_operands(name)
    assert 9 * gy[:, 0].numel() < 2**24 and x.abs().max() <= 3 and gy.abs().max() <= 3
    for g in cases.wgrad_reference(name):
        if g is not None:
            assert torch.equal(g, g.round()) and g.abs().max() < 2**24 and g.abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("group", cases.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(cases.run(group), EXPECTED[group], group)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.WGRAD))
def test_wgrad_equals_float64_reference(name):
    for got, want in zip(cases.wgrad_outputs(name), cases.wgrad_reference(name)):
        assert (got is None) == (want is None)
        if want is not None:
            assert torch.equal(got.double().cpu(), want), f"{name}: {(got.double().cpu() - want).abs().max().item()} off"
