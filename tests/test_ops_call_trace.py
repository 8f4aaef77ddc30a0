"""What ops.py sends across the C ABI is pinned, on the CPU: every `L.call` / `L.query` of the operators' forward and
backward (entry, arguments, pointer arguments as (tensor label, byte offset), `work`, the evaluated `meta`) must equal
tests/golden/ops_call_trace.json, which tests/golden/make_golden_ops_trace.py recorded from the commit BEFORE the
host-side change under test.  The Python-side counterpart of test_conv3_routing_is_pinned: a swapped C1 / Cout, a lost
`| WS_CLEAN`, another workspace or a reordered launch shows here without a GPU."""

import json

import pytest
import torch

import ops_trace_cases as cases
from conftest import GOLDEN

EXPECTED = json.loads((GOLDEN / "ops_call_trace.json").read_text())


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(cases.CASES)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_call_trace_is_pinned(name):
    from turbdiff_amd import ops

    got, want = cases.record(ops, name), EXPECTED[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: record {i} differs"
    assert len(got) == len(want), f"{name}: {len(got)} records, expected {len(want)}"


def test_prefetched_operands_are_found_in_the_cache():
    from turbdiff_amd import ops

    names = [r.get("call") for r in cases.record(ops, "prefetch_then_convs")]
    assert "tdx_conv3_pack_weights" in names and "tdx_transpose_many" in names
    assert "tdx_conv3_pack_weight" not in names and names.count("tdx_conv3_fwd") == 2 and names.count("tdx_conv1_fwd") == 1


def test_recorder_leaves_the_binding_as_it_was():
    from turbdiff_amd import _lib, ops

    before = (_lib.call, _lib.query, _lib.ptr, _lib.stream, ops.WGRAD_STREAM, ops.WS_CLEAN, ops.FUSE_SKIP_TAIL)
    cases.record(ops, "resize")
    assert before == (_lib.call, _lib.query, _lib.ptr, _lib.stream, ops.WGRAD_STREAM, ops.WS_CLEAN, ops.FUSE_SKIP_TAIL)
    assert "data_ptr" not in torch.Tensor.__dict__
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.resize(torch.zeros(1, 4, 4, 4, 8), (3, 3, 3))
