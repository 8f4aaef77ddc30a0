"""The attention family (csrc/tdx_attention*.hip) computes the bits it computed before its host side was rewritten around one
plan per call and its kernels around one head view: every case of tests/attention_bits_cases.py must reproduce the digest in
tests/golden/attention_bits.json, which tests/golden/make_golden_bits.py recorded on the MI355X from the library of the commit
BEFORE that change (twice, in separate processes: the two recordings were byte-identical).  One case per group stores the
first elements of its outputs themselves, so a mismatch there is reported in units of the last place."""

import json

import pytest

import attention_bits_cases as bits
from attention_cases import expected_plan
from conftest import GOLDEN
from pinned_bits import assert_pinned

EXPECTED = json.loads((GOLDEN / bits.FIXTURE).read_text())
CODES = {"f32": 0, "bf16": 1, "f16": 3}  # TDX_F32, TDX_BF16, TDX_F16


def test_fixture_and_cases_agree():
    assert sorted(EXPECTED) == sorted(bits.GROUPS)
    for g in bits.GROUPS:
        assert sorted(EXPECTED[g]) == sorted(bits.names(g))
        assert [n for n, rec in EXPECTED[g].items() if "bits" in rec] == [bits.BITS[g]]
    # the first group's raw bits hold every element of out and lse of the smallest case (2 x 8 x 4 x 32 and 2 x 4 x 8 float32)
    assert [len(b) // 8 for b in EXPECTED["vector"][bits.BITS["vector"]]["bits"]] == [bits.HEAD, 64, bits.HEAD]


def test_cases_reach_every_plan():
    """By the rule the library's plan is held to (attention_cases.expected_plan; tests/test_switches_host.py), under the
    default 96 MB arena and with none: both families, stream-K on and off, the norm bound on and off, the four backward
    instances, and a stream-K case whose segments start on every key tile."""
    plans = {g: [expected_plan(B, N, H, 32, CODES[d], env, 0 if g == "no_arena" else 96 << 20) for B, H, N, d, env in bits.CASES[g]]
             for g in bits.GROUPS}
    assert {p["fwd"] for p in plans["vector"]} == {"vector"}
    assert {p["fwd"] for g in bits.GROUPS[1:] for p in plans[g]} == {"mfma"}
    assert {(p["streamk"], p["bound"]) for p in plans["mfma"]} == {(0, 0), (0, 1)}
    assert {(p["tw_dq"], p["tw_dkv"]) for p in plans["bwd_tw"]} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert [(p["streamk"], p["nwg"], p["chunk"]) for p in plans["streamk"]] == [(1, 512, 17)] * 2 + [(0, 528, 16)] * 2
    assert {(w * 17) % 16 for w in range(512)} == set(range(16))  # first key tile of workgroup w's first segment
    assert {(p["streamk"], p["bound"]) for p in plans["no_arena"]} == {(0, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("group", bits.GROUPS)
def test_bits_are_pinned(group):
    assert_pinned(bits.run(group), EXPECTED[group], group)
