"""The bits of the attention family (csrc/tdx_attention.hip, tdx_attention_mfma.hip, tdx_attention_bwd_mfma.hip): the cases
shared by tests/test_attention_bits.py and tests/golden/make_golden_bits.py.

`run(group)` returns one record per case (tests/pinned_bits.py).  A case is (B, H, N, dtype, library switches) and pins three
outputs: `out` and `lse` of tdx_attn_fwd and `dqkv` of tdx_attn_bwd on them, under the same switches.  Nothing in the family
merges in an order that varies from run to run -- the key-norm table is an integer atomicMax, the stream-K partials are merged
in workgroup order -- so every case is pinned.  Inputs are seeded N(0, 1); at N = 1000 they are the growing-scores inputs of
attention_cases.py, so that the lazy maximum's raise path, the norm bound's check loop and the ragged last tile all run.  Only
digests are stored, and for one case per group the raw bits of the first HEAD elements of every output, so that a mismatch
there reads in ulps.

    vector    the row-wise kernels: fp32 at N = 8 (the LocalAttention window) and N = 127 (the last size below the matrix-core
              threshold), bf16 and fp16 at N = 144 under TDX_ATTN_IMPL=vector
    mfma      the matrix-core kernels, bf16 and fp16: N = 128 (the threshold: no norm bound), 144, 257, 1000; N = 1000 again
              under TDX_ATTN_BOUND=0
    bwd_tw    every shipped instance of the two backward kernels: N = 257 under TDX_ATTN_BWD_TW = 11, 12, 21, 22
    streamk   B = 33, H = 4, N = 1000: 528 query blocks on 512 slots, segments that start on every key tile (the ragged last
              one included), partials and merge; and under TDX_ATTN_STREAMK=0
    no_arena  N = 1000 with no arena bound: no norm bound, no stream-K

B = 2, H = 4 unless stated otherwise.
"""

import torch

from attention_cases import growing_scores_qkv
from conv1_bits_cases import _env, no_arena
from pinned_bits import record as _digest, tensor_bytes

GROUPS = ["vector", "mfma", "bwd_tw", "streamk", "no_arena"]
FIXTURE = "attention_bits.json"
HEAD = 256  # elements of each output whose raw bits one case of a group stores
D = 32
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
H16 = ("bf16", "f16")
SWITCHES = ("TDX_ATTN_IMPL", "TDX_ATTN_BWD_TW", "TDX_ATTN_STREAMK", "TDX_ATTN_BOUND")

# group -> [(B, H, N, dtype name, {switch: value})]
CASES = {
    "vector": [(2, 4, 8, "f32", {}), (2, 4, 127, "f32", {})] + [(2, 4, 144, d, {"TDX_ATTN_IMPL": "vector"}) for d in H16],
    "mfma": [(2, 4, N, d, {}) for N in (128, 144, 257, 1000) for d in H16] + [(2, 4, 1000, d, {"TDX_ATTN_BOUND": "0"}) for d in H16],
    "bwd_tw": [(2, 4, 257, d, {"TDX_ATTN_BWD_TW": tw}) for tw in ("11", "12", "21", "22") for d in H16],
    "streamk": [(33, 4, 1000, d, env) for env in ({}, {"TDX_ATTN_STREAMK": "0"}) for d in H16],
    "no_arena": [(2, 4, 1000, d, {}) for d in H16],
}
# the case of each group that stores raw bits
BITS = {"vector": "2x4x8/f32", "mfma": "2x4x128/bf16", "bwd_tw": "2x4x257/f16/TDX_ATTN_BWD_TW=11", "streamk": "33x4x1000/bf16",
        "no_arena": "2x4x1000/f16"}


def case_id(case):
    B, H, N, dname, env = case
    return "/".join([f"{B}x{H}x{N}", dname] + [f"{k}={v}" for k, v in sorted(env.items())])


def names(group):
    return [case_id(c) for c in CASES[group]]


def record(outs, smallest=False):
    rec = _digest(outs)
    if smallest:
        rec["bits"] = [tensor_bytes(o.flatten()[:HEAD]).hex() for o in outs]
        rec["itemsize"] = [o.element_size() for o in outs]
    return rec


def inputs(B, H, N, dt):
    """q|k|v (B, N, 3 H D) and dO (B, N, H D) in `dt` on the device"""
    g = torch.Generator().manual_seed(1000 * B + 10 * H + N)
    if N >= 1000:
        q, k, v = growing_scores_qkv(B, N, H, D, seed=5)
    else:
        q, k, v = (torch.randn(B, N, H, D, generator=g) for _ in range(3))
    go = torch.randn(B, N, H * D, generator=g)
    qkv = torch.cat([t.reshape(B, N, H * D) for t in (q, k, v)], dim=-1)
    dev = torch.device("cuda:0")
    return qkv.to(dt).to(dev), go.to(dt).to(dev)


def forward_backward(qkv, go, H):
    """out, lse, dqkv of tdx_attn_fwd and tdx_attn_bwd under the library switches as they are now"""
    from turbdiff_amd import _lib as L

    B, N, _ = qkv.shape
    code = L.dtype_code(qkv.dtype)
    out = torch.empty(B, N, H * D, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(max(L.query("tdx_attn_bwd_workspace_bytes", B, N, H, D), 16), dtype=torch.uint8, device=qkv.device)
    L.call("tdx_attn_fwd", L.ptr(qkv), L.ptr(out), L.ptr(lse), B, N, H, D, code, L.stream())
    L.call("tdx_attn_bwd", L.ptr(qkv), L.ptr(out), L.ptr(lse), L.ptr(go), L.ptr(dqkv), B, N, H, D, code, L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return out, lse, dqkv


def _run(group):
    res = {}
    for case in CASES[group]:
        B, H, N, dname, env = case
        qkv, go = inputs(B, H, N, DTYPES[dname])
        with _env(**{**dict.fromkeys(SWITCHES), **env}):
            res[case_id(case)] = record(forward_backward(qkv, go, H), case_id(case) == BITS[group])
    return res


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd._lib` is bound to."""
    if group == "no_arena":
        with no_arena():
            return _run(group)
    return _run(group)
