"""The attention backward (tdx_attn_bwd: matrix-core kernels for bf16 / fp16 at N >= 128, row-wise kernels below and under
TDX_ATTN_IMPL=vector), gradient by gradient against fp64.

Reference: fp64 autograd through the oracle's SDPA restatement on the SAME format-rounded q|k|v and dO (at the config-5
sizes, where the N x N matrix does not fit, the same mathematics in query chunks on a subset of rows: `attn_bwd_rows`).
dQ, dK and dV are judged separately, each by rel-L2 over the whole gradient and by its worst row,
max_i |got_i - ref_i| / rms_i |ref_i| with rows = (b, token, head).

Tolerances come from the reference side only.  `attn_bwd_rows(..., model=True)` restates the kernels' STATED arithmetic in
fp64: q * log2(e) / sqrt(D) rounded to the operand format (in all three kernels -- the saved log-sum-exp belongs to those
scores), P, dS, O and the three gradients rounded to the format, everything else exact.  A case's bound is 2 x the model's
rel-L2 and 4 x the model's worst row for that gradient: the model leaves out fp32 accumulation order and the hardware
exp2 (far below operand rounding), but model and kernel round different realisations of the same sums, so aggregates agree
to tens of percent and a maximum over ~10^4 rows scatters more.  Where the inputs are N(0,1) the project's absolute
tolerances (gradients: bf16 2e-2, fp16 5e-3) hold in addition.  Every case prints kernel / model before it asserts."""

import functools
import math

import pytest
import torch

from attention_cases import growing_scores_qkv
from conftest import rel_l2
from oracle import turbdiff_oracle as O

pytestmark = pytest.mark.gpu

D = 32
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
ABS_TOL = {torch.bfloat16: 2e-2, torch.float16: 5e-3}  # rel-L2 of a gradient, N(0,1) inputs (test_hip_ops.py)
DTYPES = [torch.bfloat16, torch.float16]
NAMES = ("dQ", "dK", "dV")


def dev():
    return torch.device("cuda:0")


def _tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def attn_bwd_rows(q, k, v, go, dtype, I=None, J=None, chunk=1024, model=True):
    """dQ[I], dK[J], dV[J] of softmax(q k^T / sqrt(D)) v under the output gradient go; all tensors (B, H, N, D) fp64, already
    rounded to `dtype`; I / J index tensors of query / key rows (None = all rows).  Walks the queries in chunks, so only
    chunk x N scores exist at a time.  model=False: exact fp64.  model=True: the format model of the kernels' stated arithmetic,
    r(.) = round to dtype through fp32, c = log2(e) / sqrt(D):
        qs = r(q c)   S2 = qs k^T   lse2 = log2 sum_j 2^S2   P = 2^(S2 - lse2)   O = r(r(P) v)   delta = sum_d dO O
        dP = dO v^T   dS = P (dP - delta)   dQ = r(r(dS) k / sqrt(D))   dV = r(r(P)^T dO)   dK = r(r(dS)^T q / sqrt(D))"""
    B, H, N, _ = q.shape
    isd = 1.0 / math.sqrt(D)
    r = (lambda t: t.float().to(dtype).double()) if model else (lambda t: t)
    qs = r(q * (LOG2E * isd))
    kT, vT = k.transpose(-1, -2), v.transpose(-1, -2)
    vJT = vT if J is None else v[:, :, J].transpose(-1, -2)

    def block(idx):  # probabilities, dO and delta of the query rows idx against ALL keys
        S2 = qs[:, :, idx] @ kT
        lse2 = torch.logsumexp(S2 * LN2, dim=-1, keepdim=True) / LN2
        P = torch.exp2(S2 - lse2)
        del S2
        gi = go[:, :, idx]
        delta = (gi * r(r(P) @ v)).sum(-1, keepdim=True)
        return P, gi, delta

    nJ = N if J is None else len(J)
    dK = torch.zeros(B, H, nJ, D, dtype=torch.float64, device=q.device)
    dV = torch.zeros_like(dK)
    dQ = [] if I is None else None
    for a in range(0, N, chunk):
        idx = torch.arange(a, min(a + chunk, N), device=q.device)
        P, gi, delta = block(idx)
        if I is None:
            dQ.append(r(r(P * (gi @ vT - delta)) @ k * isd))
        PJ = P if J is None else P[..., J]
        del P
        dSJ = PJ * (gi @ vJT - delta)
        dV += r(PJ).transpose(-1, -2) @ gi
        dK += r(dSJ).transpose(-1, -2) @ q[:, :, idx] * isd
        del PJ, dSJ
    if I is None:
        dQ = torch.cat(dQ, dim=2)
    else:
        P, gi, delta = block(I)
        dQ = r(r(P * (gi @ vT - delta)) @ k * isd)
    return dQ, r(dK), r(dV)


def heads_first(t, H):
    """(B, N, H * D) -> (B, H, N, D)"""
    return t.reshape(t.shape[0], t.shape[1], H, D).transpose(1, 2)


def split_grad(dqkv, H):
    return tuple(heads_first(p, H).double() for p in dqkv.chunk(3, dim=-1))


def make_inputs(regime, dtype, B, H, N):
    """q|k|v (B, N, 3 H D) and dO (B, N, H D) in `dtype` on the device; distinct random data in every (b, h)"""
    seed = 1000 * B + 10 * H + N
    if regime == "grow":
        q, k, v = growing_scores_qkv(B, N, H, D, seed=5)
    else:
        g = torch.Generator().manual_seed(seed)
        s = float(regime)
        q, k = torch.randn(B, N, H, D, generator=g) * s, torch.randn(B, N, H, D, generator=g) * s
        v = torch.randn(B, N, H, D, generator=g)
    go = torch.randn(B, N, H * D, generator=torch.Generator().manual_seed(seed + 1))  # dO ~ N(0,1), not ones
    qkv = torch.cat([t.reshape(B, N, H * D) for t in (q, k, v)], dim=-1)
    return qkv.to(dtype).to(dev()), go.to(dtype).to(dev())


@functools.lru_cache(maxsize=3)
def dense_case(regime, dtype, B, H, N):
    """inputs, fp64 autograd reference through the oracle's SDPA and the format model, all rows (on the device)"""
    qkv, go = make_inputs(regime, dtype, B, H, N)
    x = qkv.double().requires_grad_()
    q, k, v = (heads_first(p, H) for p in x.chunk(3, dim=-1))
    O.sdpa(q, k, v).transpose(1, 2).reshape(B, N, H * D).backward(go.double())
    ref = split_grad(x.grad, H)
    with torch.no_grad():
        model = attn_bwd_rows(q.detach(), k.detach(), v.detach(), heads_first(go.double(), H), dtype, chunk=2048)
    return qkv, go, ref, model


def rowmax(a, b):
    """worst row error over the rms row norm of its (b, h); a, b (B, H, n, D)"""
    e = (a - b).norm(dim=-1)
    s = b.norm(dim=-1).pow(2).mean(-1, keepdim=True).sqrt()
    return (e / s).max().item()


def check(tag, got, ref, model, abs_tol=None):
    """the model bounds (2 x rel-L2, 4 x worst row) per gradient; prints every figure, then asserts"""
    bad = []
    for name, g, rf, m in zip(NAMES, got, ref, model):
        e, em, w, wm = rel_l2(g, rf), rel_l2(m, rf), rowmax(g, rf), rowmax(m, rf)
        print(f"ATTN_BWD {tag} {name}: rel-L2 {e:.2e} model {em:.2e} ratio {e / em:.2f} | worst row {w:.2e} model {wm:.2e} "
              f"ratio {w / wm:.2f}")
        if not e <= 2 * em:
            bad.append(f"{name} rel-L2 {e:.3e} > 2 x {em:.3e}")
        if not w <= 4 * wm:
            bad.append(f"{name} worst row {w:.3e} > 4 x {wm:.3e}")
        if abs_tol is not None and not e < abs_tol:
            bad.append(f"{name} rel-L2 {e:.3e} >= {abs_tol}")
    assert not bad, (tag, bad)


def run_autograd(qkv, go, H):
    from turbdiff_amd import ops

    x = qkv.clone().requires_grad_()
    ops.attention(x, H).backward(go)
    return split_grad(x.grad, H)


def abi_forward(qkv, H):
    from turbdiff_amd import _lib as L

    B, N, _ = qkv.shape
    out = torch.empty(B, N, H * D, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    L.call("tdx_attn_fwd", L.ptr(qkv), L.ptr(out), L.ptr(lse), B, N, H, D, L.dtype_code(qkv.dtype), L.stream())
    return out, lse


def abi_backward(qkv, out, lse, go, dqkv, H):
    from turbdiff_amd import _lib as L

    B, N, _ = qkv.shape
    ws = torch.empty(max(L.query("tdx_attn_bwd_workspace_bytes", B, N, H, D), 16), dtype=torch.uint8, device=qkv.device)
    L.call("tdx_attn_bwd", L.ptr(qkv), L.ptr(out), L.ptr(lse), L.ptr(go), L.ptr(dqkv), B, N, H, D, L.dtype_code(qkv.dtype),
           L.ptr(ws), L.stream())
    torch.cuda.synchronize()


def planned(B, N, H, dtype):
    """what the library plans for a call on this stream, under the switches as they are now (its arena bound first)"""
    from turbdiff_amd import _lib as L

    L.ensure_scratch()
    return L.attn_plan(B, N, H, D, L.dtype_code(dtype))


@pytest.fixture(autouse=True)
def _attention_env(monkeypatch):
    for name in ("TDX_ATTN_IMPL", "TDX_ATTN_BWD_TW", "TDX_ATTN_STREAMK", "TDX_ATTN_BOUND"):
        monkeypatch.delenv(name, raising=False)


def test_chunked_reference_equals_autograd():
    """the chunked fp64 passes of `attn_bwd_rows` (the reference at the config-5 sizes) against autograd, on a row subset"""
    B, H, N = 2, 3, 300
    qkv, go, ref, _ = dense_case("1", torch.bfloat16, B, H, N)
    q, k, v = (heads_first(p, H).double() for p in qkv.chunk(3, dim=-1))
    I = torch.tensor([0, 5, 63, 64, 255, 256, 299], device=dev())
    J = torch.tensor([1, 31, 32, 128, 298], device=dev())
    dq, dk, dv = attn_bwd_rows(q, k, v, heads_first(go.double(), H), torch.bfloat16, I, J, chunk=77, model=False)
    assert rel_l2(dq, ref[0][:, :, I]) < 1e-12 and rel_l2(dk, ref[1][:, :, J]) < 1e-12 and rel_l2(dv, ref[2][:, :, J]) < 1e-12


# ---- (a) layout and grid: the N = 128 threshold, ragged and aligned ends, batch and head counts other than (2, 4)
LAYOUT_CASES = [(2, 4, N) for N in (127, 128, 129, 144, 255, 256, 257, 300, 511, 513, 1000, 2049)] + [
    (B, H, N) for (B, H) in ((1, 1), (3, 2), (1, 8), (6, 4), (5, 3)) for N in (144, 257, 1000)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("B,H,N", LAYOUT_CASES)
def test_layout_and_grid(B, H, N, dtype):
    qkv, go, ref, model = dense_case("1", dtype, B, H, N)
    check(f"layout {_tag(dtype)} B={B} H={H} N={N}", run_autograd(qkv, go, H), ref, model, ABS_TOL[dtype])


# ---- (b) every shipped instance of the two matrix-core kernels
@pytest.mark.parametrize("tw", [None, "11", "12", "21"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("N", [144, 257, 1000, 2049])
def test_every_shipped_instance(N, dtype, tw, monkeypatch):
    if tw is not None:
        monkeypatch.setenv("TDX_ATTN_BWD_TW", tw)
    qkv, go, ref, model = dense_case("1", dtype, 2, 4, N)
    p = planned(2, N, 4, dtype)  # the instance the switch names is the one that runs
    assert (p["bwd"], 10 * p["tw_dq"] + p["tw_dkv"]) == ("mfma", int(tw or "22"))
    check(f"instance TW={tw} {_tag(dtype)} N={N}", run_autograd(qkv, go, 4), ref, model, ABS_TOL[dtype])


# ---- (c) large logits
def _large_logits(B, H, N, regime, dtype, streamk, monkeypatch, streamk_runs):
    if streamk is not None:
        monkeypatch.setenv("TDX_ATTN_STREAMK", streamk)
    assert planned(B, N, H, dtype)["streamk"] == int(streamk_runs)
    qkv, go, ref, model = dense_case(regime, dtype, B, H, N)
    got = run_autograd(qkv, go, H)
    sum_go = heads_first(go.double(), H).sum(2)
    res, res_m = rel_l2(got[2].sum(2), sum_go), rel_l2(model[2].sum(2), sum_go)
    tag = f"logits {regime} {_tag(dtype)} N={N} streamk={streamk}"
    print(f"ATTN_BWD {tag} sum_keys dV: residual {res:.2e} model {res_m:.2e} ratio {res / res_m:.2f}")
    check(tag, got, ref, model)
    assert res <= 2 * res_m, (tag, res, res_m)


@pytest.mark.parametrize("streamk", [None, "0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("regime", ["grow", "3"])
@pytest.mark.parametrize("N", [1000, 4096 + 64 * 37 + 5])
def test_large_logits(N, regime, dtype, streamk, monkeypatch):
    """|q| |k| / sqrt(D) up to ~200 (the growing-scores inputs) and 3 N(0,1) q, k (largest score ~50): the recomputed
    probabilities are only as good as the agreement of the backward's scores with the forward's, whose log-sum-exp they are
    normalised by.  All three gradients at the model bounds, and sum_keys dV = sum_queries dO per (b, h, d) -- the rows of P
    sum to one -- at twice the model's own residual.  (B = 2, H = 4 is at most 208 query blocks: the forward runs one
    workgroup per block in both `streamk` arms, as its plan says; test_large_logits_stream_k has the shape that splits.)"""
    _large_logits(2, 4, N, regime, dtype, streamk, monkeypatch, streamk_runs=False)


@pytest.mark.parametrize("streamk", [None, "0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("regime", ["grow", "3"])
def test_large_logits_stream_k(regime, dtype, streamk, monkeypatch):
    """The same at B = 33, H = 4, N = 1000, the smallest shape whose forward the stream-K schedule takes: 528 query blocks on
    512 workgroups of 17 (block, key tile) iterations, so segments start on every one of the 16 key tiles, the ragged last one
    included, and every block is merged from partials.  The plan says stream-K runs in one arm and not in the other; the
    backward consumes either forward's log-sum-exp at the same bounds."""
    _large_logits(33, 4, 1000, regime, dtype, streamk, monkeypatch, streamk_runs=streamk is None)


# ---- (d) overwrite, not accumulate; nothing outside
@pytest.mark.parametrize("impl", ["mfma", "vector"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("N", [256, 257, 1000])
def test_overwrites_its_output_and_nothing_else(N, dtype, impl, monkeypatch):
    """dqkv pre-filled with NaN, a view into a larger buffer with 256 guard rows (what one workgroup owns) of a sentinel in
    front and behind: no NaN left inside, the guards untouched, and the same bits as into a zero-filled buffer."""
    if impl == "vector":
        monkeypatch.setenv("TDX_ATTN_IMPL", "vector")
    B, H, G = 2, 4, 256
    ld = 3 * H * D
    p = planned(B, N, H, dtype)
    assert (p["fwd"], p["bwd"]) == (impl, impl)
    qkv, go = make_inputs("1", dtype, B, H, N)
    out, lse = abi_forward(qkv, H)
    buf = torch.full((G + B * N + G, ld), -1234.0, dtype=dtype, device=dev())
    before = buf.clone()
    dqkv = buf[G:G + B * N].view(B, N, ld)
    dqkv.fill_(float("nan"))
    abi_backward(qkv, out, lse, go, dqkv, H)
    assert not torch.isnan(dqkv).any()
    assert torch.equal(buf[:G].view(torch.int16), before[:G].view(torch.int16))
    assert torch.equal(buf[G + B * N:].view(torch.int16), before[G + B * N:].view(torch.int16))
    again = torch.zeros(B, N, ld, dtype=dtype, device=dev())
    abi_backward(qkv, out, lse, go, again, H)
    assert torch.equal(again.view(torch.int16), dqkv.view(torch.int16))


# ---- (e) the config-5 size and one ragged large size, element-wise on 256 query rows and 256 key rows
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
@pytest.mark.parametrize("N", [96 * 32 * 24, 20011])
def test_config5_size_rows(N, dtype):
    """B = 1, H = 4, N = 73 728 (BASELINE configs[4]) and N = 20 011 (no multiple of 256 or 64): dQ on a query subset, dK and dV
    on a key subset, 256 rows each -- the first 32 and the last 32 tokens (the first and the last workgroup of the grid) plus
    192 from a fixed-seed permutation -- against the same chunked fp64 passes, exact and as the format model."""
    B, H = 1, 4
    qkv, go = make_inputs("1", dtype, B, H, N)
    perm = torch.randperm(N - 64, generator=torch.Generator().manual_seed(12))[:192] + 32
    rows = torch.cat([torch.arange(32), perm.sort().values, torch.arange(N - 32, N)]).to(dev())
    assert len(rows) == 256 and len(torch.unique(rows)) == 256
    got = run_autograd(qkv, go, H)
    got = (got[0][:, :, rows], got[1][:, :, rows], got[2][:, :, rows])
    q, k, v = (heads_first(p, H).double() for p in qkv.chunk(3, dim=-1))
    g = heads_first(go.double(), H)
    ref = attn_bwd_rows(q, k, v, g, dtype, rows, rows, model=False)
    model = attn_bwd_rows(q, k, v, g, dtype, rows, rows, model=True)
    check(f"rows {_tag(dtype)} N={N}", got, ref, model, ABS_TOL[dtype])


# ---- (f) the hand-over: (B, H, N) natural-log lse and out, whichever forward wrote them
@pytest.mark.parametrize("bwd_impl", ["mfma", "vector"])
@pytest.mark.parametrize("fwd_impl", ["mfma", "vector"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_tag)
def test_lse_handover_between_kernel_families(dtype, fwd_impl, bwd_impl, monkeypatch):
    B, H, N = 2, 4, 1000
    qkv, go, ref, model = dense_case("1", dtype, B, H, N)
    if fwd_impl == "vector":
        monkeypatch.setenv("TDX_ATTN_IMPL", "vector")
    assert planned(B, N, H, dtype)["fwd"] == fwd_impl
    out, lse = abi_forward(qkv, H)
    torch.cuda.synchronize()
    monkeypatch.delenv("TDX_ATTN_IMPL", raising=False)
    if bwd_impl == "vector":
        monkeypatch.setenv("TDX_ATTN_IMPL", "vector")
    assert planned(B, N, H, dtype)["bwd"] == bwd_impl
    dqkv = torch.empty_like(qkv)
    abi_backward(qkv, out, lse, go, dqkv, H)
    check(f"handover {_tag(dtype)} fwd={fwd_impl} bwd={bwd_impl}", split_grad(dqkv, H), ref, model, ABS_TOL[dtype])
