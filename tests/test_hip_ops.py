"""Per-operator parity of the HIP kernels (through the C ABI) against the CPU oracle.

fp32 kernels must match to ~1e-5 rel-L2 (different summation order only); bf16 kernels are
compared with the oracle evaluated on the same bf16-rounded inputs, so the remaining error
is the bf16 rounding of the output (2^-9 relative per element, ~2e-3 rel-L2) plus fp32
accumulation order.
"""

import math

import pytest
import torch
import torch.nn.functional as F

from attention_cases import growing_scores_qkv
from conftest import rel_l2
from oracle import turbdiff_oracle as O

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5
BF16_TOL = 6e-3
FP16_TOL = 8e-4  # IEEE half storage: 2^-12 relative per element (~2.5e-4 rel-L2 measured), an eighth of bf16's


def dev():
    return torch.device("cuda:0")


def nvc(x):  # (B,C,X,Y,Z) -> (B,X,Y,Z,C)
    return x.permute(0, 2, 3, 4, 1).contiguous()


def ncv(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def q(x, dtype):
    """round to the compute dtype and back (what the kernel sees)"""
    return x.to(dtype).float()


def tol_for(dtype):
    return {torch.float32: F32_TOL, torch.bfloat16: BF16_TOL, torch.float16: FP16_TOL}[dtype]


MODE_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(autouse=True)
def _conv_impl_env(monkeypatch):
    monkeypatch.delenv("TDX_CONV_IMPL", raising=False)


def test_library_loads_on_gpu_box():
    from turbdiff_amd import _lib

    lib = _lib.load()
    assert lib.tdx_version() >= 1 and lib.tdx_arch() == b"gfx950"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_layout_roundtrip(dtype):
    from turbdiff_amd import ops

    x = rnd(2, 5, 7, 3, 9).to(dev())
    y = ops.to_nvc(x, dtype)
    assert y.shape == (2, 7, 3, 9, 5)
    assert torch.equal(y.float().cpu(), nvc(q(x.cpu(), dtype)))
    back = ops.to_ncv(y, torch.float32)
    assert torch.equal(back.cpu(), q(x.cpu(), dtype))


CONV_CASES = [
    # B, Cin1, Cin2, Cout, X, Y, Z
    (2, 8, 0, 16, 7, 5, 6),
    (1, 32, 0, 32, 9, 8, 8),
    (2, 64, 0, 64, 5, 9, 11),
    (1, 32, 32, 64, 6, 10, 7),
    (1, 128, 0, 32, 4, 8, 8),
    (1, 16, 0, 96, 3, 3, 3),
    (1, 64, 0, 64, 12, 4, 3),
    # the deep U-Net levels at their real channel counts
    (2, 256, 0, 256, 12, 4, 3),
    (1, 256, 256, 128, 24, 8, 6),
]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("mode", ["f32-direct", "f32-auto", "f32-split", "bf16-direct", "bf16-auto", "fp16-direct", "fp16-auto"])
def test_conv3_fwd_bwd(case, mode, monkeypatch):
    from turbdiff_amd import ops

    B, C1, C2, Cout, X, Y, Z = case
    dtype = MODE_DTYPE[mode.split("-")[0]]
    monkeypatch.setenv("TDX_CONV_IMPL", mode.split("-")[1])
    Cin = C1 + C2
    x = q(rnd(B, Cin, X, Y, Z, seed=1), dtype)
    w = q(rnd(Cout, Cin, 3, 3, 3, seed=2, scale=1 / math.sqrt(27 * Cin)), dtype)
    b = rnd(Cout, seed=3)
    gy = q(rnd(B, Cout, X, Y, Z, seed=4), dtype)
    # oracle (CPU, fp64 accumulate for a clean reference)
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    yr = O.conv3_replicate(xr, wr, br)
    yr.backward(gy.double())

    xd = nvc(x).to(dev()).to(dtype)
    x1 = xd[..., :C1].contiguous().requires_grad_()
    x2 = xd[..., C1:].contiguous().requires_grad_() if C2 else None
    wd = w.to(dev()).requires_grad_()
    bd = b.to(dev()).requires_grad_()
    y = ops.conv3(x1, wd, bd, x2=x2)
    y.backward(nvc(gy).to(dev()).to(dtype))
    # split-precision MFMA (bf16 hi + lo operands): ~4e-6 per layer, gated at 2e-5
    tol = 2e-5 if mode == "f32-split" else tol_for(dtype)
    assert rel_l2(ncv(y.float().cpu()), yr) < tol
    gx = torch.cat([x1.grad] + ([x2.grad] if C2 else []), dim=-1)
    assert rel_l2(ncv(gx.float().cpu()), xr.grad) < tol
    assert rel_l2(wd.grad.cpu(), wr.grad) < (1e-4 if dtype == torch.float32 else tol)
    assert rel_l2(bd.grad.cpu(), br.grad) < (1e-4 if dtype == torch.float32 else tol)


def test_conv3_mfma_matches_direct_bf16(monkeypatch):
    """same bf16 inputs through both implementations: only accumulation order differs"""
    from turbdiff_amd import ops

    x = rnd(2, 9, 17, 10, 64, seed=5).to(dev()).bfloat16()
    w = rnd(64, 64, 3, 3, 3, seed=6, scale=0.03).to(dev())
    outs = {}
    for impl in ("direct", "mfma"):
        monkeypatch.setenv("TDX_CONV_IMPL", impl)
        xi = x.clone().requires_grad_()
        y = ops.conv3(xi, w, None)
        y.backward(torch.ones_like(y))
        outs[impl] = (y.float(), xi.grad.float())
    assert rel_l2(outs["mfma"][0], outs["direct"][0]) < 3e-3
    assert rel_l2(outs["mfma"][1], outs["direct"][1]) < 3e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", [(2, 4, 0, 32, 100), (1, 64, 64, 32, 333), (3, 128, 0, 384, 70), (2, 32, 0, 4, 257)])
def test_conv1_fwd_bwd(dtype, case):
    from turbdiff_amd import ops

    B, C1, C2, Cout, V = case
    Cin = C1 + C2
    x = q(rnd(B, V, Cin, seed=1), dtype)
    w = rnd(Cout, Cin, 1, 1, 1, seed=2, scale=1 / math.sqrt(Cin))
    b = rnd(Cout, seed=3)
    add = q(rnd(B, V, Cout, seed=4), dtype)
    gy = q(rnd(B, V, Cout, seed=5), dtype)
    xr, wr, br, ar = (t.double().requires_grad_() for t in (x, w, b, add))
    yr = xr @ wr.reshape(Cout, Cin).t() + br + ar
    yr.backward(gy.double())

    xd = x.to(dev()).to(dtype).reshape(B, V, 1, 1, Cin)
    x1 = xd[..., :C1].contiguous().requires_grad_()
    x2 = xd[..., C1:].contiguous().requires_grad_() if C2 else None
    wd, bd = w.to(dev()).requires_grad_(), b.to(dev()).requires_grad_()
    ad = add.to(dev()).to(dtype).reshape(B, V, 1, 1, Cout).requires_grad_()
    y = ops.conv1(x1, wd, bd, x2=x2, add=ad)
    y.backward(gy.to(dev()).to(dtype).reshape(B, V, 1, 1, Cout))
    tol = tol_for(dtype)
    assert rel_l2(y.float().cpu().reshape(B, V, Cout), yr) < tol
    gx = torch.cat([x1.grad] + ([x2.grad] if C2 else []), dim=-1).reshape(B, V, Cin)
    assert rel_l2(gx.float().cpu(), xr.grad) < tol
    assert rel_l2(wd.grad.cpu(), wr.grad) < (1e-4 if dtype == torch.float32 else tol)
    assert rel_l2(bd.grad.cpu(), br.grad) < (1e-4 if dtype == torch.float32 else tol)
    assert rel_l2(ad.grad.float().cpu().reshape(B, V, Cout), ar.grad) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", [(2, 16, 8, 7, 5, 6, True, True), (1, 64, 8, 9, 4, 3, False, True), (2, 32, 32, 5, 5, 5, True, False),
                                  (1, 512, 8, 12, 4, 3, True, True), (2, 24, 1, 6, 5, 4, False, False),
                                  # V = 12000 / 9000: 94 and 512 streaming blocks per sample (gn_bwd_group_kernel's slots past the first)
                                  (1, 64, 8, 30, 20, 20, True, True), (1, 512, 8, 25, 20, 18, True, False)])
def test_gn_film_silu(dtype, case):
    from turbdiff_amd import ops

    B, Cc, G, X, Y, Z, film, res = case
    x = q(rnd(B, Cc, X, Y, Z, seed=1) * 1.5 + 0.3, dtype)
    gamma, beta = 1 + 0.3 * rnd(Cc, seed=2), 0.2 * rnd(Cc, seed=3)
    scale, shift = 0.5 * rnd(B, Cc, seed=4), 0.5 * rnd(B, Cc, seed=5)
    r = q(rnd(B, Cc, X, Y, Z, seed=6), dtype)
    gy = q(rnd(B, Cc, X, Y, Z, seed=7), dtype)
    leaves = [t.double().requires_grad_() for t in (x, gamma, beta, scale, shift, r)]
    xr, gr, br, sr, hr, rr = leaves
    n = O.group_norm(xr, G, gr, br)
    if film:
        n = hr[..., None, None, None] + (sr[..., None, None, None] + 1) * n
    yr = F.silu(n) + (rr if res else 0)
    yr.backward(gy.double())

    d = dev()
    xd = nvc(x).to(d).to(dtype).requires_grad_()
    gd, bd = gamma.to(d).requires_grad_(), beta.to(d).requires_grad_()
    sd_, hd = scale.to(d).requires_grad_(), shift.to(d).requires_grad_()
    rd = nvc(r).to(d).to(dtype).requires_grad_()
    y = ops.gn_film_silu(xd, gd, bd, G, sd_ if film else None, hd if film else None, res=rd if res else None)
    y.backward(nvc(gy).to(d).to(dtype))
    tol = tol_for(dtype)
    assert rel_l2(ncv(y.float().cpu()), yr) < tol
    assert rel_l2(ncv(xd.grad.float().cpu()), xr.grad) < (1e-4 if dtype == torch.float32 else 2e-2)
    ptol = 1e-4 if dtype == torch.float32 else 2e-2
    assert rel_l2(gd.grad.cpu(), gr.grad) < ptol
    assert rel_l2(bd.grad.cpu(), br.grad) < ptol
    if film:
        assert rel_l2(sd_.grad.cpu(), sr.grad) < ptol
        assert rel_l2(hd.grad.cpu(), hr.grad) < ptol
    if res:
        assert rel_l2(ncv(rd.grad.float().cpu()), rr.grad) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sizes", [((13, 7, 6), (6, 3, 3)), ((6, 3, 3), (13, 7, 6)), ((12, 8, 9), (6, 4, 4)),
                                   ((6, 4, 4), (12, 8, 9)), ((3, 3, 3), (3, 3, 3)), ((5, 4, 3), (3, 3, 3)), ((3, 3, 3), (5, 4, 3))])
def test_resize(dtype, sizes):
    from turbdiff_amd import ops

    si, so = sizes
    x = q(rnd(2, 16, *si, seed=1), dtype)
    gy = q(rnd(2, 16, *so, seed=2), dtype)
    xr = x.double().requires_grad_()
    yr = O.resize(xr, so)
    yr.backward(gy.double())
    xd = nvc(x).to(dev()).to(dtype).requires_grad_()
    y = ops.resize(xd, so)
    y.backward(nvc(gy).to(dev()).to(dtype))
    tol = tol_for(dtype)
    assert rel_l2(ncv(y.float().cpu()), yr) < tol
    assert rel_l2(ncv(xd.grad.float().cpu()), xr.grad) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N", [37, 144, 200])
def test_attention(dtype, N):
    from turbdiff_amd import ops

    B, H, D = 2, 4, 32
    qkv = q(rnd(B, N, 3 * H * D, seed=1), dtype)
    go = q(rnd(B, N, H * D, seed=2), dtype)
    ref = qkv.double().requires_grad_()
    qq, kk, vv = (p.reshape(B, N, H, D).transpose(1, 2) for p in ref.chunk(3, dim=-1))
    o = O.sdpa(qq, kk, vv).transpose(1, 2).reshape(B, N, H * D)
    o.backward(go.double())
    qd = qkv.to(dev()).to(dtype).requires_grad_()
    out = ops.attention(qd, H)
    out.backward(go.to(dev()).to(dtype))
    tol = 1e-5 if dtype == torch.float32 else 8e-3
    assert rel_l2(out.float().cpu(), o) < tol
    assert rel_l2(qd.grad.float().cpu(), ref.grad) < (1e-4 if dtype == torch.float32 else 2e-2)


def test_fused_attention_api(golden):
    from turbdiff_amd.models.attention import fused_attention

    g = golden("ops")
    o = fused_attention(*(g[f"sdpa/{n}"].to(dev()) for n in "qkv"))
    assert rel_l2(o.cpu(), g["sdpa/o"]) < 1e-5


# ------------------------------------------------------------------ DDPM arithmetic


def _mask_idx(V, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.sort(torch.randperm(V, generator=g)[: (2 * V) // 3]).values


@pytest.mark.parametrize("shape", [(2, 4, 5, 4, 3), (3, 4, 8, 8, 4)])
@pytest.mark.parametrize("keep_bcs", [False, True])
def test_q_sample(shape, keep_bcs):
    from turbdiff_amd import ops

    buf = O.schedule_buffers("log-snr-linear", 10)
    x0, nz = rnd(*shape, seed=1), rnd(*shape, seed=2)
    V = x0[0, 0].numel()
    idx = _mask_idx(V)
    t = torch.tensor([3, 9, 0][: shape[0]])
    ref = O.q_sample(buf, x0, t, nz)
    if keep_bcs:
        ref = O.where_cells(idx, ref, x0)
    d = dev()
    mask = ops.cell_mask(idx.to(d), V)
    assert mask.sum().item() == idx.numel()
    out = ops.q_sample(x0.to(d), nz.to(d), buf["sqrt_alphas_cumprod"].to(d), buf["sqrt_one_minus_alphas_cumprod"].to(d),
                       t.to(d), mask=mask, keep_bcs=keep_bcs)
    assert torch.allclose(out.cpu(), ref, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("t", [0, 1, 7])
def test_p_sample_step(noise_bcs, t):
    from turbdiff_amd import ops, schedules

    T = 10
    buf = O.schedule_buffers("log-snr-linear", T)
    shape = (2, 4, 6, 5, 4)
    x_t, eps, z, z2, xb = (rnd(*shape, seed=s) for s in range(5))
    V = 120
    idx = _mask_idx(V)
    tt = torch.full((2,), t)
    _, mean = O.model_mean(buf, x_t, tt, eps, idx, noise_bcs)
    if t == 0:
        ref = O.where_cells(idx, mean, xb)
    else:
        zz = z if noise_bcs else O.where_cells(idx, z)
        ref = mean + (buf["log_betas"][t] / 2).exp() * zz
        if noise_bcs:
            ref = O.where_cells(idx, ref, O.q_sample(buf, xb, tt, z2))
    d = dev()
    sched = schedules.pack_step_tables(schedules.diffusion_tables("log-snr-linear", T)).to(d)
    mask = ops.cell_mask(idx.to(d), V)
    out = ops.p_sample_step(x_t.to(d), eps.to(d), z.to(d), z2.to(d), xb.to(d), mask, sched, T,
                            torch.tensor([t], device=d), noise_bcs, False)
    assert torch.allclose(out.cpu(), ref, rtol=2e-6, atol=1e-6)


@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("t", [0, 1, 7])
@pytest.mark.parametrize("shape", [(3, 4, 6, 5, 4), (1, 4, 2, 2, 1), (2, 4, 40, 33, 28), (1, 4, 48, 48, 32)])
def test_p_sample_step_rng_matches_separate_draws_bitwise(noise_bcs, clip, t, shape):
    """tdx_p_sample_step_rng == tdx_randn_batched(z); [tdx_randn_batched(z2);] tdx_p_sample_step, bit for bit, and it leaves
    the same RNG offset and t - 1 behind (the contract include/tdx.h states)."""
    from turbdiff_amd import ops, schedules

    T, d = 10, dev()
    V = shape[2] * shape[3] * shape[4]
    x_t, eps, xb = (rnd(*shape, seed=s).to(d) for s in range(3))
    mask = ops.cell_mask(_mask_idx(V).to(d), V)
    sched = schedules.pack_step_tables(schedules.diffusion_tables("log-snr-linear", T)).to(d)
    sids = torch.tensor([(5 << 32) | 7, 11, (1 << 32) | 2][: shape[0]], dtype=torch.int64, device=d)
    seed, off0 = 1234, 4096

    off = torch.full((1,), off0, dtype=torch.int64, device=d)
    z = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off)
    z2 = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off) if noise_bcs else None
    tt = torch.tensor([t], device=d)
    ref = ops.p_sample_step(x_t, eps, z, z2, xb, mask, sched, T, tt, noise_bcs, clip)

    off_f = torch.full((1,), off0, dtype=torch.int64, device=d)
    tf = torch.tensor([t], device=d)
    assert ops.p_sample_step_rng_supported(x_t)
    out = ops.p_sample_step_rng(x_t, eps, xb, mask, sched, T, tf, noise_bcs, clip, seed, sids, off_f)
    assert torch.equal(out, ref)
    assert int(off_f) == int(off) == off0 + (2 if noise_bcs else 1) * (4 * V // 4)
    assert int(tf) == t - 1
    # in place, as the sampler calls it
    x_in = x_t.clone()
    off_f.fill_(off0); tf.fill_(t)
    ops.p_sample_step_rng(x_in, eps, xb, mask, sched, T, tf, noise_bcs, clip, seed, sids, off_f, out=x_in)
    assert torch.equal(x_in, ref)


def test_p_sample_step_rng_refuses_unaligned_planes():
    from turbdiff_amd import ops

    x = torch.zeros(1, 4, 3, 3, 3, device=dev())
    assert not ops.p_sample_step_rng_supported(x)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float16])
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("B,D,grid", [(2, 32, (13, 9, 11)), (1, 32, (1, 1, 1)), (3, 16, (5, 1, 7)), (1, 64, (33, 32, 32)),
                                      (2, 8, (17, 16, 2))])
def test_gn_apply_encoded_equals_encode_then_apply_bitwise(dtype, with_c, B, D, grid):
    """include/tdx.h: tdx_gn_apply_encoded == tdx_encode_fwd + tdx_gn_apply(res = its output, act = 1), bit for bit;
    shapes: one voxel, fewer voxels than a trip, full trips + a ragged tail, many blocks, narrow / wide rows."""
    from turbdiff_amd import _lib as L, ops

    d = dev()
    G = 8
    V = grid[0] * grid[1] * grid[2]
    C = 2 * D if with_c else D
    x = rnd(B, 4, *grid, seed=1).to(d)
    c = rnd(4, *grid, seed=2).to(d) if with_c else None
    wx, bx = rnd(D, 4, 1, 1, 1, seed=3).to(d), rnd(D, seed=4).to(d)
    wc, bc = (rnd(D, 4, 1, 1, 1, seed=5).to(d), rnd(D, seed=6).to(d)) if with_c else (None, None)
    h2 = rnd(B, *grid, C, seed=7).to(d).to(dtype)
    stats = torch.stack((rnd(B, G, seed=8) * 0.1, rnd(B, G, seed=9).abs() + 0.5), dim=-1).contiguous().to(d)
    gamma, beta = rnd(C, seed=10).to(d), rnd(C, seed=11).to(d)
    code = L.dtype_code(dtype)

    res = ops.encode(x, c, wx, bx, wc, bc, dtype)
    ref = torch.empty_like(h2)
    L.call("tdx_gn_apply", L.ptr(h2), L.ptr(stats), L.ptr(gamma), L.ptr(beta), None, None, L.ptr(res), L.ptr(ref), B, V, C, G,
           1, code, L.stream())
    out = torch.empty_like(h2)
    w2 = lambda w: None if w is None else w.reshape(D, 4).contiguous()
    wx2, wc2 = w2(wx), w2(wc)
    L.call("tdx_gn_apply_encoded", L.ptr(h2), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(x), 4, L.ptr(wx2), L.ptr(bx),
           L.ptr(c), 4 if with_c else 0, L.ptr(wc2), L.ptr(bc), L.ptr(out), B, V, D, G, code, L.stream())
    assert torch.equal(out, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float16])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("B,grid", [(2, (13, 9, 11)), (1, (1, 1, 1)), (3, (5, 1, 7)), (1, (33, 32, 32))])
def test_gn_apply_decode_equals_apply_then_decode_bitwise(dtype, C, B, grid):
    """include/tdx.h: tdx_gn_apply_decode == tdx_gn_apply(res, act = 1) + tdx_decode_fwd, bit for bit; shapes: one voxel,
    fewer voxels than a trip, full trips + a ragged tail, many blocks."""
    from turbdiff_amd import _lib as L, ops

    d = dev()
    G = 8
    V = grid[0] * grid[1] * grid[2]
    h2 = rnd(B, *grid, C, seed=1).to(d).to(dtype)
    res = rnd(B, *grid, C, seed=2).to(d).to(dtype)
    stats = torch.stack((rnd(B, G, seed=8) * 0.1, rnd(B, G, seed=9).abs() + 0.5), dim=-1).contiguous().to(d)
    gamma, beta = rnd(C, seed=10).to(d), rnd(C, seed=11).to(d)
    w, bias = rnd(4, C, 1, 1, 1, seed=12).to(d), rnd(4, seed=13).to(d)
    code = L.dtype_code(dtype)
    y = torch.empty_like(h2)
    L.call("tdx_gn_apply", L.ptr(h2), L.ptr(stats), L.ptr(gamma), L.ptr(beta), None, None, L.ptr(res), L.ptr(y), B, V, C, G, 1,
           code, L.stream())
    ref = ops.decode(y, w, bias)
    out = torch.empty_like(ref)
    w2 = w.reshape(4, C).contiguous()
    L.call("tdx_gn_apply_decode", L.ptr(h2), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(res), L.ptr(w2), L.ptr(bias),
           L.ptr(out), B, V, C, G, 4, code, L.stream())
    assert torch.equal(out, ref)


@pytest.mark.parametrize("l1", [False, True])
def test_masked_loss(l1):
    from turbdiff_amd import ops

    shape = (3, 4, 7, 6, 5)
    e, n = rnd(*shape, seed=1), rnd(*shape, seed=2)
    V = 210
    idx = _mask_idx(V)
    er = e.clone().requires_grad_()
    err = (er - n).abs() if l1 else (er - n) ** 2
    ref = err.flatten(-3)[..., idx].flatten(1).mean(1).mean()
    ref.backward()
    d = dev()
    ed = e.to(d).requires_grad_()
    loss = ops.masked_loss(ed, n.to(d), ops.cell_mask(idx.to(d), V), idx.numel(), l1=l1)
    (loss * 2).backward()
    assert abs(loss.item() - ref.item()) < 1e-6 * abs(ref.item())
    assert rel_l2(ed.grad.cpu(), 2 * er.grad) < 1e-6


def test_philox_randn_equals_the_published_generator():
    """tdx_randn / tdx_randn_batched draw Philox4x32-10 words with counter = (offset + i, trajectory stream id) and key =
    seed, then Box-Muller: against tests/philox_ref.py (numpy, pinned to Random123's known-answer vectors in the CPU
    suite).  Tolerance: the kernel's fast log / sincos."""
    from philox_ref import normals
    from turbdiff_amd import ops

    d = dev()
    seed, sid, off0, n = (0x1234 << 32) | 0x9ABCDEF0, (77 << 32) | 5, (1 << 33) + 12345, 4099
    off = torch.full((1,), off0, dtype=torch.int64, device=d)
    a = ops.randn_philox(torch.empty(n, device=d), seed, sid, off).cpu().double().numpy()
    ref = normals(n, seed, sid, off0)
    assert abs(a - ref).max() < 2e-4 and int(off) == off0 + (n + 3) // 4
    sids = torch.tensor([sid, 3], dtype=torch.int64, device=d)
    off.fill_(off0)
    b = ops.randn_philox_batched(torch.empty(2, n, device=d), seed, sids, off).cpu().double().numpy()
    assert abs(b[0] - ref).max() < 2e-4 and abs(b[1] - normals(n, seed, 3, off0)).max() < 2e-4


def test_philox_randn_moments_and_replay():
    from turbdiff_amd import ops

    d = dev()
    off = torch.zeros(1, dtype=torch.int64, device=d)
    a = ops.randn_philox(torch.empty(1 << 20, device=d), 1234, 7, off)
    assert off.item() == (1 << 18)
    assert abs(a.mean().item()) < 5e-3 and abs(a.std().item() - 1) < 5e-3
    assert abs((a**4).mean().item() - 3) < 0.05
    off.zero_()
    b = ops.randn_philox(torch.empty(1 << 20, device=d), 1234, 7, off)
    assert torch.equal(a, b)  # same (seed, stream, offset) -> same numbers
    c = ops.randn_philox(torch.empty(1 << 20, device=d), 1234, 8, torch.zeros(1, dtype=torch.int64, device=d))
    assert abs((a * c).mean().item()) < 5e-3  # other trajectory stream: independent


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("D", [8, 32])
def test_encode_decode_fused(dtype, with_c, D):
    """encode_x / encode_c_local / decode.1 fused with the layout changes (ddpm.py:495-505)"""
    from turbdiff_amd import ops

    B, X, Y, Z = 2, 7, 5, 6
    x = rnd(B, 4, X, Y, Z, seed=1)
    c = rnd(4, X, Y, Z, seed=2)
    wx, bx = rnd(D, 4, 1, 1, 1, seed=3, scale=0.5), rnd(D, seed=4)
    wc, bc = rnd(D, 4, 1, 1, 1, seed=5, scale=0.5), rnd(D, seed=6)
    Dt = 2 * D if with_c else D
    gy = q(rnd(B, Dt, X, Y, Z, seed=7), dtype)
    leaves = [t.double().requires_grad_() for t in (c, wx, bx, wc, bc)]
    cr, wxr, bxr, wcr, bcr = leaves
    yr = F.conv3d(x.double(), wxr, bxr)
    if with_c:
        yr = torch.cat((yr, F.conv3d(cr[None], wcr, bcr).expand(B, -1, -1, -1, -1)), dim=1)
    yr.backward(gy.double())
    d = dev()
    cd = c.to(d).requires_grad_()
    wxd, bxd, wcd, bcd = (t.to(d).requires_grad_() for t in (wx, bx, wc, bc))
    assert ops.encode_supported(x.to(d), cd if with_c else None, wxd)
    y = ops.encode(x.to(d), cd if with_c else None, wxd, bxd, wcd if with_c else None, bcd if with_c else None, dtype)
    y.backward(nvc(gy).to(d).to(dtype))
    tol = tol_for(dtype)
    assert rel_l2(ncv(y.float().cpu()), yr) < tol
    assert rel_l2(wxd.grad.cpu(), wxr.grad) < 1e-4 and rel_l2(bxd.grad.cpu(), bxr.grad) < 1e-4
    if with_c:
        assert rel_l2(wcd.grad.cpu(), wcr.grad) < 1e-4 and rel_l2(bcd.grad.cpu(), bcr.grad) < 1e-4
        assert rel_l2(cd.grad.cpu(), cr.grad) < 1e-4
    # decode
    h = q(rnd(B, D, X, Y, Z, seed=8), dtype)
    w, b = rnd(4, D, 1, 1, 1, seed=9, scale=0.3), rnd(4, seed=10)
    g4 = rnd(B, 4, X, Y, Z, seed=11)
    hr, wr, br = h.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    F.conv3d(hr, wr, br).backward(g4.double())
    hd = nvc(h).to(d).to(dtype).requires_grad_()
    wd, bd = w.to(d).requires_grad_(), b.to(d).requires_grad_()
    out = ops.decode(hd, wd, bd)
    assert out.shape == (B, 4, X, Y, Z) and out.dtype == torch.float32
    out.backward(g4.to(d))
    assert rel_l2(out.cpu(), F.conv3d(hr, wr, br)) < 1e-5
    assert rel_l2(ncv(hd.grad.float().cpu()), hr.grad) < tol
    assert rel_l2(wd.grad.cpu(), wr.grad) < 1e-4 and rel_l2(bd.grad.cpu(), br.grad) < 1e-4


@pytest.mark.parametrize("case", [(2, 64, 0, 64, 9, 10, 7, 8), (1, 32, 32, 32, 8, 8, 8, 8), (2, 16, 0, 96, 5, 4, 3, 1), (1, 8, 0, 16, 6, 5, 4, 8)])
@pytest.mark.parametrize("dtype,impl,exact", [
    pytest.param(dt, impl, exact, id=f"dtype{i}-{impl}" + ("-exact" if exact else ""))
    for exact in (False, True) for i, dt, impl in ((0, torch.float32, "auto"), (1, torch.float32, "split"), (2, torch.bfloat16, "auto"))])
def test_conv3_with_fused_gn_statistics(case, dtype, impl, exact, monkeypatch):
    """tdx_conv3_fwd_gn: statistics accumulated in the conv epilogue == the streaming
    statistics pass over the stored conv output (ragged bricks included).

    exact: x and w in {-1, 0, 1} with at most 8 taps per output channel, an integer bias in [-2, 2]: |y| <= 10 is an integer,
    exact in bf16 and in every partial sum, so y must EQUAL the float64 convolution and the statistics (32 replicas of f64
    atomics, gn_stats_finalize with R = 32) are exact sums: 1 ulp of float32 from the float64 statistics of y, the rounding of
    the final cast (tests/gn_reference.py).  A voxel of a ragged brick counted twice or not at all moves them by far more."""
    from turbdiff_amd import ops

    B, C1, C2, Cout, X, Y, Z, G = case
    d = dev()
    monkeypatch.setenv("TDX_CONV_IMPL", impl)
    if exact:
        import gn_reference as R

        gen = torch.Generator().manual_seed(8)
        ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
        x1c, x2c = ints(-1, 1, B, X, Y, Z, C1), ints(-1, 1, B, X, Y, Z, C2) if C2 else None
        taps = 27 * (C1 + C2)
        wc = torch.zeros(Cout, taps)
        for o in range(Cout):
            wc[o, torch.randperm(taps, generator=gen)[:8]] = ints(0, 1, 8) * 2 - 1
        wc, bc = wc.reshape(Cout, C1 + C2, 3, 3, 3), ints(-2, 2, Cout)
        xin = ncv(x1c if x2c is None else torch.cat((x1c, x2c), dim=-1)).double()
        y64 = nvc(F.conv3d(F.pad(xin, (1,) * 6, mode="replicate"), wc.double(), bc.double()))
        assert y64.abs().max() <= 10 and torch.equal(y64, y64.round())  # the precondition: integers that bf16 holds
        y, stats = ops.conv3_gn_stats(x1c.to(d).to(dtype), wc.to(d), bc.to(d), G, 1e-5, x2=None if x2c is None else x2c.to(d).to(dtype))
        assert torch.equal(y.double().cpu(), y64)
        want = R.stats(y64.reshape(B, -1, Cout), G, R.f32(1e-5)).float()
        assert int(R.ulp_distance(stats.cpu(), want).max()) <= 1
        return
    x1 = rnd(B, X, Y, Z, C1, seed=1).to(d).to(dtype)
    x2 = rnd(B, X, Y, Z, C2, seed=2).to(d).to(dtype) if C2 else None
    w = rnd(Cout, C1 + C2, 3, 3, 3, seed=3, scale=0.05).to(d)
    b = rnd(Cout, seed=4).to(d)
    gamma, beta = (1 + 0.2 * rnd(Cout, seed=5)).to(d), (0.1 * rnd(Cout, seed=6)).to(d)
    y, stats = ops.conv3_gn_stats(x1, w, b, G, 1e-5, x2=x2)
    y_ref = ops.conv3(x1, w, b, x2=x2)
    assert torch.equal(y, y_ref)
    yr = ncv(y.float().cpu()).double().reshape(B, G, -1)
    mean, var = yr.mean(-1), yr.var(-1, unbiased=False)
    assert torch.allclose(stats[..., 0].cpu().double(), mean, rtol=1e-4, atol=1e-5)
    assert torch.allclose(stats[..., 1].cpu().double(), (var + 1e-5).rsqrt(), rtol=1e-4)
    a = ops.gn_film_silu(y, gamma, beta, G, stats=stats)
    a_ref = ops.gn_film_silu(y, gamma, beta, G)
    assert rel_l2(a.float(), a_ref.float()) < 1e-5


@pytest.mark.parametrize("N", [256, 257, 319, 511, 1000, 1023, 4096])
def test_attention_mfma_forward(N, monkeypatch):
    """bf16 MFMA flash attention (used for N >= 128) vs the oracle on the same bf16 inputs"""
    from turbdiff_amd import _lib as L, ops

    B, H, D = 2, 4, 32

    def family():  # what a call on this stream runs under the switches as they are now
        L.ensure_scratch()
        return L.attn_plan(B, N, H, D, L.BF16)["fwd"]

    qkv = q(rnd(B, N, 3 * H * D, seed=1), torch.bfloat16)
    qq, kk, vv = (p.reshape(B, N, H, D).transpose(1, 2).double() for p in qkv.chunk(3, dim=-1))
    ref = O.sdpa(qq, kk, vv).transpose(1, 2).reshape(B, N, H * D)
    qd = qkv.to(dev()).bfloat16()
    assert family() == "mfma"
    out = ops.attention(qd, H)
    assert rel_l2(out.float().cpu(), ref) < 1e-2
    # the vector-ALU kernel on the same input (exact fp32 softmax): agree to bf16 rounding
    monkeypatch.setenv("TDX_ATTN_IMPL", "vector")
    assert family() == "vector"
    out_v = ops.attention(qd, H)
    assert rel_l2(out.float(), out_v.float()) < 1e-2
    # backward (vector-ALU kernels, driven by the MFMA forward's out / lse)
    monkeypatch.delenv("TDX_ATTN_IMPL")
    if N <= 1000:
        refq = qkv.double().requires_grad_()
        q2, k2, v2 = (p.reshape(B, N, H, D).transpose(1, 2) for p in refq.chunk(3, dim=-1))
        go = q(rnd(B, N, H * D, seed=2), torch.bfloat16)
        O.sdpa(q2, k2, v2).transpose(1, 2).reshape(B, N, H * D).backward(go.double())
        qg = qd.clone().requires_grad_()
        ops.attention(qg, H).backward(go.to(dev()).bfloat16())
        assert rel_l2(qg.grad.float().cpu(), refq.grad) < 3e-2
        # the MFMA flash backward against the row-wise (exact fp32 softmax) kernels, per gradient
        monkeypatch.setenv("TDX_ATTN_IMPL", "vector")
        qv = qd.clone().requires_grad_()
        ops.attention(qv, H).backward(go.to(dev()).bfloat16())
        monkeypatch.delenv("TDX_ATTN_IMPL")
        for name, a, b in zip("qkv", qg.grad.float().chunk(3, dim=-1), qv.grad.float().chunk(3, dim=-1)):
            assert rel_l2(a, b) < 1.5e-2, (name, N)


def test_attention_full_config5_size(monkeypatch):
    """BASELINE config 5: N = 96*32*24 = 73 728 tokens, 4 heads x 32 (too large for the CPU
    oracle's N x N matrix): MFMA kernel vs the exact vector-ALU kernel on a query subset is
    replaced by two size-independent properties -- softmax rows sum to one (V = const gives
    O = const) and permuting the keys/values together leaves the output unchanged."""
    from turbdiff_amd import ops

    B, H, D, N = 1, 4, 32, 96 * 32 * 24
    d = dev()
    g = torch.Generator(device=d).manual_seed(0)
    qkv = torch.randn(B, N, 3 * H * D, device=d, generator=g).bfloat16()
    out = ops.attention(qkv, H)
    assert torch.isfinite(out.float()).all()
    # (1) constant V -> output equals that constant
    qc = qkv.clone()
    qc[..., 2 * H * D:] = 0.75
    oc = ops.attention(qc, H)
    assert (oc.float() - 0.75).abs().max().item() < 8e-3
    # (2) key/value permutation invariance
    perm = torch.randperm(N, device=d, generator=g)
    qp = qkv.clone()
    qp[:, :, H * D:] = qkv[:, perm, H * D:]
    op = ops.attention(qp, H)
    assert rel_l2(op.float(), out.float()) < 5e-3
    # (3) exact vector kernel on the same input, first 4096 queries only would need a sliced API;
    #     instead compare full outputs at a reduced size inside test_attention_mfma_forward
    # (4) MFMA flash backward at full size: softmax rows sum to one, so sum_keys dV = sum_queries dO per
    #     (head, d); and the gradient is invariant under the same key/value permutation
    qg = qkv.clone().requires_grad_()
    go = torch.randn(B, N, H * D, device=d, generator=g).bfloat16()
    ops.attention(qg, H).backward(go)
    dq, dk, dv = qg.grad.float().chunk(3, dim=-1)
    assert torch.isfinite(qg.grad.float()).all()
    assert rel_l2(dv.sum(1), go.float().sum(1)) < 5e-3
    qpg = qp.clone().requires_grad_()
    ops.attention(qpg, H).backward(go)
    dqp, dkp, dvp = qpg.grad.float().chunk(3, dim=-1)
    assert rel_l2(dqp, dq) < 1.5e-2 and rel_l2(dkp, dk[:, perm]) < 1.5e-2 and rel_l2(dvp, dv[:, perm]) < 1.5e-2


def test_attention_config5_rows_vs_oracle():
    """BASELINE config 5 (N = 96*32*24 = 73 728 tokens, 4 heads x 32) against the oracle on a SUBSET of query rows:
    softmax(q_i K^T / sqrt(d)) V for 256 random queries x all keys, evaluated by the CPU oracle's SDPA
    restatement (reference attention.py:9-15) in fp32 on the same bf16-rounded inputs."""
    from oracle import turbdiff_oracle as O
    from turbdiff_amd import ops

    B, H, D, N = 1, 4, 32, 96 * 32 * 24
    d = dev()
    g = torch.Generator(device=d).manual_seed(11)
    qkv = torch.randn(B, N, 3 * H * D, device=d, generator=g).bfloat16()
    out = ops.attention(qkv, H).float().cpu()          # (B, N, H*D), head-major channels
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(12))[:256]
    q, k, v = qkv.float().cpu().reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)  # each (B, H, N, D)
    ref = O.sdpa(q[:, :, rows], k, v)                  # (B, H, 256, D)
    got = out.reshape(B, N, H, D)[:, rows].permute(0, 2, 1, 3)
    assert rel_l2(got, ref) < 6e-3                     # bf16 P and V operands, fp32 accumulation
    assert (got - ref).abs().max().item() < 2e-2


@pytest.mark.parametrize("N", [144, 333, 1000, 4096])
def test_attention_fp16_operands(N, monkeypatch):
    """BASELINE configs[4] names fp16 MFMA QK^T / AV: the matrix-core attention kernels with fp16 tensors and fp16
    operands (tdx_attn_fwd / tdx_attn_bwd, dtype TDX_F16: 11 significand bits in K, V and P instead of bf16's 8).
    Forward and all three gradients against the fp64 oracle on the same fp16-rounded inputs at 2e-3 / 5e-3 -- four
    times tighter than the bf16 kernels' tolerances; the row-wise kernels (short sequences, TDX_ATTN_IMPL=vector) too."""
    from turbdiff_amd import ops

    B, H, D = 2, 4, 32
    qkv = rnd(B, N, 3 * H * D, seed=1).half()
    refq = qkv.double().requires_grad_()
    q2, k2, v2 = (p.reshape(B, N, H, D).transpose(1, 2) for p in refq.chunk(3, dim=-1))
    go = rnd(B, N, H * D, seed=2).half()
    ref = O.sdpa(q2, k2, v2).transpose(1, 2).reshape(B, N, H * D)
    ref.backward(go.double())
    for impl in ("mfma", "vector"):
        if impl == "vector":
            monkeypatch.setenv("TDX_ATTN_IMPL", "vector")
        from turbdiff_amd import _lib as L

        L.ensure_scratch()
        plan = L.attn_plan(B, N, H, D, L.F16)
        assert (plan["fwd"], plan["bwd"]) == (impl, impl)
        qd = qkv.to(dev()).requires_grad_()
        out = ops.attention(qd, H)
        assert out.dtype == torch.float16
        out.backward(go.to(dev()))
        assert rel_l2(out.float().cpu(), ref.detach()) < 2e-3, impl
        for name, a, b in zip("qkv", qd.grad.float().cpu().chunk(3, dim=-1), refq.grad.chunk(3, dim=-1)):
            assert rel_l2(a, b) < 5e-3, (impl, name)
    monkeypatch.delenv("TDX_ATTN_IMPL")


def _growing_scores_and_loose_norm_bound(B, H, N, dtype, tol, monkeypatch, streamk_runs, ref_device="cpu"):
    """The matrix-core forward's lazy running maximum (round 5): scores that keep GROWING along the key index (every
    tile outgrows the stale maximum: the raise path runs over and over), an outlier key of huge norm that no query
    aligns with (the Cauchy-Schwarz bound |q| max|k| is loose by far more than the allowance: the per-tile check must
    stay on), queries of very different norms in one wave, and a ragged last tile -- against the fp64 oracle on the same
    rounded inputs; with the norm bound switched off (TDX_ATTN_BOUND=0: always checking) and with the stream-K schedule
    forced off, bit-identical results are not required, the tolerance is.  The library's plan must say what each
    environment asks for: the bound off under TDX_ATTN_BOUND=0, stream-K on only where `streamk_runs` and not under
    TDX_ATTN_STREAMK=0.  ref_device: where the fp64 reference is evaluated."""
    from turbdiff_amd import _lib as L, ops

    D = 32
    q, k, v = growing_scores_qkv(B, N, H, D, seed=5)
    qkv = torch.cat([t.reshape(B, N, H * D) for t in (q, k, v)], dim=-1).to(dtype)
    qd, kd, vd = (t.reshape(B, N, H, D).transpose(1, 2).double().to(ref_device) for t in qkv.chunk(3, dim=-1))
    ref = O.sdpa(qd, kd, vd).transpose(1, 2).reshape(B, N, H * D).cpu()
    lse_ref = torch.logsumexp(qd @ kd.transpose(-1, -2) / D**0.5, dim=-1).cpu()  # (B, H, N)
    qd, kd, vd = qd.cpu(), kd.cpu(), vd.cpu()
    for env in ({}, {"TDX_ATTN_BOUND": "0"}, {"TDX_ATTN_STREAMK": "0"}):
        for kk, vv in env.items():
            monkeypatch.setenv(kk, vv)
        L.ensure_scratch()
        plan = L.attn_plan(B, N, H, D, L.dtype_code(dtype))
        assert (plan["fwd"], plan["bound"], plan["streamk"]) == ("mfma", int("TDX_ATTN_BOUND" not in env and B * H <= 256),
                                                                 int(streamk_runs and "TDX_ATTN_STREAMK" not in env)), (env, plan)
        x = qkv.to(dev()).requires_grad_()
        out = ops.attention(x, H)
        assert torch.isfinite(out).all()
        assert rel_l2(out.float().cpu(), ref) < tol, (env, rel_l2(out.float().cpu(), ref))
        out.backward(torch.ones_like(out))
        assert torch.isfinite(x.grad).all()
        # the log-sum-exp the backward pass consumes, straight from the entry point
        xd = qkv.to(dev())
        o2 = torch.empty(B, N, H * D, dtype=dtype, device=dev())
        lse = torch.empty(B, H, N, dtype=torch.float32, device=dev())
        L.call("tdx_attn_fwd", L.ptr(xd), L.ptr(o2), L.ptr(lse), B, N, H, D, L.dtype_code(dtype), L.stream())
        assert torch.equal(o2, out.detach())
        # (the kernels round q * log2(e) / sqrt(d) to the operand format once more: a score carries an error of up to
        # 2^-9 |q| |k| / sqrt(d) with bf16 operands, 2^-12 with fp16 -- |q| |k| / sqrt(d) reaches ~200 here)
        err = (lse.cpu().double() - lse_ref).abs()
        ulp = 2.0**-9 if dtype == torch.bfloat16 else 2.0**-12
        kmax = kd.norm(dim=-1).amax(dim=-1, keepdim=True)                       # (B, H, 1)
        assert (err <= 2e-2 + ulp * qd.norm(dim=-1) * kmax / D**0.5).all(), (env, err.max())
        # against the SAME arithmetic in fp64 (q * log2(e) / sqrt(d) rounded to the operand format first) the kernel's
        # log-sum-exp is exact to fp32 / operand-rounding-of-P noise
        qs = (qd.float() * (1.4426950408889634 / D**0.5)).to(dtype).double()
        lse_same = torch.logsumexp((qs @ kd.transpose(-1, -2)) / 1.4426950408889634, dim=-1)
        assert (lse.cpu().double() - lse_same).abs().max().item() < 1e-2, env
        for kk in env:
            monkeypatch.delenv(kk)


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 8e-3), (torch.float16, 2e-3)])
@pytest.mark.parametrize("N", [1000, 4096 + 64 * 37 + 5])
def test_attention_growing_scores_and_loose_norm_bound(dtype, tol, N, monkeypatch):
    """B = 2, H = 4: at most 208 query blocks, one workgroup each in every environment (see the helper)"""
    _growing_scores_and_loose_norm_bound(2, 4, N, dtype, tol, monkeypatch, streamk_runs=False)


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 8e-3), (torch.float16, 2e-3)])
def test_attention_growing_scores_stream_k(dtype, tol, monkeypatch):
    """B = 33, H = 4, N = 1000: the smallest shape the stream-K schedule takes (528 query blocks on 512 workgroups, segments
    starting on every key tile, every block merged from partials), at the same tolerances; reference on the device"""
    _growing_scores_and_loose_norm_bound(33, 4, 1000, dtype, tol, monkeypatch, streamk_runs=True, ref_device=dev())


def test_attention_config5_rows_vs_oracle_fp16():
    """The config-5 size itself (N = 73 728, 4 heads x 32) with fp16 operands: 256 oracle rows at 2e-3."""
    from oracle import turbdiff_oracle as O
    from turbdiff_amd import ops

    B, H, D, N = 1, 4, 32, 96 * 32 * 24
    d = dev()
    g = torch.Generator(device=d).manual_seed(11)
    qkv = torch.randn(B, N, 3 * H * D, device=d, generator=g).half()
    out = ops.attention(qkv, H).float().cpu()
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(12))[:256]
    q, k, v = qkv.float().cpu().reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    ref = O.sdpa(q[:, :, rows], k, v)
    got = out.reshape(B, N, H, D)[:, rows].permute(0, 2, 1, 3)
    assert rel_l2(got, ref) < 2e-3
    assert (got - ref).abs().max().item() < 5e-3


@pytest.mark.parametrize("grid", [(18, 10, 10), (10, 18, 9), (9, 10, 18), (14, 18, 18), (6, 9, 10)])
def test_conv3_thin_slab_bricks(grid, monkeypatch):
    """grids with a 1-2 voxel remainder per axis (the reference's real 194x50x50 family) are tiled
    with thin 2x16x8 bricks on permuted axes on big grids: same numbers as the vector-ALU kernels,
    which know no bricks, and as the oracle.  (TDX_CONV3_THIN is read per call: 0 = all-main-brick
    tiling, 2 = thin slabs on grids of any size.)"""
    from turbdiff_amd import ops

    X, Y, Z = grid
    B, Cin, Cout = 2, 32, 64
    x = q(rnd(B, Cin, X, Y, Z, seed=1), torch.bfloat16)
    w = q(rnd(Cout, Cin, 3, 3, 3, seed=2, scale=0.05), torch.bfloat16)
    gy = q(rnd(B, Cout, X, Y, Z, seed=3), torch.bfloat16)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = O.conv3_replicate(xr, wr)
    yr.backward(gy.double())
    outs = {}
    for impl in ("mfma", "direct"):
        monkeypatch.setenv("TDX_CONV_IMPL", impl)
        xd = nvc(x).to(dev()).bfloat16().requires_grad_()
        wd = w.to(dev()).requires_grad_()
        y, stats = ops.conv3_gn_stats(xd, wd, None, 8)
        y.backward(nvc(gy).to(dev()).bfloat16())
        outs[impl] = (y.float(), xd.grad.float(), stats)
        assert rel_l2(ncv(y.float().cpu()), yr) < BF16_TOL
        assert rel_l2(ncv(xd.grad.float().cpu()), xr.grad) < BF16_TOL
        assert rel_l2(wd.grad.cpu(), wr.grad) < BF16_TOL
    assert rel_l2(outs["mfma"][0], outs["direct"][0]) < 3e-3
    assert rel_l2(outs["mfma"][1], outs["direct"][1]) < 3e-3
    assert torch.allclose(outs["mfma"][2], outs["direct"][2], rtol=2e-3, atol=2e-3)


def test_clean_workspace_protocol():
    """TDX_WS_CLEAN (include/tdx.h): with an all-zero workspace the fused-statistics forward and
    the weight gradient give the same results as the self-zeroing calls and leave the workspace
    all-zero, twice in a row."""
    from turbdiff_amd import _lib as L, ops

    torch.manual_seed(0)
    d = torch.device("cuda:0")
    B, X, Y, Z, Ci, Co = 2, 9, 8, 10, 32, 64
    x = torch.randn(B, X, Y, Z, Ci, device=d).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, 3, device=d) * 0.05)
    bias = torch.randn(Co, device=d)
    gy = torch.randn(B, X, Y, Z, Co, device=d).bfloat16()
    wf, _ = ops._packed_conv3(w, torch.bfloat16)
    st = L.stream()

    def fwd(ws, impl):
        y = torch.empty(B, X, Y, Z, Co, device=d, dtype=torch.bfloat16)
        stats = torch.empty(B, 8, 2, device=d)
        L.call("tdx_conv3_fwd_gn", L.ptr(x), Ci, None, 0, L.ptr(wf), L.ptr(bias), L.ptr(y), L.ptr(stats), 8, 1e-5, L.ptr(ws),
               B, X, Y, Z, Co, L.BF16, impl, st)
        return y, stats

    def wgrad(ws, impl):
        gw, gb = torch.empty_like(w), torch.empty(Co, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x), Ci, None, 0, L.ptr(gy), L.ptr(gw), L.ptr(gb), B, X, Y, Z, Co, L.BF16, impl,
               L.ptr(ws), st)
        return gw, gb

    n1, n2 = L.query("tdx_gn_workspace_bytes", B, Co), L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, 0)
    dirty1 = torch.full((n1,), 0x5A, dtype=torch.uint8, device=d)
    dirty2 = torch.full((n2,), 0x5A, dtype=torch.uint8, device=d)
    ref_y, ref_stats = fwd(dirty1, L.CONV_AUTO)
    ref_gw, ref_gb = wgrad(dirty2, L.CONV_AUTO)
    assert rel_l2(ref_gb.cpu(), gy.float().sum((0, 1, 2, 3)).cpu()) < 1e-3
    clean1 = torch.zeros(n1, dtype=torch.uint8, device=d)
    clean2 = torch.zeros(n2, dtype=torch.uint8, device=d)
    for _ in range(2):
        y, stats = fwd(clean1, L.CONV_AUTO | L.WS_CLEAN)
        gw, gb = wgrad(clean2, L.CONV_AUTO | L.WS_CLEAN)
        assert torch.equal(y, ref_y) and rel_l2(stats.cpu(), ref_stats.cpu()) < 1e-6
        assert rel_l2(gw.cpu(), ref_gw.cpu()) < 1e-5 and rel_l2(gb.cpu(), ref_gb.cpu()) < 1e-5
        n_acc = (27 * Ci * Co + Co) * 4  # the accumulator part; the slabs behind it are scratch
        assert int(clean1.count_nonzero()) == 0 and int(clean2[:n_acc].count_nonzero()) == 0


@pytest.mark.parametrize("max_norm", [0.1, None])
def test_clip_radam_matches_torch(max_norm):
    """ClipRAdam == clip_grad_norm_ + torch.optim.RAdam over 8 steps (the first 5 take RAdam's
    un-rectified branch), odd tensor sizes, a parameter without gradient, LR changed mid-way."""
    from turbdiff_amd.optim import ClipRAdam

    torch.manual_seed(0)
    d = torch.device("cuda:0")
    shapes = [(3,), (17, 5), (64, 64, 3, 3, 3), (1,), (40000,), (33, 7, 2)]
    pa = [torch.randn(s, device=d).requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa = torch.optim.RAdam(pa, lr=1e-2)
    ob = ClipRAdam(pb, lr=1e-2, max_norm=max_norm, write_clipped_grads=True)
    for step in range(8):
        gs = [torch.randn(s, device=d) * (3.0 if step % 2 else 0.01) for s in shapes]
        for k, (a, b, g) in enumerate(zip(pa, pb, gs)):
            a.grad, b.grad = (None, None) if k == 3 else (g.clone(), g.clone())
        if step == 4:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 3e-3
        if max_norm:
            ref_norm = torch.nn.utils.clip_grad_norm_(pa, max_norm)
        versions = [b._version for b in pb]
        oa.step()
        ob.step()
        assert all((b._version > v) == (k != 3) for k, (b, v) in enumerate(zip(pb, versions)))
        if max_norm:
            assert abs(ob.last_grad_norm.item() - ref_norm.item()) < 1e-5 * ref_norm.item()
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (step, k, (a - b).abs().max().item())
            if k != 3:
                assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-9)
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for k in sa:
        assert float(sa[k]["step"]) == float(sb[k]["step"])
        assert torch.allclose(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"], rtol=1e-4, atol=1e-12)


def test_clip_radam_parameters_at_different_step_counts():
    """A parameter that receives a gradient only on some steps (a conditional branch of the model) has its own
    step count in torch.optim.RAdam; the fused optimiser follows (one launch per distinct count)."""
    from turbdiff_amd.optim import ClipRAdam

    torch.manual_seed(2)
    d = torch.device("cuda:0")
    shapes = [(9,), (33, 5), (20000,), (7, 3)]
    pa = [torch.randn(s, device=d).requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa, ob = torch.optim.RAdam(pa, lr=1e-2), ClipRAdam(pb, lr=1e-2, max_norm=None)
    for step in range(9):
        for k, (a, b) in enumerate(zip(pa, pb)):
            skip = (k == 1 and step % 2 == 1) or (k == 3 and step < 4)  # parameter 1: every other step; 3: late joiner
            g = torch.randn(a.shape, device=d)
            a.grad, b.grad = (None, None) if skip else (g.clone(), g.clone())
        oa.step()
        ob.step()
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (step, k)
    assert [int(oa.state[p]["step"]) for p in pa] == [int(ob.state[p]["step"]) for p in pb] == [9, 5, 9, 5]


def test_clip_radam_loss_scaling_unscales_skips_and_adapts():
    """ClipRAdam(loss_scale=S) (fp16 training): gradients stored S times too large give the updates and the norm of the
    unscaled reference (clip_grad_norm_ + torch.optim.RAdam); a step with a non-finite gradient changes NOTHING (parameters,
    moments, and -- once its flag has reached the host, two steps later -- the step counters) and halves S; S doubles after
    `scale_growth_interval` clean steps.  Parameter 3 takes no gradients on odd steps (per-parameter step counts)."""
    from turbdiff_amd.optim import ClipRAdam

    torch.manual_seed(3)
    d = torch.device("cuda:0")
    shapes = [(5,), (17, 3), (40000,), (9, 2)]
    pa = [torch.randn(s, device=d).requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa = torch.optim.RAdam(pa, lr=1e-2)
    # sync_flags: every step waits for its own flag (exact step counts right after an overflow, comparable with the
    # reference step by step); the default lazy mode is checked below
    ob = ClipRAdam(pb, lr=1e-2, max_norm=0.5, loss_scale=2.0**12, scale_growth_interval=4, sync_flags=True)
    bad_steps = {3, 4}
    for step in range(12):
        S = ob.loss_scale  # what scale_loss() multiplies this step's loss by
        loss = torch.tensor(1.5, device=d)
        assert ob.scale_loss(loss).item() == 1.5 * S
        gs = [torch.randn(s, device=d) * (2.0 if step % 2 else 0.02) for s in shapes]
        for k, (a, b, g) in enumerate(zip(pa, pb, gs)):
            if k == 3 and step % 2 == 1:
                a.grad, b.grad = None, None
            else:
                a.grad, b.grad = g.clone(), g * S
        if step in bad_steps:
            pb[2].grad[123] = float("inf") if step == 3 else float("nan")
            before = [b.detach().clone() for b in pb]
            ob.step()
            assert all(torch.equal(b, v) for b, v in zip(pb, before)), "a skipped step must not touch the parameters"
            continue
        ref_norm = torch.nn.utils.clip_grad_norm_(pa, 0.5)
        oa.step()
        ob.step()
        assert abs(ob.last_grad_norm.item() - ref_norm.item()) < 1e-5 * ref_norm.item()
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert torch.allclose(a, b, rtol=3e-6, atol=2e-7), (step, k, (a - b).abs().max().item())
    ob.settle()
    assert ob.skipped_steps == 2
    # 12 steps: flags 0-2 clean, 3 and 4 skipped (S: 2^12 -> 2^10), then 7 clean steps = one doubling after 4 (-> 2^11)
    assert ob.loss_scale == 2.0**11 and ob._clean_steps == 3
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for k in sa:
        assert float(sa[k]["step"]) == float(sb[k]["step"]), (k, float(sa[k]["step"]), float(sb[k]["step"]))
        assert torch.allclose(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"], rtol=1e-4, atol=1e-12)
    # the default: flags are read two steps late, never waited for.  Same bookkeeping once settled (scale, skipped steps,
    # step counts); the scale a step's backward ran on is the scale its update divides by, also across a change
    pc = [p.detach().clone().requires_grad_() for p in pa]
    oc = ClipRAdam(pc, lr=1e-2, max_norm=0.5, loss_scale=2.0**12, scale_growth_interval=4)
    norms = []
    for step in range(12):
        S = oc.loss_scale
        for k, c in enumerate(pc):
            c.grad = None if (k == 3 and step % 2 == 1) else torch.full_like(c, 0.25) * S
        if step in bad_steps:
            pc[2].grad[7] = float("inf")
        oc.step()
        if step not in bad_steps:
            norms.append(oc.last_grad_norm.item())
    oc.settle()
    assert oc.skipped_steps == 2 and oc.loss_scale == 2.0**11
    assert [int(oc.state[c]["step"]) for c in pc] == [10, 10, 10, 5]
    full = 0.25 * (sum(c.numel() for c in pc)) ** 0.5
    part = 0.25 * (sum(c.numel() for c in pc[:3])) ** 0.5
    assert all(abs(n - (part if i % 2 else full)) < 1e-4 for i, n in zip([0, 1, 2, 5, 6, 7, 8, 9, 10, 11], norms)), norms


_LS_SHAPES = [(5,), (17, 3), (40000,), (9, 2)]
_LS_BAD = {3: float("inf"), 4: float("nan")}  # the overflow steps of the 12-step schedule


def _ls_schedule(d):
    """The synthetic schedule of the test above: 12 steps of unscaled gradients, alternately large and small."""
    gen = torch.Generator().manual_seed(9)
    return [[(torch.randn(s, generator=gen) * (2.0 if step % 2 else 0.02)).to(d) for s in _LS_SHAPES] for step in range(12)]


def _ls_scaled_step(opt, params, grads, step):
    """One step of the loss-scaling optimiser: gradients S times too large, parameter 3 only on even steps, an overflow in
    parameter 2 on the bad steps."""
    S = opt.loss_scale
    for k, (p, g) in enumerate(zip(params, grads[step])):
        p.grad = None if (k == 3 and step % 2 == 1) else g * S
    if step in _LS_BAD:
        params[2].grad[123] = _LS_BAD[step]
    opt.step()


def _ls_reference_step(opt, params, grads, step):
    """The reference: clip_grad_norm_ + torch.optim.RAdam on the unscaled gradients; an overflow step does not happen."""
    if step in _LS_BAD:
        return
    for k, (p, g) in enumerate(zip(params, grads[step])):
        p.grad = None if (k == 3 and step % 2 == 1) else g.clone()
    torch.nn.utils.clip_grad_norm_(params, 0.5)
    opt.step()


def _ls_params(d):
    gen = torch.Generator().manual_seed(4)
    return [torch.randn(s, generator=gen).to(d).requires_grad_() for s in _LS_SHAPES]


def _through_a_file(sd):
    """What a checkpoint does to a state_dict: torch.save / torch.load (no tensor shared with the live optimiser)."""
    import io

    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


def _ls_optimizer(params, loss_scale=2.0**12):
    from turbdiff_amd.optim import ClipRAdam

    return ClipRAdam(params, lr=1e-2, max_norm=0.5, loss_scale=loss_scale, scale_growth_interval=4)  # lazy flags (the default)


@pytest.mark.parametrize("k", [5, 8])
def test_clip_radam_state_dict_holds_settled_step_counts(k):
    """A state_dict() taken after step k of the schedule -- k = 5: right behind the two overflows, inside the two-step lag of
    their flags -- holds the step counts torch.optim.RAdam holds at that point (the skipped steps taken out), and the
    loss-scaling state of all k steps."""
    d = torch.device("cuda:0")
    grads = _ls_schedule(d)
    pa, pb = _ls_params(d), _ls_params(d)
    oa, ob = torch.optim.RAdam(pa, lr=1e-2), _ls_optimizer(pb)
    for step in range(k):
        _ls_reference_step(oa, pa, grads, step)
        _ls_scaled_step(ob, pb, grads, step)
    sa, sb = oa.state_dict(), ob.state_dict()
    want = {5: [3, 3, 3, 2], 8: [6, 6, 6, 3]}[k]
    assert [int(sa["state"][i]["step"]) for i in range(4)] == want
    assert [float(sb["state"][i]["step"]) for i in range(4)] == [float(w) for w in want]
    # k = 5: flags 1-3 clean, 4 and 5 skipped; k = 8: three more clean steps
    assert sb["loss_scaling"] == {"loss_scale": 2.0**10, "clean_steps": {5: 0, 8: 3}[k], "skipped_steps": 2, "step_index": k}
    for i in range(4):
        assert torch.allclose(sa["state"][i]["exp_avg_sq"], sb["state"][i]["exp_avg_sq"], rtol=1e-4, atol=1e-12)


@pytest.mark.parametrize("k", [5, 8])
def test_clip_radam_resumed_from_a_checkpoint_equals_the_run_that_went_on(k):
    """Loss-scaling mode, flags read lazily: a run takes a checkpoint (state_dict() + parameters) after step k and goes on; a
    fresh optimiser on copies of the parameters loads the checkpoint and runs the remaining steps.  The arithmetic is the
    same, so everything is EQUAL: parameters after every step, moments, per-parameter step counts, loss scale, skipped and
    clean step counts.  (state_dict() settles the outstanding flags -- the run that goes on continues from settled counters,
    like the resumed one; k = 5 is inside the two-step lag behind the overflows of steps 3 and 4.)"""
    d = torch.device("cuda:0")
    grads = _ls_schedule(d)
    pa = _ls_params(d)
    oa = _ls_optimizer(pa)
    trace = {}
    for step in range(12):
        if step == k:
            saved = _through_a_file(oa.state_dict())
            saved_params = [p.detach().clone() for p in pa]
        _ls_scaled_step(oa, pa, grads, step)
        trace[step] = [p.detach().clone() for p in pa]
    pb = [p.clone().requires_grad_() for p in saved_params]
    ob = _ls_optimizer(pb)  # starts at the initial scale; the checkpoint must bring the scale of step k
    ob.load_state_dict(saved)
    for step in range(k, 12):
        _ls_scaled_step(ob, pb, grads, step)
        for i, (b, a) in enumerate(zip(pb, trace[step])):
            assert torch.equal(b.detach(), a), (step, i, (b.detach() - a).abs().max().item())
    oa.settle()
    ob.settle()
    assert (ob.loss_scale, ob.skipped_steps, ob._clean_steps) == (oa.loss_scale, oa.skipped_steps, oa._clean_steps) == (2.0**11, 2, 3)
    for i, (a, b) in enumerate(zip(pa, pb)):
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]) == [10, 10, 10, 5][i], (i, float(sa["step"]), float(sb["step"]))
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), i


def test_clip_radam_state_dicts_interchange_with_torch_radam_under_loss_scaling():
    """The module's promise with loss scaling on, at k = 5 (behind the overflows): (a) a ClipRAdam state_dict loads into
    torch.optim.RAdam -- its loss-scaling entry sits where torch does not look -- and torch goes on as the reference that
    ran from the start does; (b) a torch.optim.RAdam state_dict loads into a loss-scaling ClipRAdam, which goes on as torch
    does and keeps its own scale (the dictionary has none)."""
    d = torch.device("cuda:0")
    grads = _ls_schedule(d)
    k = 5
    pr, pc = _ls_params(d), _ls_params(d)
    ref, oc = torch.optim.RAdam(pr, lr=1e-2), _ls_optimizer(pc)
    for step in range(k):
        _ls_reference_step(ref, pr, grads, step)
        _ls_scaled_step(oc, pc, grads, step)
    from_clip, from_torch = _through_a_file(oc.state_dict()), _through_a_file(ref.state_dict())
    # (a) ClipRAdam -> torch
    pt = [p.detach().clone().requires_grad_() for p in pc]
    ot = torch.optim.RAdam(pt, lr=1e-2)
    ot.load_state_dict(from_clip)
    # (b) torch -> ClipRAdam, at a scale of its own
    pd = [p.detach().clone().requires_grad_() for p in pr]
    od = _ls_optimizer(pd, loss_scale=2.0**10)
    od.load_state_dict(from_torch)
    for step in range(k, 12):
        _ls_reference_step(ref, pr, grads, step)
        _ls_reference_step(ot, pt, grads, step)
        _ls_scaled_step(od, pd, grads, step)
        for i, r in enumerate(pr):
            assert torch.allclose(pt[i], r, rtol=3e-6, atol=2e-7), ("clip->torch", step, i, (pt[i] - r).abs().max().item())
            assert torch.allclose(pd[i], r, rtol=3e-6, atol=2e-7), ("torch->clip", step, i, (pd[i] - r).abs().max().item())
    od.settle()
    assert od.loss_scale == 2.0**11 and od.skipped_steps == 0 and od._clean_steps == 3  # seven clean steps from 2^10
    for i, r in enumerate(pr):
        assert float(ref.state[r]["step"]) == float(ot.state[pt[i]]["step"]) == float(od.state[pd[i]]["step"]) == [10, 10, 10, 5][i], i
        for other in (ot.state[pt[i]], od.state[pd[i]]):
            assert torch.allclose(ref.state[r]["exp_avg_sq"], other["exp_avg_sq"], rtol=1e-4, atol=1e-12), i


def test_clip_radam_with_bucket_view_gradients():
    """Gradients that are views into a flat all-reduce bucket (parallel.BucketedDataParallel.finish) are
    only 4-byte aligned: the fused optimiser must not assume 16-byte alignment."""
    from turbdiff_amd.optim import ClipRAdam

    torch.manual_seed(1)
    d = torch.device("cuda:0")
    shapes = [(5,), (7, 3), (1001,), (64, 3, 3)]
    pa = [torch.randn(s, device=d).requires_grad_() for s in shapes]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa, ob = torch.optim.RAdam(pa, lr=1e-2), ClipRAdam(pb, lr=1e-2, max_norm=0.5)
    for step in range(7):
        flat = torch.randn(1 + sum(p.numel() for p in pa), device=d)
        off = 1  # odd element offset -> 4-byte aligned views
        for a, b in zip(pa, pb):
            n = a.numel()
            a.grad = flat[off : off + n].view_as(a).clone()
            b.grad = flat[off : off + n].view_as(b)
            off += n
        torch.nn.utils.clip_grad_norm_(pa, 0.5)
        oa.step()
        ob.step()
        for a, b in zip(pa, pb):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7)


def test_stage_scaled_moves_a_bucket_in_one_launch():
    """tdx_stage_scaled (the gradient staging of parallel.BucketedDataParallel): dst = src * scale over many tensors per
    launch -- bit-exact against torch.mul for odd sizes, slices that are only 4-byte aligned, missing gradients (src NULL ->
    zeros), a gradient that already IS its slice (scaled in place), empty tensors and more items than one launch holds."""
    from turbdiff_amd import _lib as L

    torch.manual_seed(3)
    d = torch.device("cuda:0")
    sizes = [1, 3, 4, 5, 8191, 8192, 8193, 0, 100003, 17, 64 * 3 * 27, 1 << 20] + [7 + 13 * k for k in range(70)]
    srcs = [torch.randn(n, device=d) for n in sizes]
    flat = torch.full((sum(sizes) + len(sizes) + 1,), float("nan"), device=d)
    tab, views, off = (L.StageItem * len(sizes))(), [], 1
    for k, (n, g) in enumerate(zip(sizes, srcs)):
        v = flat[off : off + n]  # odd offsets: some slices 16-byte aligned, most not
        off += n + (k % 2)
        views.append(v)
        if k == 5:  # no gradient this step
            tab[k].src = None
        elif k == 8:  # the gradient already lives in its slice
            v.copy_(g)
            tab[k].src = v.data_ptr()
        else:
            tab[k].src = g.data_ptr()
        tab[k].dst, tab[k].n = v.data_ptr(), n
    for scale in (0.125, 1.0 / 3.0):
        views[8].copy_(srcs[8])
        L.call("tdx_stage_scaled", tab, len(sizes), scale, L.stream())
        for k, (g, v) in enumerate(zip(srcs, views)):
            want = torch.zeros_like(g) if k == 5 else g * scale
            assert torch.equal(v, want), (k, sizes[k])
    assert torch.isnan(flat[0]) and torch.isnan(flat[off:]).all()  # nothing written outside the slices
    with pytest.raises(RuntimeError):
        bad = (L.StageItem * 1)()
        bad[0].src, bad[0].dst, bad[0].n = srcs[0].data_ptr(), None, 1
        L.call("tdx_stage_scaled", bad, 1, 1.0, L.stream())


def _stage_case(kinds, sizes, scale, d):
    """One tdx_stage_scaled call over items of the given kinds ("copy": src != dst, "inplace": src == dst, "null": src NULL ->
    zeros, "empty": n == 0) whose destinations are slices of one NaN-filled buffer at odd element offsets (4-byte alignment
    only) with one NaN guard element between neighbours; every slice bit-exact against torch.mul, every guard still NaN."""
    from turbdiff_amd import _lib as L

    assert len(kinds) == len(sizes)
    gen = torch.Generator().manual_seed(len(kinds))
    sizes = [0 if kind == "empty" else n for kind, n in zip(kinds, sizes)]
    flat = torch.full((1 + sum(n + 1 for n in sizes),), float("nan"), device=d)
    guard = torch.ones(flat.numel(), dtype=torch.bool)
    tab, checks, off = (L.StageItem * len(kinds))(), [], 1
    for k, (kind, n) in enumerate(zip(kinds, sizes)):
        v = flat[off : off + n]
        guard[off : off + n] = False
        off += n + 1
        g = torch.randn(n, generator=gen).to(d)
        if kind == "inplace":
            v.copy_(g)
            tab[k].src = v.data_ptr()
        elif kind == "null":
            v.fill_(7.0)  # must be overwritten with zeros
            tab[k].src = None
        else:
            tab[k].src = g.data_ptr()
        tab[k].dst, tab[k].n = v.data_ptr(), n
        checks.append((k, kind, v, torch.zeros_like(g) if kind == "null" else torch.mul(g, scale), g))  # (g: the source stays alive)
    L.call("tdx_stage_scaled", tab, len(kinds), scale, L.stream())
    torch.cuda.synchronize()
    wrong = [(k, kind, v.numel()) for k, kind, v, want, _ in checks if not torch.equal(v, want)]
    assert not wrong, f"items staged wrongly (position, kind, size): {wrong}"
    assert torch.isnan(flat[guard.to(d)]).all(), "written outside the slices"


@pytest.mark.parametrize("n_empty", [1, 2, 3, 70])
def test_stage_scaled_scales_in_place_items_once_across_launch_boundaries(n_empty):
    """A launch holds 64 NON-EMPTY items; empty items take no slot, so a pass reads more than 64 inputs when some are empty,
    and the next pass has to go on where this one stopped -- not 64 inputs after its start, which stages the overlap a
    second time.  For src != dst that is invisible; a gradient that already lives in its slice (src == dst) would be scaled
    twice.  In-place items at and around input positions 63, 64, 65, 127 and 128, `n_empty` empty items in front of them in
    the first pass, scale 1 / 3 (not idempotent): every one scaled exactly once."""
    d = torch.device("cuda:0")
    around = {p + o for p in (63, 64, 65, 127, 128) for o in (-1, 0, 1)} | set(range(n_empty + 60, n_empty + 70))
    n_items = 140 + n_empty
    empties = set(range(2, 2 + n_empty)) - around if n_empty < 10 else set(range(40, 40 + n_empty)) - around
    assert len(empties) >= min(n_empty, 20) and max(empties) < 63 + n_empty
    kinds = ["empty" if k in empties else "inplace" if k in around else "copy" for k in range(n_items)]
    sizes = [5 + 7 * (k % 11) if k % 9 else 8192 + k for k in range(n_items)]
    _stage_case(kinds, sizes, 1.0 / 3.0, d)


@pytest.mark.parametrize("kinds", [["empty"] * 65, ["empty"] * 200, ["inplace", "copy"] + ["empty"] * 130,
                                   ["copy"] * 64 + ["empty"] * 3, ["empty"] * 64 + ["inplace"], ["empty"] * 100 + ["inplace"] * 70 + ["empty"]],
                         ids=["65-empty", "200-empty", "ends-in-130-empty", "full-launch-then-empty", "64-empty-then-one", "empty-both-ends"])
def test_stage_scaled_lists_of_empty_items(kinds):
    """More than 64 empty items in a row (alone, in front of and behind real items), lists that end in empty items."""
    _stage_case(kinds, [33 + k for k in range(len(kinds))], 1.0 / 3.0, torch.device("cuda:0"))


def test_stage_scaled_mixed_list_of_250_items():
    """250 items mixing missing gradients (src NULL), in-place, ordinary and empty items, 4-byte alignment only, sizes on both
    sides of a block's 8192 elements; the NaN guard elements between the slices stay NaN."""
    gen = torch.Generator().manual_seed(5)
    pick = torch.randint(0, 8, (250,), generator=gen).tolist()
    kinds = [("null", "inplace", "inplace", "empty", "copy", "copy", "copy", "inplace")[p] for p in pick]
    assert min(kinds.count(k) for k in ("null", "inplace", "empty", "copy")) >= 15
    sizes = [[1, 3, 17, 8191, 8192, 8193, 260, 20001][(k * 5 + p) % 8] for k, p in enumerate(pick)]
    _stage_case(kinds, sizes, 1.0 / 3.0, torch.device("cuda:0"))


@pytest.mark.parametrize("C,src,dst", [(24, (5, 4, 3), (9, 9, 17)), (8, (3, 3, 3), (20, 7, 30)), (64, (13, 9, 10), (6, 4, 5)),
                                       (512, (6, 4, 3), (3, 3, 3))])
def test_resize_odd_channel_counts_and_large_factors(C, src, dst):
    """tdx_resize_fwd/bwd on the tile mappings the U-Net grids do not reach: C / 8 not a power of two,
    up-sampling by up to 10x along an axis (z spans of 15 and 28 outputs per input: both up-sampling cases take the generic
    adjoint, not resize_bwd_kernel<T, 12> -- tests/resize_cases.py has the routes), wide channels (4-voxel passes),
    down-sampling."""
    from turbdiff_amd import ops

    torch.manual_seed(0)
    x = torch.randn(2, *src, C, device="cuda:0").requires_grad_()
    y = ops.resize(x, list(dst))
    gy = torch.randn_like(y)
    y.backward(gy)
    xr = x.detach().permute(0, 4, 1, 2, 3).cpu().requires_grad_()
    yr = F.interpolate(xr, size=dst, mode="trilinear", align_corners=True)
    yr.backward(gy.permute(0, 4, 1, 2, 3).cpu())
    assert rel_l2(y.detach().permute(0, 4, 1, 2, 3).cpu(), yr.detach()) < 1e-5
    assert rel_l2(x.grad.permute(0, 4, 1, 2, 3).cpu(), xr.grad) < 1e-5


@pytest.mark.parametrize("grid", [(4, 8, 8), (12, 4, 3), (9, 8, 10)])
def test_conv3_wgrad_split_merge_modes(grid):
    """Weight gradient with few K-splits (per-split slabs, plain stores) and with many (f32 atomics) against
    the vector-ALU kernel, twice on one persistent TDX_WS_CLEAN workspace."""
    from turbdiff_amd import _lib as L

    torch.manual_seed(0)
    d = torch.device("cuda:0")
    B, (X, Y, Z), Ci, Co = 2, grid, 64, 128
    x = torch.randn(B, X, Y, Z, Ci, device=d).bfloat16()
    gy = torch.randn(B, X, Y, Z, Co, device=d).bfloat16()
    st = L.stream()

    def wgrad(ws, impl):
        gw, gb = torch.empty(Co, Ci, 3, 3, 3, device=d), torch.empty(Co, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x), Ci, None, 0, L.ptr(gy), L.ptr(gw), L.ptr(gb), B, X, Y, Z, Co, L.BF16, impl,
               L.ptr(ws), st)
        return gw, gb

    n = L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, 0)
    ref_gw, ref_gb = wgrad(torch.empty(n, dtype=torch.uint8, device=d), L.CONV_DIRECT)
    ws = torch.zeros(n, dtype=torch.uint8, device=d)
    for _ in range(2):
        gw, gb = wgrad(ws, L.CONV_MFMA | L.WS_CLEAN)
        assert rel_l2(gw.cpu(), ref_gw.cpu()) < 1e-5 and rel_l2(gb.cpu(), ref_gb.cpu()) < 1e-5
        assert int(ws[: (27 * Ci * Co + Co) * 4].count_nonzero()) == 0


@pytest.mark.parametrize("mode", ["bf16", "f32s"])
@pytest.mark.parametrize("case", [
    # B, C1, C2, Cout, grid -- the deep levels of the shipped model and ragged / tiny relatives
    (6, 512, 0, 512, (12, 4, 3)), (6, 256, 0, 512, (24, 8, 6)), (6, 512, 512, 256, (24, 8, 6)), (2, 128, 0, 32, (5, 3, 1)),
    (3, 256, 0, 64, (7, 9, 4)), (8, 512, 0, 512, (12, 4, 3)), (1, 160, 0, 96, (13, 7, 6)),
])
def test_conv3_small_grid_kernel_vs_brick_kernels(case, mode, monkeypatch):
    """The small-grid conv (packed M tiles, split K, reduce pass with the halo fold; tdx_conv3_small.hip) against the
    brick kernels + halo-shell kernel it replaces on the deep levels (arena registered vs not), forward with fused
    statistics and data gradient with addends; and both against the fp64 oracle on the smallest case.  bf16 tensors,
    and fp32 tensors with split-precision products (the f32s mode)."""
    from turbdiff_amd import _lib as L, ops

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    dt, DT, IMPL = (torch.bfloat16, L.BF16, L.CONV_AUTO) if mode == "bf16" else (torch.float32, L.F32, L.CONV_SPLIT)
    tols = [4e-3, 1e-3, 4e-3, 6e-3, 6e-3] if mode == "bf16" else [2e-5, 1e-5, 2e-5, 2e-5, 2e-5]
    g = torch.Generator(device=d).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1).to(dt), (rn(B, X, Y, Z, C2).to(dt) if C2 else None)
    w = rn(Co, Ci, 3, 3, 3) * (2.0 / (27 * Ci)) ** 0.5
    bias, gy = rn(Co), rn(B, X, Y, Z, Co).to(dt)
    st = L.stream()
    prev = L._conv_impl_override
    if mode == "f32s":
        L.set_conv_impl("split")  # fp32 weights packed as bf16 hi + lo images
    try:
        wf, wb = ops._packed_conv3(w, dt)
    finally:
        L.set_conv_impl(prev)

    def run():
        y = torch.empty(B, X, Y, Z, Co, device=d, dtype=dt)
        stats = torch.empty(B, 8, 2, device=d)
        ws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, Co), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_fwd_gn", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), L.ptr(bias), L.ptr(y), L.ptr(stats), 8, 1e-5, L.ptr(ws),
               B, X, Y, Z, Co, DT, IMPL | L.WS_CLEAN, st)
        assert int(ws.count_nonzero()) == 0
        y2 = torch.empty_like(y)
        L.call("tdx_conv3_fwd", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), L.ptr(bias), L.ptr(y2), B, X, Y, Z, Co, DT, IMPL, st)
        gx1, gx2 = torch.empty_like(x1), (torch.empty_like(x2) if C2 else None)
        dws = torch.empty(L.query("tdx_conv3_bwd_data_workspace_bytes", B, X, Y, Z, Ci, DT, 0), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_bwd_data_add", L.ptr(gy), L.ptr(wb), L.ptr(gx1), C1, L.ptr(gx2), C2, L.ptr(x1), L.ptr(x2), B, X, Y, Z, Co,
               DT, IMPL, L.ptr(dws), st)
        torch.cuda.synchronize()
        return y, stats, y2, gx1, gx2

    monkeypatch.setenv("TDX_CONV3_SMALL_ROWS", "30000")  # also the 24 x 8 x 6 shapes, which the product leaves to the brick kernels
    arena = L.scratch_arena(d)
    arena[64:].zero_()
    small = run()
    assert int(arena[64:].count_nonzero()) > 0, "the small-grid kernel did not run"
    assert int(arena[:64].count_nonzero()) == 0
    L.load().tdx_set_scratch(None, 0)
    try:
        brick = run()
    finally:
        L._ACTIVE = None
        L.ensure_scratch(d)
    for n, a, b, tol in zip(["y", "stats", "y (plain fwd)", "gx1", "gx2"], small, brick, tols):
        if a is None:
            continue
        assert torch.isfinite(a.float()).all(), n
        assert rel_l2(a.float(), b.float()) < tol, (n, case, mode)
    assert torch.equal(small[0], small[2])
    if X * Y * Z <= 20:  # the oracle on the smallest case: replicate-padded conv and its adjoint in fp64
        xr = torch.cat([x1] + ([x2] if C2 else []), dim=-1).double().cpu().permute(0, 4, 1, 2, 3).requires_grad_()
        yr = O.conv3_replicate(xr, w.double().cpu(), bias.double().cpu())
        yr.backward(gy.double().cpu().permute(0, 4, 1, 2, 3))
        assert rel_l2(small[0].float().cpu().permute(0, 4, 1, 2, 3), yr) < (4e-3 if mode == "bf16" else 2e-5)
        gx = torch.cat([small[3]] + ([small[4]] if C2 else []), dim=-1).float().cpu() - torch.cat([x1] + ([x2] if C2 else []), dim=-1).float().cpu()
        assert rel_l2(gx.permute(0, 4, 1, 2, 3), xr.grad) < (1e-2 if mode == "bf16" else 5e-5)


@pytest.mark.parametrize("mode", ["bf16", "f32", "f32s"])
@pytest.mark.parametrize("case", [(2, 32, 0, 64, (24, 16, 8)), (1, 32, 32, 32, (9, 10, 7)), (2, 64, 0, 32, (1, 5, 4)),
                                  (1, 32, 0, 32, (16, 2, 16))])
def test_conv3_data_gradient_deterministic_shell_route(case, mode, monkeypatch):
    """TDX_SHELL_DETERMINISTIC=1: the halo-shell term goes through one fp32 row per shell position and a fixed-order fold
    (tdx_conv3_shell.hip) instead of atomics on edge and corner voxels.  The data gradient must be bit-identical from run to
    run, agree with the default (atomics) route to rounding noise and with the fp64 oracle (adjoint of the replicate-padded
    conv) -- incl. grids one and two voxels thick, where both faces of an axis fold onto the same plane -- and the
    workspace query must cover the position buffer."""
    import torch.nn.functional as F

    from turbdiff_amd import _lib as L, ops

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    monkeypatch.setenv("TDX_CONV_IMPL", "split" if mode == "f32s" else "auto")
    monkeypatch.setenv("TDX_CONV3_SMALL_ROWS", "1")  # keep the small-grid kernels (no shell launch) out of the way
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=gen) / (27 * Ci) ** 0.5
    gy = q(torch.randn(B, Co, X, Y, Z, generator=gen), dt)
    x1 = torch.zeros(B, X, Y, Z, C1, device=d, dtype=dt, requires_grad=True)
    x2 = torch.zeros(B, X, Y, Z, C2, device=d, dtype=dt, requires_grad=True) if C2 else None
    wd = w.to(d)

    def grad():
        y = ops.conv3(x1, wd, None, x2=x2)
        g = torch.autograd.grad(y, [x1] + ([x2] if C2 else []), nvc(gy).to(d).to(dt))
        return torch.cat([t.float() for t in g], dim=-1).cpu()

    base = grad()
    monkeypatch.setenv("TDX_SHELL_DETERMINISTIC", "1")
    a, b = grad(), grad()
    assert torch.equal(a, b)
    # oracle: adjoint of y = conv3(replicate_pad(x)) in fp64 (the conv is linear, so x = 0 is as good a point as any)
    xr = torch.zeros(B, Ci, X, Y, Z, dtype=torch.float64, requires_grad=True)
    wr = (q(w, dt) if mode == "bf16" else w).double()
    F.conv3d(F.pad(xr, (1,) * 6, mode="replicate"), wr).backward(gy.double())
    ref = nvc(xr.grad.float())
    tol = 4e-3 if mode == "bf16" else (2e-5 if mode == "f32s" else 2e-6)
    assert rel_l2(a, ref) < tol and rel_l2(base, ref) < tol
    # (bf16: the default route's atomics round per add in arrival order; measured 2.5e-3 ... 4.0e-3 on the thin grids)
    assert rel_l2(a, base) < (6e-3 if mode == "bf16" else 1e-6)
    ws = L.query("tdx_conv3_bwd_data_workspace_bytes", B, X, Y, Z, Ci, L.dtype_code(dt), L.conv_impl())
    assert ws >= 2 * ((X + 2) * (Y + 2) + (X + 2) * Z + Y * Z) * B * Ci * 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    # B, C1, C2, Cout, grid: whole 8 x 8 x 8 bricks; one brick per workgroup ... nine per workgroup; one K slice (the composed
    # first conv) ... eight; one / two / four N tiles; 32-wide tiles; two inputs
    (2, 32, 0, 64, (16, 16, 16)), (1, 16, 0, 64, (32, 32, 16)), (3, 64, 0, 64, (64, 32, 32)), (2, 32, 32, 32, (64, 64, 32)),
    (1, 64, 64, 128, (48, 32, 24)), (2, 128, 0, 256, (32, 16, 24)), (5, 32, 0, 32, (32, 32, 32)), (2, 64, 0, 64, (192, 64, 48)),
    (6, 16, 0, 64, (96, 32, 24)),
    # ragged grids (round 4): whole bricks on the ring kernel + 1-2 voxel remainder slabs on the thin-brick kernel --
    # remainders on every axis / on one axis only / 32-wide tiles (16 x 8 x 8 bricks) / the reference's real grid and its level 1
    (1, 64, 0, 64, (50, 26, 18)), (2, 32, 32, 64, (24, 17, 16)), (2, 32, 0, 32, (34, 17, 9)), (1, 16, 0, 64, (194, 50, 50)),
    (2, 64, 64, 128, (97, 25, 25)),
    # 4-deep bricks (round 6; the trailing 4 forces them where 8-deep ones are legal too): level 2 of the benchmark grid at its
    # own channel counts (48 x 16 x 12: 128 -> 256, 256 -> 256, [256 | 256] -> 128), one brick, 32-wide tiles (32 x 8 x 4 bricks),
    # remainders on every axis, a grid both depths can tile
    (6, 128, 0, 256, (48, 16, 12), 4), (2, 256, 0, 256, (48, 16, 12), 4), (1, 256, 256, 128, (48, 16, 12), 4),
    (2, 64, 0, 64, (16, 8, 4), 4), (2, 32, 0, 32, (64, 16, 12), 4), (1, 64, 0, 64, (34, 17, 14), 4), (2, 32, 32, 64, (32, 16, 16), 4),
])
@pytest.mark.parametrize("h16", ["bf16", "fp16"])
def test_conv3_ring_kernel_vs_brick_kernel(case, h16, monkeypatch):
    """The persistent LDS-DMA ring kernel (tdx_conv3_ring.hip) against the brick kernel it replaces on the two finest
    levels: the same bf16 products accumulated in fp32 in a different order (8-channel units, taps in pairs, bias first),
    so forward output and data gradient (main term + halo shell, with addends, split over two tensors) agree to fp32
    summation noise after one bf16 rounding (rel-L2 < 5e-4, a few per cent of the elements one ulp apart), the fused
    GroupNorm statistics to 1e-5; and the smallest case against the fp64 oracle.  Run twice to catch copies that outlive
    a launch or arrive late (counted vmcnt waits)."""
    from turbdiff_amd import _lib as L, ops

    B, C1, C2, Co, (X, Y, Z) = case[:5]
    depth = case[5] if len(case) > 5 else 8
    monkeypatch.setenv("TDX_RING_Z4", "2" if depth == 4 else "0")
    d = dev()
    Ci = C1 + C2
    # fp16 (round 6): the same kernels instantiated on the other operand format; one ulp is 2^-11 instead of 2^-8, the
    # agreement bounds below scale with it
    dt, DT = (torch.bfloat16, L.BF16) if h16 == "bf16" else (torch.float16, L.F16)
    ulp = 1.0 if h16 == "bf16" else 0.125
    if h16 == "fp16" and B * X * Y * Z > 200000:
        pytest.skip("fp16 repeats the small and medium cases only")
    g = torch.Generator(device=d).manual_seed(11)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1).to(dt), (rn(B, X, Y, Z, C2).to(dt) if C2 else None)
    w = rn(Co, Ci, 3, 3, 3) * (2.0 / (27 * Ci)) ** 0.5
    bias, gy = rn(Co), rn(B, X, Y, Z, Co).to(dt)
    st = L.stream()
    wf, wb = ops._packed_conv3(w, dt)
    L.ensure_scratch(d)

    def run():
        y = torch.empty(B, X, Y, Z, Co, device=d, dtype=dt)
        stats = torch.empty(B, 8, 2, device=d)
        ws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, Co), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_fwd_gn", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), L.ptr(bias), L.ptr(y), L.ptr(stats), 8, 1e-5, L.ptr(ws),
               B, X, Y, Z, Co, DT, L.CONV_AUTO | L.WS_CLEAN, st)
        assert int(ws.count_nonzero()) == 0
        y2 = torch.empty_like(y)
        L.call("tdx_conv3_fwd", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), None, L.ptr(y2), B, X, Y, Z, Co, DT, L.CONV_AUTO, st)
        gx1, gx2 = torch.empty_like(x1), (torch.empty_like(x2) if C2 else None)
        dws = torch.empty(L.query("tdx_conv3_bwd_data_workspace_bytes", B, X, Y, Z, Ci, DT, 0), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_bwd_data_add", L.ptr(gy), L.ptr(wb), L.ptr(gx1), C1, L.ptr(gx2), C2, L.ptr(x1), L.ptr(x2), B, X, Y, Z, Co,
               DT, L.CONV_AUTO, L.ptr(dws), st)
        gp1, gp2 = torch.empty_like(x1), (torch.empty_like(x2) if C2 else None)
        L.call("tdx_conv3_bwd_data", L.ptr(gy), L.ptr(wb), L.ptr(gp1), C1, L.ptr(gp2), C2, 0, B, X, Y, Z, Co, DT, L.CONV_AUTO,
               L.ptr(dws), st)
        torch.cuda.synchronize()
        return y, stats, y2, gx1, gx2, gp1, gp2

    monkeypatch.setenv("TDX_CONV3_RING", "0")
    brick = run()
    monkeypatch.setenv("TDX_CONV3_RING", "2")
    names = ["y", "stats", "y (no bias, no stats)", "gx1", "gx2", "gx1 (no addend)", "gx2 (no addend)"]
    for rep in range(2):
        ring = run()
        for n, a, b in zip(names, ring, brick):
            if a is None:
                continue
            assert torch.isfinite(a.float()).all(), n
            if n == "stats":
                assert rel_l2(a, b) < 1e-5, (n, case, rep)
            elif n.startswith("gx"):
                # + the halo-shell kernel's read-add-write / bf16 atomic adds on the boundary voxels, whose rounding
                # depends on arrival order (both paths; a large share of the voxels on the small grids)
                assert rel_l2(a.float(), b.float()) < 2e-3 * ulp and (a != b).float().mean() < 0.1, (n, case, rep)
            else:
                assert rel_l2(a.float(), b.float()) < 5e-4 * ulp and (a != b).float().mean() < 0.05, (n, case, rep)
        if rep == 0:
            first = ring
        else:  # run-to-run: the conv kernel itself is deterministic (interior voxels carry no halo-shell atomics)
            assert torch.equal(ring[0], first[0]) and torch.equal(ring[2], first[2])
            assert torch.equal(ring[3][:, 1:-1, 1:-1, 1:-1], first[3][:, 1:-1, 1:-1, 1:-1])
    if X * Y * Z <= 4096:  # the fp64 oracle: replicate-padded conv and its adjoint
        xr = torch.cat([x1] + ([x2] if C2 else []), dim=-1).double().cpu().permute(0, 4, 1, 2, 3).requires_grad_()
        yr = O.conv3_replicate(xr, w.to(dt).double().cpu(), bias.double().cpu())
        yr.backward(gy.double().cpu().permute(0, 4, 1, 2, 3))
        assert rel_l2(ring[0].float().cpu().permute(0, 4, 1, 2, 3), yr) < 4e-3 * ulp
        gx = torch.cat([ring[5]] + ([ring[6]] if C2 else []), dim=-1).float().cpu()
        assert rel_l2(gx.permute(0, 4, 1, 2, 3), xr.grad) < 6e-3 * ulp
    # the switch does select the kernel: with one workgroup per CU the ring launch leaves the brick path's timing,
    # not its results; check the dispatcher's own report instead
    assert bool(L.query("tdx_conv3_uses_ring", C1, C2, Co, B, X, Y, Z))
    assert L.query("tdx_conv3_ring_brick_depth", C1, C2, Co, B, X, Y, Z) == depth
    if depth == 4:
        assert L.query("tdx_conv3_ring_brick_depth", Co, 0, Ci, B, X, Y, Z) == depth  # the data gradient's launch


@pytest.mark.gpu
@pytest.mark.parametrize("cus", [224, 240, 64, 8])
@pytest.mark.parametrize("case", [(3, 64, 0, 64, (64, 32, 32)), (2, 32, 32, 32, (64, 64, 32)), (2, 128, 0, 256, (32, 16, 24))])
def test_persistent_kernels_on_fewer_cus(case, cus, monkeypatch):
    """TDX_PERSISTENT_CUS: the persistent one-workgroup-per-CU kernels (ring conv forward / data
    gradient, producer / consumer weight gradient) launched on 224 / 240 / 64 / 8 workgroups instead of 256, so that a
    data-parallel run can leave CUs to RCCL.  A brick's arithmetic does not depend on which workgroup walks it: forward
    output and the data gradient's interior are BIT-identical to the 256-workgroup launch; GroupNorm statistics (f64
    atomics in another order) and the weight gradient (another K split) agree to rounding."""
    from turbdiff_amd import _lib as L, ops

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    dt, DT = torch.bfloat16, L.BF16
    g = torch.Generator(device=d).manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1).to(dt), (rn(B, X, Y, Z, C2).to(dt) if C2 else None)
    w = rn(Co, Ci, 3, 3, 3) * (2.0 / (27 * Ci)) ** 0.5
    bias, gy = rn(Co), rn(B, X, Y, Z, Co).to(dt)
    st = L.stream()
    wf, wb = ops._packed_conv3(w, dt)
    L.ensure_scratch(d)
    monkeypatch.setenv("TDX_CONV3_RING", "2")

    def run():
        y = torch.empty(B, X, Y, Z, Co, device=d, dtype=dt)
        stats = torch.empty(B, 8, 2, device=d)
        ws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, Co), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_fwd_gn", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), L.ptr(bias), L.ptr(y), L.ptr(stats), 8, 1e-5, L.ptr(ws),
               B, X, Y, Z, Co, DT, L.CONV_AUTO | L.WS_CLEAN, st)
        gx1, gx2 = torch.empty_like(x1), (torch.empty_like(x2) if C2 else None)
        dws = torch.empty(L.query("tdx_conv3_bwd_data_workspace_bytes", B, X, Y, Z, Ci, DT, 0), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_bwd_data", L.ptr(gy), L.ptr(wb), L.ptr(gx1), C1, L.ptr(gx2), C2, 0, B, X, Y, Z, Co, DT, L.CONV_AUTO,
               L.ptr(dws), st)
        dw, db = torch.empty(Co, Ci, 3, 3, 3, device=d), torch.empty(Co, device=d)
        wws = torch.zeros(L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, 0), dtype=torch.uint8, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(gy), L.ptr(dw), L.ptr(db), B, X, Y, Z, Co, DT,
               L.CONV_AUTO | L.WS_CLEAN, L.ptr(wws), st)
        torch.cuda.synchronize()
        # TDX_WS_CLEAN covers the accumulators at the head of the weight-gradient workspace (the slabs behind are scratch)
        assert int(wws[: (27 * Ci * Co + Co) * 4].count_nonzero()) == 0 and int(ws.count_nonzero()) == 0
        return y, stats, gx1, gx2, dw, db

    full = run()
    monkeypatch.setenv("TDX_PERSISTENT_CUS", str(cus))
    ntn = Co // 64 if Co % 64 == 0 else Co // 32
    assert bool(L.query("tdx_conv3_uses_ring", C1, C2, Co, B, X, Y, Z)) == (ntn <= cus // 8)
    few = run()
    assert rel_l2(few[1], full[1]) < 1e-5 and rel_l2(few[2].float(), full[2].float()) < 2e-3
    if ntn <= cus // 8:
        inner = lambda t: t[:, 1:-1, 1:-1, 1:-1]
        assert torch.equal(few[0], full[0]) and torch.equal(inner(few[2]), inner(full[2]))
        if C2:
            assert torch.equal(inner(few[3]), inner(full[3]))
    else:  # more N tiles than an XCD has workgroups left: the call falls back to the brick kernel
        assert rel_l2(few[0].float(), full[0].float()) < 5e-4
    assert rel_l2(few[4], full[4]) < 1e-5 and rel_l2(few[5], full[5]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("B,V,C1,C2,Co", [(2, 1000, 64, 0, 128), (3, 777, 64, 64, 32), (1, 256, 32, 0, 32), (6, 4097, 128, 128, 64),
                                          (4, 100, 64, 0, 64), (7, 40, 32, 32, 32)])  # several samples inside one 256-row tile
def test_conv1_fused_with_groupnorm_tail(B, V, C1, C2, Co):
    """tdx_conv1_fwd_gn -- y = silu(GN(h)) + bias + [x1|x2] @ w, the tail of a ResnetBlock with a projected skip
    (reference ddpm.py:176,188,197) in one pass -- against the two calls it replaces (tdx_conv1_fwd into a temporary,
    tdx_gn_apply with that residual): same arithmetic, so equal up to the last bf16 bit of a few elements (fp32
    contraction of the coefficient), and against a float64 evaluation of the formula.  Rows not a multiple of the
    256-row tile, sample boundaries inside a tile, one / two inputs, 32- and 64-wide channel tiles."""
    from turbdiff_amd import _lib as L

    d = dev()
    g = torch.Generator(device=d).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    dt, DT, G = torch.bfloat16, L.BF16, 8
    x1, x2 = rn(B, V, C1).to(dt), (rn(B, V, C2).to(dt) if C2 else None)
    w, bias = rn(C1 + C2, Co) * (C1 + C2) ** -0.5, rn(Co)
    h = (rn(B, V, Co) * 1.7 + 0.3).to(dt)
    gamma, beta = rn(Co) * 0.5 + 1.0, rn(Co) * 0.2
    hf = h.float().view(B, V, G, Co // G)
    mean = hf.mean(dim=(1, 3))
    rstd = (hf.var(dim=(1, 3), unbiased=False) + 1e-5).rsqrt()
    stats = torch.stack((mean, rstd), dim=-1).contiguous()
    st = L.stream()
    y = torch.empty(B, V, Co, device=d, dtype=dt)
    L.call("tdx_conv1_fwd_gn", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(w), Co, L.ptr(bias), L.ptr(h), L.ptr(stats), L.ptr(gamma),
           L.ptr(beta), G, L.ptr(y), B, V, Co, DT, st)
    res, y2 = torch.empty_like(y), torch.empty_like(y)
    L.call("tdx_conv1_fwd", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(w), Co, L.ptr(bias), None, L.ptr(res), B * V, Co, DT, st)
    L.call("tdx_gn_apply", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), None, None, L.ptr(res), L.ptr(y2), B, V, Co, G, 1, DT, st)
    torch.cuda.synchronize()
    assert rel_l2(y.float(), y2.float()) < 1e-3 and (y != y2).float().mean() < 0.01
    xr = torch.cat([x1] + ([x2] if C2 else []), dim=-1).double()
    n = (h.double().view(B, V, G, -1) - mean.double()[:, None, :, None]) * rstd.double()[:, None, :, None]
    n = n.view(B, V, Co) * gamma.double() + beta.double()
    ref = n * torch.sigmoid(n) + (xr @ w.to(dt).double() + bias.double()).to(dt).double()
    assert rel_l2(y.float(), ref.float()) < 6e-3
    # fp32 tensors: not this kernel's (the caller runs the two launches)
    assert L.load().tdx_conv1_fwd_gn(L.ptr(x1), C1, None, 0, L.ptr(w), Co, None, L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                                     G, L.ptr(y), B, V, Co, L.F32, st) == -3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 64, 0, 64, (32, 32, 32)), (2, 32, 0, 32, (48, 32, 16)), (1, 64, 64, 32, (32, 32, 16)),
                                  (3, 16, 0, 64, (32, 16, 16))])
def test_conv3_weight_gradient_is_run_to_run_reproducible(case, monkeypatch):
    """Round 4: the fine levels' weight gradients (K split over 32-512 workgroups) store per-split slabs that
    conv3_unpack_sum_kernel adds in slab order, instead of merging by fp32 atomics in arrival order: the weight gradient
    of the ring and brick kernels is bit-identical from run to run (the bias gradient still merges by atomics), equal to
    the oracle's fp64 weight gradient at bf16-operand accuracy (the atomic route it replaced and its switch are gone), and
    the accumulator part of the workspace stays all-zero (TDX_WS_CLEAN)."""
    from turbdiff_amd import _lib as L

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    g = torch.Generator(device=d).manual_seed(9)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1).bfloat16(), (rn(B, X, Y, Z, C2).bfloat16() if C2 else None)
    gy = rn(B, X, Y, Z, Co).bfloat16()
    st = L.stream()
    L.ensure_scratch(d)
    wws = torch.zeros(L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, 0), dtype=torch.uint8, device=d)

    def run():
        dw, db = torch.empty(Co, Ci, 3, 3, 3, device=d), torch.empty(Co, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(gy), L.ptr(dw), L.ptr(db), B, X, Y, Z, Co, L.BF16,
               L.CONV_AUTO | L.WS_CLEAN, L.ptr(wws), st)
        torch.cuda.synchronize()
        assert int(wws[: (27 * Ci * Co + Co) * 4].count_nonzero()) == 0
        return dw, db

    runs = [run() for _ in range(4)]
    for dw, db in runs[1:]:
        assert torch.equal(dw, runs[0][0])
        assert rel_l2(db, runs[0][1]) < 1e-5
    # ... and equal to the fp64 weight gradient of the oracle's conv at bf16-operand accuracy
    xr = torch.cat([t for t in (x1, x2) if t is not None], dim=-1).double().permute(0, 4, 1, 2, 3).cpu()
    wr = torch.zeros(Co, Ci, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    O.conv3_replicate(xr, wr).backward(gy.double().permute(0, 4, 1, 2, 3).cpu())
    assert rel_l2(runs[0][0].cpu().double(), wr.grad) < 2e-5  # (exact bf16 products, fp32 accumulation)


@pytest.mark.gpu
def test_scratch_arena_is_per_stream():
    """The library holds one arena pointer, bound per launch to the launching stream's arena (_lib.ensure_scratch): convs
    that use it (K-split slabs of the small-grid kernel) run concurrently on two streams, many times over, with different
    operands and must each reproduce their single-stream result; the two streams own different arenas; a GraphSampler's
    graph is captured on a stream of its own (tests/test_hip_model.py::test_graph_sampler_equals_eager_loop replays it
    next to eager steps)."""
    from turbdiff_amd import _lib as L, ops

    d = dev()
    B, C, X, Y, Z = 6, 512, 12, 4, 3
    g = torch.Generator(device=d).manual_seed(21)
    xs = [torch.randn(B, X, Y, Z, C, device=d, generator=g).bfloat16() for _ in range(2)]
    ws = [torch.randn(C, C, 3, 3, 3, device=d, generator=g) * 0.02 for _ in range(2)]
    packed = [ops._packed_conv3(w, torch.bfloat16)[0] for w in ws]

    def conv(i, y):
        L.call("tdx_conv3_fwd", L.ptr(xs[i]), C, None, 0, L.ptr(packed[i]), None, L.ptr(y), B, X, Y, Z, C, L.BF16, L.CONV_AUTO,
               L.stream())

    refs = []
    for i in range(2):
        y = torch.empty(B, X, Y, Z, C, device=d, dtype=torch.bfloat16)
        conv(i, y)
        refs.append(y)
    torch.cuda.synchronize()
    # torch hands out stream handles from a pool of 32 per device: late in a long session a "new" Stream() can BE the block
    # backward's weight-gradient side stream, which is declared zero-block-only (a 4-KiB arena: the small-grid kernel then does
    # not apply and the brick kernel's different summation order fails the bit comparison -- seen once in eleven full-suite
    # runs).  Take streams that own full arenas.
    streams = []
    while len(streams) < 2:
        st = torch.cuda.Stream()
        if (d.index, st.cuda_stream) not in L._SMALL_STREAMS and all(st.cuda_stream != o.cuda_stream for o in streams):
            streams.append(st)
    outs = [[torch.empty_like(refs[0]) for _ in range(20)] for _ in range(2)]
    arenas = []
    for k in range(20):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                conv(i, outs[i][k])
                if k == 0:
                    arenas.append(L.scratch_arena(d).data_ptr())
    torch.cuda.synchronize()
    assert arenas[0] != arenas[1] and L.scratch_arena(d).data_ptr() not in arenas
    for i in range(2):
        for k in range(20):
            assert torch.equal(outs[i][k], refs[i]), (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,chans", [(6, 32, (64, 64, 128, 256, 512, 512, 32)), (1, 96, (8,)), (19, 64, (40, 24, 512)),
                                       (3, 32, tuple([16] * 37)),
                                       (200, 32, (64, 32)),    # 85 KiB of LDS in the backward: above the default 48 KiB cap
                                       (600, 32, (64, 32))])   # beyond the kernels' 160 KiB: per-block torch projection
def test_film_projections_match_linear(B, T, chans):
    """tdx_film_fwd / tdx_film_bwd (all ResnetBlocks' nn.Linear(c_dim, 2 C) + chunk in one launch, reference
    ddpm.py:184,191-192) against F.linear in fp64: outputs, and the gradients of c, every weight and every bias; more
    layers than one table holds; a layer whose output is unused gets zero gradients."""
    from turbdiff_amd import ops

    d = dev()
    torch.manual_seed(3)
    lins = [torch.nn.Linear(T, 2 * C).to(d) for C in chans]
    c = torch.randn(B, T, device=d, requires_grad=True)
    films = ops.film_projections(c, lins)
    cr = c.detach().double().cpu().requires_grad_()
    refs = [torch.nn.functional.linear(cr, l.weight.detach().double().cpu(), l.bias.detach().double().cpu()) for l in lins]
    wr = [(l.weight.detach().double().cpu().requires_grad_(), l.bias.detach().double().cpu().requires_grad_()) for l in lins]
    refs = [torch.nn.functional.linear(cr, w, b) for w, b in wr]
    loss, loss_r = 0.0, 0.0
    skip = len(chans) - 1 if len(chans) > 2 else None  # this layer's result does not reach the loss
    for i, (f, r, C) in enumerate(zip(films, refs, chans)):
        assert f.shape == (2, B, C) and f.dtype == torch.float32 and f.is_contiguous()
        rr = torch.stack((r[:, :C], r[:, C:]))
        assert rel_l2(f.detach().cpu(), rr.detach()) < 1e-6
        if i == skip:
            continue
        m = torch.randn(2, B, C, generator=torch.Generator().manual_seed(i)).double()
        loss = loss + (f * m.float().to(d)).sum()
        loss_r = loss_r + (rr * m).sum()
    loss.backward()
    loss_r.backward()
    assert rel_l2(c.grad.cpu(), cr.grad) < 1e-5
    for i, (l, (w, b)) in enumerate(zip(lins, wr)):
        if i == skip:
            assert float(l.weight.grad.abs().max()) == 0.0 and float(l.bias.grad.abs().max()) == 0.0
            continue
        assert rel_l2(l.weight.grad.cpu(), w.grad) < 1e-5 and rel_l2(l.bias.grad.cpu(), b.grad) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f32s", "f32"])
def test_prefetch_weights_equals_one_by_one(mode):
    """ops.prefetch_weights (tdx_conv3_pack_weights + tdx_transpose_many: all weights of a model in one launch each)
    leaves exactly the cache entries _packed_conv3 / _conv1_wt build one by one -- bit for bit, for the MFMA layouts,
    the shapes that fall back to the plain pack kernel, and more weights than one launch table holds."""
    from turbdiff_amd import _lib as L, ops

    d = dev()
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    prev = L._conv_impl_override
    L.set_conv_impl("split" if mode == "f32s" else None)
    try:
        g = torch.Generator(device=d).manual_seed(11)
        shapes = [(64, 64), (32, 128), (512, 256), (16, 48), (24, 8), (4, 64)] + [(32, 32)] * 35
        w3 = [torch.randn(co, ci, 3, 3, 3, device=d, generator=g) for co, ci in shapes]
        w1 = [torch.randn(co, ci, 1, 1, 1, device=d, generator=g) for co, ci in [(64, 32), (96, 40), (7, 33), (512, 1024)]]
        ref3 = [tuple(t.clone() for t in ops._packed_conv3(w, dt)) for w in w3]
        ref1 = [ops._conv1_wt(w).clone() for w in w1]
        ops._pack_cache.clear()
        ops.prefetch_weights(w3, w1, dt)
        for w, (rf, rb) in zip(w3, ref3):
            hit = ops._pack_cache[(id(w), dt, L.pack_code(dt))]
            assert torch.equal(hit[3].view(torch.uint8), rf.view(torch.uint8)) and torch.equal(hit[4].view(torch.uint8), rb.view(torch.uint8))
            got = ops._packed_conv3(w, dt)
            assert got[0] is hit[3] and got[1] is hit[4]  # the later per-layer call is a cache hit
        for w, r in zip(w1, ref1):
            assert torch.equal(ops._conv1_wt(w), r)
        with torch.no_grad():  # an in-place update makes that entry stale: it alone is packed again
            w3[1].add_(1.0)
        ops.prefetch_weights(w3, w1, dt)
        assert torch.equal(ops._packed_conv3(w3[1], dt)[0].view(torch.uint8), _fresh_pack(w3[1], dt)[0].view(torch.uint8))
    finally:
        L.set_conv_impl(prev)
        ops._pack_cache.clear()


def _fresh_pack(w, dt):
    from turbdiff_amd import _lib as L

    Cout, Cin = w.shape[:2]
    wf = torch.empty(27 * Cin * Cout, dtype=dt, device=w.device)
    wb = torch.empty_like(wf)
    L.call("tdx_conv3_pack_weight", L.ptr(w.detach().contiguous()), L.ptr(wf), L.ptr(wb), Cin, Cout, L.pack_code(dt), L.stream())
    return wf, wb


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("C1,C2,Cout", [(64, 0, 128), (256, 256, 128), (32, 0, 4), (40, 24, 72), (1024, 0, 256)])
def test_conv1_weight_gradient_in_parameter_layout(dt, C1, C2, Cout):
    """tdx_conv1_bwd_weight_oc: dW stored as (Cout, Cin) -- the parameter's own layout -- and the bias gradient, against
    the fp64 sums and against tdx_conv1_bwd_weight's [Cin][Cout] result; two-input form writes column blocks."""
    from turbdiff_amd import _lib as L, ops

    d = dev()
    g = torch.Generator(device=d).manual_seed(5)
    rows = 6 * 11 * 7 * 5
    x1 = torch.randn(rows, C1, device=d, generator=g).to(dt)
    x2 = torch.randn(rows, C2, device=d, generator=g).to(dt) if C2 else None
    gy = torch.randn(rows, Cout, device=d, generator=g).to(dt)
    gw, gb = ops._conv1_weight_grad(x1, C1, x2, C2, gy, Cout, True, rows, L.dtype_code(dt), L.stream())
    x = torch.cat([x1] + ([x2] if C2 else []), dim=1).double().cpu()
    ref = gy.double().cpu().t() @ x
    tol = 1e-5 if dt == torch.float32 else 1e-5  # fp32 accumulation of exact products either way
    assert gw.shape == (Cout, C1 + C2) and gw.is_contiguous()
    assert rel_l2(gw.cpu(), ref) < tol and rel_l2(gb.cpu(), gy.double().cpu().sum(0)) < tol
    old = torch.empty(C1, Cout, device=d)
    L.call("tdx_conv1_bwd_weight", L.ptr(x1), C1, L.ptr(gy), Cout, L.ptr(old), Cout, None, rows, L.dtype_code(dt), L.stream())
    assert rel_l2(gw[:, :C1].t().cpu(), old.cpu()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    # B, C1, C2, Cout, grid: 64-wide output tiles; whole and ragged bricks (zero rows from the arena's zero block), two
    # inputs, a half-filled last ci tile (C1 = 16), several co tiles, few and many bricks per workgroup, level-0 size
    (2, 64, 0, 64, (32, 32, 16)), (1, 32, 32, 64, (48, 32, 24)), (2, 16, 0, 64, (32, 16, 16)), (1, 64, 0, 128, (20, 18, 13)),
    (3, 32, 0, 64, (9, 17, 10)), (1, 64, 0, 64, (96, 32, 24)), (2, 64, 0, 64, (192, 64, 48)), (6, 128, 0, 256, (48, 16, 12)),
    # 32-wide output tiles (round 5): level-0 size, four ci tiles, ragged bricks + two inputs + three co tiles, half-filled ci tile
    (2, 32, 0, 32, (192, 64, 48)), (1, 128, 0, 32, (96, 32, 24)), (3, 32, 32, 96, (50, 33, 20)), (4, 16, 0, 32, (64, 64, 32)),
])
@pytest.mark.parametrize("h16", ["bf16", "fp16"])
def test_conv3_weight_gradient_producer_consumer_kernel_vs_brick_kernel(case, h16, monkeypatch):
    """The producer / consumer weight-gradient kernel (tdx_conv3_wgrad_ring.hip: 8 computing + 4 loader waves) against the
    brick kernel it replaces, 64- and 32-wide output tiles (TDX_WGRAD_RING = 1 / 0): the same per-workgroup partial sums,
    merged by fp32 atomics or slabs in a different order -> 2e-6; the bias gradient comes from an all-ones MFMA slot
    instead of the staging registers; the workspace is left zero; and the fp64 sums on the small cases.  Twice: the
    second call catches stale LDS / late copies."""
    from turbdiff_amd import _lib as L

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    dt, DT = (torch.bfloat16, L.BF16) if h16 == "bf16" else (torch.float16, L.F16)  # fp16 (round 6): the other instantiations
    if h16 == "fp16" and B * X * Y * Z > 200000:
        pytest.skip("fp16 repeats the small and medium cases only")
    g = torch.Generator(device=d).manual_seed(13)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1).to(dt), (rn(B, X, Y, Z, C2).to(dt) if C2 else None)
    gy = rn(B, X, Y, Z, Co).to(dt)
    st = L.stream()
    L.ensure_scratch(d)
    ws = torch.zeros(L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, L.CONV_AUTO), dtype=torch.uint8, device=d)

    def run(ring):
        monkeypatch.setenv("TDX_WGRAD_RING", str(ring))
        monkeypatch.setenv("TDX_WGRAD_SMALL_ROWS", "0")
        dw, db = torch.empty(Co, Ci, 3, 3, 3, device=d), torch.empty(Co, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(gy), L.ptr(dw), L.ptr(db), B, X, Y, Z, Co, DT,
               L.CONV_AUTO | L.WS_CLEAN, L.ptr(ws), st)
        torch.cuda.synchronize()
        assert int(ws[: (27 * Ci * Co + Co) * 4].count_nonzero()) == 0
        return dw, db

    brick = run(0)
    for rep in range(2):
        ring = run(1)
        assert torch.isfinite(ring[0]).all() and torch.isfinite(ring[1]).all()
        assert rel_l2(ring[0], brick[0]) < 2e-6 and rel_l2(ring[1], brick[1]) < 2e-6, (case, rep)
    if B * X * Y * Z <= 20000 or Co == 96:
        xr = torch.cat([x1] + ([x2] if C2 else []), dim=-1).double().cpu().permute(0, 4, 1, 2, 3)
        w = torch.zeros(Co, Ci, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        bz = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
        O.conv3_replicate(xr, w, bz).backward(gy.double().cpu().permute(0, 4, 1, 2, 3))
        assert rel_l2(ring[0].cpu(), w.grad) < 1e-5 and rel_l2(ring[1].cpu(), bz.grad) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    # B, C1, C2, Cout, grid: level-0 size; several ci and co tiles; ragged bricks, two inputs; a half-filled ci tile (C1 = 16);
    # too few bricks per workgroup (the call stays on the single-role kernel: both runs are that kernel)
    (2, 32, 0, 32, (96, 64, 48)), (1, 128, 0, 64, (96, 32, 24)), (3, 32, 32, 96, (50, 33, 20)), (4, 16, 0, 32, (64, 64, 32)),
    (1, 64, 0, 64, (20, 18, 13)),
])
def test_conv3_split_weight_gradient_producer_consumer_kernel(case, monkeypatch):
    """The producer / consumer split-precision weight gradient (tdx_conv3_wgrad_split_ring.hip: 2 x 8 x 8 bricks, loader waves
    split fp32 -> bf16 hi + lo) against the single-role kernel (TDX_WGRAD_SPLIT_RING = 1 / 0; other brick shape and K split,
    so other partial sums: 1e-5) and against the fp64 sums (three bf16 products per fp32 product: 3e-5); the bias gradient comes
    from ones x (dy_hi + dy_lo) instead of the fp32 registers.  On 8 workgroups (TDX_PERSISTENT_CUS) as well; twice: the second
    call catches stale LDS."""
    from turbdiff_amd import _lib as L

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    g = torch.Generator(device=d).manual_seed(17)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1), (rn(B, X, Y, Z, C2) if C2 else None)
    gy = rn(B, X, Y, Z, Co)
    st = L.stream()
    L.ensure_scratch(d)
    ws = torch.zeros(L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, L.CONV_SPLIT), dtype=torch.uint8, device=d)

    def run(ring, cus=None):
        monkeypatch.setenv("TDX_WGRAD_SPLIT_RING", str(ring))
        if cus is None:
            monkeypatch.delenv("TDX_PERSISTENT_CUS", raising=False)
        else:
            monkeypatch.setenv("TDX_PERSISTENT_CUS", str(cus))
        dw, db = torch.empty(Co, Ci, 3, 3, 3, device=d), torch.empty(Co, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(gy), L.ptr(dw), L.ptr(db), B, X, Y, Z, Co, L.F32,
               L.CONV_SPLIT | L.WS_CLEAN, L.ptr(ws), st)
        torch.cuda.synchronize()
        assert int(ws[: (27 * Ci * Co + Co) * 4].count_nonzero()) == 0
        return dw, db

    single = run(0)
    for rep, cus in enumerate((None, None, 8)):
        ring = run(1, cus)
        assert torch.isfinite(ring[0]).all() and torch.isfinite(ring[1]).all()
        assert rel_l2(ring[0], single[0]) < 1e-5 and rel_l2(ring[1], single[1]) < 1e-5, (case, rep)
    if B * X * Y * Z <= 100000:
        xr = torch.cat([x1] + ([x2] if C2 else []), dim=-1).double().cpu().permute(0, 4, 1, 2, 3)
        w = torch.zeros(Co, Ci, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        bz = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
        O.conv3_replicate(xr, w, bz).backward(gy.double().cpu().permute(0, 4, 1, 2, 3))
        assert rel_l2(ring[0].cpu(), w.grad) < 3e-5 and rel_l2(ring[1].cpu(), bz.grad) < 3e-5


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    # B, C1, C2, Cout, grid -- the deep levels of the shipped model and ragged / tiny relatives
    (6, 512, 0, 512, (12, 4, 3)), (6, 256, 0, 512, (24, 8, 6)), (6, 512, 512, 256, (24, 8, 6)), (6, 256, 0, 256, (24, 8, 6)),
    (2, 128, 0, 32, (5, 3, 1)), (3, 256, 0, 96, (7, 9, 4)), (8, 512, 0, 512, (12, 4, 3)), (1, 160, 0, 64, (13, 7, 6)),
    (5, 128, 128, 64, (3, 17, 15)),
])
def test_conv3_weight_gradient_small_grid_kernel_vs_brick_kernel(case, monkeypatch):
    """The packed-K weight-gradient kernel of the deep levels (tdx_conv3_wgrad_small.hip) against the brick kernel it
    replaces there (row gate closed vs open) and against the fp64 sums on the smallest cases: weight and bias gradient,
    slab and atomic merges, two inputs, ragged last slab / last sample group, K rows that are not a multiple of 16; the
    workspace is left zero both ways."""
    from turbdiff_amd import _lib as L

    B, C1, C2, Co, (X, Y, Z) = case
    d = dev()
    Ci = C1 + C2
    g = torch.Generator(device=d).manual_seed(9)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    x1, x2 = rn(B, X, Y, Z, C1).bfloat16(), (rn(B, X, Y, Z, C2).bfloat16() if C2 else None)
    gy = rn(B, X, Y, Z, Co).bfloat16()
    st = L.stream()
    ws = torch.zeros(L.query("tdx_conv3_bwd_weight_workspace_bytes", Ci, Co, L.CONV_AUTO), dtype=torch.uint8, device=d)

    def run(rows):
        monkeypatch.setenv("TDX_WGRAD_SMALL_ROWS", str(rows))
        dw, db = torch.empty(Co, Ci, 3, 3, 3, device=d), torch.empty(Co, device=d)
        L.call("tdx_conv3_bwd_weight", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(gy), L.ptr(dw), L.ptr(db), B, X, Y, Z, Co, L.BF16,
               L.CONV_AUTO | L.WS_CLEAN, L.ptr(ws), st)
        torch.cuda.synchronize()
        assert int(ws[: (27 * Ci * Co + Co) * 4].count_nonzero()) == 0
        return dw, db

    small, brick = run(1 << 30), run(0)
    assert torch.isfinite(small[0]).all() and torch.isfinite(small[1]).all()
    assert rel_l2(small[0], brick[0]) < 2e-6 and rel_l2(small[1], brick[1]) < 2e-6
    if B * X * Y * Z <= 1000:
        xr = torch.cat([x1] + ([x2] if C2 else []), dim=-1).double().cpu().permute(0, 4, 1, 2, 3)
        w = torch.zeros(Co, Ci, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        bz = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
        O.conv3_replicate(xr, w, bz).backward(gy.double().cpu().permute(0, 4, 1, 2, 3))
        assert rel_l2(small[0].cpu(), w.grad) < 1e-5 and rel_l2(small[1].cpu(), bz.grad) < 1e-5
