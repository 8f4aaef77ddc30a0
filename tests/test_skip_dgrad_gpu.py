"""tdx_conv3_bwd_data_skip on the GPU: the input gradient of a ResnetBlock with a projected (1x1) skip, produced by the ring
kernel's main-term launch in one pass (csrc/tdx_conv3_ring.hip, SK = 2), against the float64 reference and the derived
element-wise bounds of tests/skip_dgrad_reference.py (derivation: that module's docstring; inputs on a grid that is exact in
bf16 and fp16, so the fp32 accumulation is exact and only the roundings to the storage format remain).

TDX_CONV3_RING=2 is set per call: the ring kernel is then legal at these small grids.  Every case asserts through
tdx_conv3_bwd_data_skip_supported which route serves it; none is skipped where the library loads.

  * the four fused shapes: |fused - ref| <= the fused bound at EVERY element (one storage rounding at an interior voxel, one
    more per shell fold on the faces), and the fused bound is below the two-launch bound at every interior element;
  * shapes the variant does not serve (a ragged grid, Cout = 64, float32): the query answers 0, the fused entry refuses with
    TDX_ESHAPE, the old route meets ITS bound, and ops.resnet_block's backward launches the old sequence;
  * TDX_SKIP_DGRAD_FUSE=0: query 0, the entry refuses, and the block backward is the two-launch sequence again;
  * TDX_DETERMINISTIC=1: two runs of the fused call are bit-equal;
  * ops.resnet_block with a projected skip on 16x16x8: gx within the bounds of the switch-off run's, every other gradient
    bit for bit the switch-off run's.
"""

import contextlib
import functools
import os

import pytest
import torch

import skip_dgrad_reference as S

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# (B, grid, C1, C2, Cout, dtype)
FUSED = [
    (2, (16, 16, 8), 32, 32, 32, "bf16"),  # split at D1 inside one N tile, several bricks per sample, all six faces
    (1, (8, 8, 16), 64, 64, 32, "bf16"),   # two N tiles: n0 != 0 in the wr fill, the N tiles of a brick on neighbouring workgroups
    (1, (8, 16, 8), 64, 0, 32, "bf16"),    # single input, d2 == NULL
    (2, (16, 8, 8), 32, 32, 32, "f16"),    # the fp16 instantiation
]
OLD = [
    (1, (17, 8, 8), 32, 32, 32, "bf16"),   # a remainder slab along x
    (1, (16, 8, 8), 32, 32, 64, "bf16"),   # K = 64
    (1, (16, 8, 8), 32, 32, 32, "f32"),
]


def _id(c):
    B, grid, C1, C2, Cout, dn = c
    return f"{B}x" + "x".join(map(str, grid)) + f"-{C1}+{C2}-{Cout}-{dn}"


@contextlib.contextmanager
def env(**kv):
    kv = {"TDX_CONV3_RING": "2", **kv}
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def lib():
    from turbdiff_amd import _lib as L

    return L


@functools.lru_cache(maxsize=None)
def _case(c):
    """(inputs, reference, device operands) of one case: computed once, shared, never written to"""
    B, grid, C1, C2, Cout, dn = c
    L, d, dt = lib(), torch.device("cuda:0"), DT[dn]
    p = S.exact_inputs(B, grid, C1, C2, Cout, seed=len(_id(c)))
    r = S.reference(p)
    S.assert_exact(p, r)
    Cin, code = C1 + C2, L.dtype_code(dt)
    w = p["w1"].to(d)
    wf, wb = (torch.empty(27 * Cin * Cout, dtype=dt, device=d) for _ in range(2))
    L.call("tdx_conv3_pack_weight", L.ptr(w), L.ptr(wf), L.ptr(wb), Cin, Cout, L.pack_code(dt), L.stream())
    torch.cuda.synchronize()
    return p, r, dict(dh1=p["dh1"].to(d).to(dt), gy=p["gy"].to(d).to(dt), wb=wb, wr=p["wr"].to(d).contiguous())


def _supported(c, L):
    B, grid, C1, C2, Cout, dn = c
    with L._LAUNCH_LOCK:
        L.ensure_scratch()
        return L.query("tdx_conv3_bwd_data_skip_supported", C1, C2, Cout, B, *grid, L.dtype_code(DT[dn]), L.CONV_AUTO)


def _outputs(c, o):
    B, grid, C1, C2, Cout, dn = c
    d, dt = o["dh1"].device, DT[dn]
    dx1 = torch.full((B, *grid, C1), float("nan"), dtype=dt, device=d)
    dx2 = torch.full((B, *grid, C2), float("nan"), dtype=dt, device=d) if C2 else None
    L = lib()
    ws = torch.empty(L.query("tdx_conv3_bwd_data_workspace_bytes", B, *grid, C1 + C2, L.dtype_code(dt), L.CONV_AUTO), dtype=torch.uint8,
                     device=d)
    return dx1, dx2, ws


def _cat(dx1, dx2):
    torch.cuda.synchronize()
    return (dx1 if dx2 is None else torch.cat((dx1, dx2), dim=-1)).double().cpu()


def fused(c, o):
    B, grid, C1, C2, Cout, dn = c
    L = lib()
    dx1, dx2, ws = _outputs(c, o)
    L.call("tdx_conv3_bwd_data_skip", L.ptr(o["dh1"]), L.ptr(o["wb"]), L.ptr(dx1), C1, L.ptr(dx2), C2, L.ptr(o["gy"]), L.ptr(o["wr"]),
           B, *grid, Cout, L.dtype_code(DT[dn]), L.CONV_AUTO, L.ptr(ws), L.stream())
    return _cat(dx1, dx2)


def two_launch(c, o):
    """tdx_conv3_bwd_data, then gy @ wr[:, block] with the adjoint as the 1x1 kernel's addend, per input tensor"""
    B, grid, C1, C2, Cout, dn = c
    L = lib()
    code, st, rows = L.dtype_code(DT[dn]), L.stream(), B * grid[0] * grid[1] * grid[2]
    t1, t2, ws = _outputs(c, o)
    L.call("tdx_conv3_bwd_data", L.ptr(o["dh1"]), L.ptr(o["wb"]), L.ptr(t1), C1, L.ptr(t2), C2, 0, B, *grid, Cout, code, L.CONV_AUTO,
           L.ptr(ws), st)
    out = []
    for t, col, C in ((t1, 0, C1), (t2, C1, C2)):
        if t is None:
            out.append(None)
            continue
        y = torch.empty_like(t)
        L.call("tdx_conv1_fwd", L.ptr(o["gy"]), Cout, None, 0, L.ptr(o["wr"]) + 4 * col, C1 + C2, None, L.ptr(t), L.ptr(y), rows, C, code, st)
        out.append(y)
    return _cat(*out)


def _worst(err, bound):
    q = err / bound.clamp_min(1e-300)
    return f"max |err| {err.max().item():.3e}, max err / bound {q.max().item():.3f}, elements over: {int((err > bound).sum())} of {err.numel()}"


@pytest.mark.parametrize("c", FUSED, ids=_id)
def test_fused_meets_the_one_rounding_bound(c):
    L = lib()
    p, r, o = _case(c)
    b_fused, b_two = S.bounds(r, DT[c[5]])
    with env():
        assert _supported(c, L) == 1
        got = fused(c, o)
    err = (got - r["ref"]).abs()
    print(_id(c), "fused:", _worst(err, b_fused))
    assert torch.isfinite(got).all()
    assert bool((err <= b_fused).all()), _worst(err, b_fused)
    inner = S.interior(c[1])[None, :, :, :, None].expand_as(err)
    assert bool((b_fused[inner] < b_two[inner]).all())  # one storage rounding against three: the tighter bound is the fused one


@pytest.mark.parametrize("c", OLD, ids=_id)
def test_unserved_shapes_refuse_and_stay_on_the_old_route(c):
    L = lib()
    p, r, o = _case(c)
    _, b_two = S.bounds(r, DT[c[5]])
    with env():
        assert _supported(c, L) == 0
        with pytest.raises(RuntimeError, match="TDX_ESHAPE"):
            fused(c, o)
        got = two_launch(c, o)
        names = _block_backward_calls(c)
    err = (got - r["ref"]).abs()
    print(_id(c), "two launches:", _worst(err, b_two))
    assert bool((err <= b_two).all()), _worst(err, b_two)
    assert "tdx_conv3_bwd_data_skip" not in names and names.count("tdx_conv1_fwd") == 2


def test_switch_off_brings_the_two_launch_sequence_back():
    c = FUSED[0]
    L = lib()
    p, r, o = _case(c)
    with env(TDX_SKIP_DGRAD_FUSE="0"):
        assert _supported(c, L) == 0
        with pytest.raises(RuntimeError, match="TDX_ESHAPE"):
            fused(c, o)
        off = _block_backward_calls(c)
    with env():
        on = _block_backward_calls(c)
    assert off.count("tdx_conv1_fwd") == 2 and "tdx_conv3_bwd_data_skip" not in off
    assert on.count("tdx_conv1_fwd") == 0 and on.count("tdx_conv3_bwd_data_skip") == 1
    # the switch removes two launches and renames one; nothing else moves
    assert [n for n in off if n != "tdx_conv1_fwd"] == [n.replace("tdx_conv3_bwd_data_skip", "tdx_conv3_bwd_data") for n in on]


def test_fused_call_is_deterministic():
    c = FUSED[0]
    p, r, o = _case(c)
    with env(TDX_DETERMINISTIC="1"):
        assert _supported(c, lib()) == 1
        a, b = fused(c, o), fused(c, o)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ block level


def _block(c, seed=0):
    """inputs and parameters of one ops.resnet_block call (Gaussian, seeded), on the device"""
    B, grid, C1, C2, Cout, dn = c
    d, dt = torch.device("cuda:0"), DT[dn]
    g = torch.Generator().manual_seed(9000 + seed)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    act = lambda C: rn(B, *grid, C).to(d).to(dt).requires_grad_(True)
    par = lambda *s, scale=1.0, shift=0.0: (rn(*s, scale=scale) + shift).to(d).requires_grad_(True)
    Cin = C1 + C2
    args = dict(x1=act(C1), x2=act(C2) if C2 else None,
                conv1=(par(Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5), par(Cout, scale=0.1)),
                norm1=(par(Cout, scale=0.2, shift=1.0), par(Cout, scale=0.1)),
                conv2=(par(Cout, Cout, 3, 3, 3, scale=(27 * Cout) ** -0.5), par(Cout, scale=0.1)),
                norm2=(par(Cout, scale=0.2, shift=1.0), par(Cout, scale=0.1)),
                skip=(par(Cout, Cin, 1, 1, 1, scale=Cin**-0.5), par(Cout, scale=0.1)), film=par(2, B, Cout, scale=0.3))
    args["gy"] = rn(B, *grid, Cout).to(d).to(dt)
    return args


def _run_block(a, groups=8):
    """(leaves, gradients) of one forward + backward of the block"""
    from turbdiff_amd import ops

    y = ops.resnet_block(a["x1"], a["x2"], None, None, a["conv1"], a["norm1"], a["conv2"], a["norm2"], a["skip"], groups, film=a["film"])
    leaves = [a["x1"]] + ([a["x2"]] if a["x2"] is not None else []) + [t for k in ("conv1", "norm1", "conv2", "norm2", "skip") for t in a[k]]
    leaves.append(a["film"])
    grads = torch.autograd.grad(y, leaves, a["gy"])
    torch.cuda.synchronize()
    return leaves, grads


def _block_backward_calls(c):
    """entry names ops.resnet_block's backward sends to the library, in order"""
    from turbdiff_amd import ops

    L = lib()
    a = _block(c)
    y = ops.resnet_block(a["x1"], a["x2"], None, None, a["conv1"], a["norm1"], a["conv2"], a["norm2"], a["skip"], 8, film=a["film"])
    names, real = [], L.call

    def spy(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)

    L.call = spy
    try:
        y.backward(a["gy"])
        torch.cuda.synchronize()
    finally:
        L.call = real
    return names


def test_block_backward_equals_the_switch_off_run():
    """Every gradient of the block but gx bit for bit (TDX_DETERMINISTIC=1: the parameter gradients' merges are ordered, so
    two runs of one route agree in every bit); gx1 | gx2 within the two routes' bounds of the float64 reference, which is
    computed from the dh1 the backward itself hands to the data gradient and the weights as the kernels read them."""
    from turbdiff_amd import ops

    c = FUSED[0]
    B, grid, C1, C2, Cout, dn = c
    dt = DT[dn]
    a = _block(c, seed=1)
    seen, real = [], ops._conv3_bwd_data

    def capture(gy, *args, **kw):
        if kw.get("skip") is not None:
            seen.append(gy.detach().clone())
        return real(gy, *args, **kw)

    with env(TDX_DETERMINISTIC="1"):
        ops._conv3_bwd_data = capture
        try:
            _, on = _run_block(a)
        finally:
            ops._conv3_bwd_data = real
        with env(TDX_SKIP_DGRAD_FUSE="0"):
            _, off = _run_block(a)
    assert len(seen) == 1, "the fused entry did not serve the block"
    nx = 2 if C2 else 1
    for k, (g_on, g_off) in enumerate(zip(on[nx:], off[nx:])):
        assert torch.equal(g_on, g_off), f"gradient {nx + k} moved"
    q = lambda t: t.detach().to(dt).float().cpu()  # the operands as the kernels read them
    p = dict(dh1=seen[0].float().cpu(), gy=a["gy"].float().cpu(), w1=q(a["conv1"][0]), wr=q(a["skip"][0]).reshape(Cout, C1 + C2))
    r = S.reference(p)
    b_fused, b_two = S.bounds(r, dt)
    gx_on, gx_off = (torch.cat([g.double().cpu() for g in gs[:nx]], dim=-1) for gs in (on, off))
    err = (gx_on - r["ref"]).abs()
    print("block gx, fused:", _worst(err, b_fused))
    assert bool((err <= b_fused).all()), _worst(err, b_fused)
    diff = (gx_on - gx_off).abs()
    assert bool((diff <= b_fused + b_two).all()), _worst(diff, b_fused + b_two)
