"""TF-Net's flow decomposition on the GPU: ops.flow_decompose (csrc/tdx_flow_decompose.hip) against the float64
restatement of tests/flow_decompose_cases.py on the same fp32 inputs, with the torch route (LES.decompose +
_to_nvc_padded + autograd, on the GPU) as the yardstick of how large an error may be; then the LES model and TFNetTrainer
with models.tfnet.FUSE_DECOMPOSE on and off against the reference's float64 fixture (tests/golden/tfnet*.npz).

Bounds.  Kernels, per output and per gradient (dS and dw as vectors of 27 and L entries): f32 err <= max(4 x the torch
route's error, 4e-6), bf16 err <= 2 x the torch route's error -- the factors test_tfnet_gpu.py gives f32 and bf16 kernels,
the floor of its _f32_bound.  Model f32: every stored quantity with the switch on within max(8 x ref32_err, 4e-6).  Model
bf16: err(on) <= 1.5 x err(off) per quantity, a stored gradient norm max(1.5 x err(off), 2^-8).  Every measured pair is
printed (`FLD ...` lines) before it is asserted."""

import functools
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import flow_decompose_cases as FC  # noqa: E402
import tfnet_cases as TC  # noqa: E402
from conftest import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SHIPPED = FC.CONFIGS[0]


def _kernel_cases():
    """Not the full product: every (T, L, F) at the host grid and the multi-tile grid, every grid at the shipped (6, 4, 4);
    B = 1 and 2 both occur at single-tile and at multi-tile grids."""
    cases = []
    for i, cfg in enumerate(FC.CONFIGS):
        cases += [(cfg, FC.HOST_GRID, 1 + i % 2, False), (cfg, FC.MULTI_GRID, 2 - i % 2, False)]
    for i, grid in enumerate(FC.GRIDS):
        cases.append((SHIPPED, grid, 2 - i % 2, False))
    cases.append((SHIPPED, FC.MULTI_GRID, 2, True))  # xx = 100 + 0.1 N(0, 1): prime cancels
    return list(dict.fromkeys(cases))


def _id(case):
    (T, L, Fn), grid, B, cancel = case
    return f"T{T}L{L}F{Fn}-{'x'.join(map(str, grid))}-B{B}" + ("-cancel" if cancel else "")


@functools.lru_cache(maxsize=None)
def _inputs(case, mode):
    """xx, the two filters (module shapes) on the device, the incoming gradients (B, X, Y, Z, Cp) rounded to the storage
    dtype (the padding channels carry noise too: no route may use them), and the float64 results.  Never modified."""
    (T, L, Fn), grid, B, cancel = case
    g = torch.Generator().manual_seed(1000 * T + 100 * L + 10 * Fn + sum(grid) + B)
    n = T - L + 1
    xx = torch.randn(B, T, Fn, *grid, generator=g)
    if cancel:
        xx = 100 + 0.1 * xx
    S = torch.randn(1, 1, 3, 3, 3, generator=g) / 27 ** 0.5
    w = torch.randn(1, L, 1, 1, 1, generator=g) / L ** 0.5
    grads = [torch.randn(B, *grid, FC.up8(n * Fn), generator=g).to(DTYPES[mode]) for _ in range(3)]
    ref = {k: FC.to_nvc(v) for k, v in zip(("bar", "tilde", "prime"), FC.decompose_ref(xx, S.reshape(3, 3, 3), w))}
    gxx, dS, dw = FC.decompose_bwd_ref(xx.numpy(), S.numpy(), w.numpy(), *(FC.from_nvc(t.double(), n, Fn).numpy() for t in grads))
    ref.update(gxx=torch.from_numpy(gxx), dS=torch.from_numpy(dS).reshape(S.shape), dw=torch.from_numpy(dw).reshape(w.shape))
    return SimpleNamespace(xx=xx.to(DEV), S=S.to(DEV), w=w.to(DEV), grads=[t.to(DEV) for t in grads], ref=ref, n=n, L=L)


def _run(route, inp, dtype, xx_grad=True):
    """{bar, tilde, prime, gxx, dS, dw} of one route; the inputs are cloned."""
    xx = inp.xx.clone().requires_grad_(xx_grad)
    S, w = inp.S.clone().requires_grad_(), inp.w.clone().requires_grad_()
    outs = route(xx, S, w, dtype)
    leaves = [xx, S, w] if xx_grad else [S, w]
    g = torch.autograd.grad(outs, leaves, inp.grads)
    out = dict(zip(("bar", "tilde", "prime"), (o.detach() for o in outs)))
    out.update(zip(("gxx", "dS", "dw") if xx_grad else ("dS", "dw"), g))
    return out


def _kernel_route(xx, S, w, dtype):
    from turbdiff_amd import ops

    return ops.flow_decompose(xx, S, w, dtype)


def _torch_route(xx, S, w, dtype):
    """LES.decompose + _to_nvc_padded, what LES.forward does with the switch off."""
    from turbdiff_amd.models.dilresnet import _to_nvc_padded, _up8
    from turbdiff_amd.models.tfnet import LES

    holder = SimpleNamespace(temporal_filtering_length=w.shape[1], spatial_filter=SimpleNamespace(weight=S),
                             temporal_filter=SimpleNamespace(weight=w))
    stacks = LES.decompose(holder, xx)
    return tuple(_to_nvc_padded(u, _up8(u.shape[1]), dtype) for u in stacks)


@pytest.mark.parametrize("case", _kernel_cases(), ids=_id)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_kernels_against_float64(mode, case):
    dtype = DTYPES[mode]
    inp = _inputs(case, mode)
    got, yard = _run(_kernel_route, inp, dtype), _run(_torch_route, inp, dtype)
    failures = []
    for k, r in inp.ref.items():
        assert got[k].shape == yard[k].shape == r.shape and got[k].dtype == yard[k].dtype, k
        e, ey = rel_l2(got[k], r), rel_l2(yard[k], r)
        bound = max(4.0 * ey, 4e-6) if mode == "f32" else 2.0 * ey
        print(f"FLD {mode} {_id(case)} {k}: kernel {e:.3e} torch {ey:.3e} ratio {e / ey if ey > 0 else float('inf') if e > 0 else 0.0:.2f} "
              f"bound {bound:.3e}")
        if not e <= bound:
            failures.append((k, e, ey))
    assert not failures, failures


@pytest.mark.parametrize("cfg", FC.CONFIGS, ids=str)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_zero_channels_are_written_by_the_kernel(mode, cfg):
    from turbdiff_amd import _lib as L

    dtype = DTYPES[mode]
    inp = _inputs((cfg, FC.MULTI_GRID, 2, False), mode)
    T, Ln, Fn = cfg
    cp, real = FC.up8(inp.n * Fn), inp.n * Fn
    outs = [torch.full((2, *FC.MULTI_GRID, cp), 7.0, dtype=dtype, device=DEV) for _ in range(3)]
    L.call("tdx_flow_decompose_fwd", L.ptr(inp.xx), L.ptr(inp.S.reshape(27)), L.ptr(inp.w.reshape(-1)), *(L.ptr(o) for o in outs),
           2, T, Ln, Fn, *FC.MULTI_GRID, L.dtype_code(dtype), L.stream())
    torch.cuda.synchronize()
    with torch.no_grad():
        want = _kernel_route(inp.xx, inp.S, inp.w, dtype)
    for o, ref in zip(outs, want):
        assert torch.all(o[..., real:] == 0) and torch.all(ref[..., real:] == 0)
        assert torch.equal(o, ref) and not torch.any(o[..., :real] == 7.0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_without_a_gradient_to_xx(mode):
    inp = _inputs((SHIPPED, FC.MULTI_GRID, 2, False), mode)
    a, b = _run(_kernel_route, inp, DTYPES[mode]), _run(_kernel_route, inp, DTYPES[mode], xx_grad=False)
    assert "gxx" not in b
    assert torch.equal(a["dS"], b["dS"]) and torch.equal(a["dw"], b["dw"])
    # and the autograd node hands back None for xx: a leaf that asks for nothing gets nothing
    xx = inp.xx.clone()
    S = inp.S.clone().requires_grad_()
    sum(o.float().sum() for o in _kernel_route(xx, S, inp.w, DTYPES[mode])).backward()
    assert xx.grad is None and S.grad is not None


@pytest.mark.parametrize("deterministic", [False, True], ids=["unset", "set"])
def test_two_calls_give_identical_bits(deterministic, monkeypatch):
    if deterministic:
        monkeypatch.setenv("TDX_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("TDX_DETERMINISTIC", raising=False)
    for mode in ("f32", "bf16"):
        inp = _inputs((SHIPPED, FC.MULTI_GRID, 2, False), mode)
        a, b = _run(_kernel_route, inp, DTYPES[mode]), _run(_kernel_route, inp, DTYPES[mode])
        for k in a:
            assert torch.equal(a[k], b[k]), (mode, k)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batch_past_the_launch_y_axis(mode):
    """B = GRID_Y + 3: the last samples lie in the second layer of the launch's z axis, whose other workgroups have no
    sample.  A sample's outputs and gxx do not depend on the batch it is in, so they equal, bit for bit, those of the same
    samples run as two smaller batches; dS and dw against the float64 restatement, held to the f32 floor 4e-6 of the
    kernel tests (f64 sums, one rounding to f32 at the end) -- the torch route is no yardstick here: MIOpen takes
    20 s for a conv over this many volumes."""
    dtype = DTYPES[mode]
    B, T, Ln, Fn, grid = FC.GRID_Y + 3, 2, 2, 1, (1, 2, 17)
    assert FC.supported(B, T, Ln, Fn, grid) and FC.tile_geometry(grid).blocks == 2
    g = torch.Generator().manual_seed(B)
    xx = torch.randn(B, T, Fn, *grid, generator=g)
    S, w = torch.randn(1, 1, 3, 3, 3, generator=g) / 27 ** 0.5, torch.randn(1, Ln, 1, 1, 1, generator=g) / Ln ** 0.5
    grads = [torch.randn(B, *grid, 8, generator=g).to(dtype) for _ in range(3)]
    _, dS, dw = FC.decompose_bwd_ref(xx.numpy(), S.numpy(), w.numpy(), *(FC.from_nvc(t.double(), 1, Fn).numpy() for t in grads))
    whole = SimpleNamespace(xx=xx.to(DEV), S=S.to(DEV), w=w.to(DEV), grads=[t.to(DEV) for t in grads])
    got = _run(_kernel_route, whole, dtype)
    cut = 40000
    for sl in (slice(0, cut), slice(cut, B)):
        part = _run(_kernel_route, SimpleNamespace(xx=whole.xx[sl].contiguous(), S=whole.S, w=whole.w,
                                                   grads=[t[sl].contiguous() for t in whole.grads]), dtype)
        for k in ("bar", "tilde", "prime", "gxx"):
            assert torch.equal(got[k][sl], part[k]), (k, sl)
    for k, ref in (("dS", dS), ("dw", dw)):
        e = rel_l2(got[k].reshape(-1), torch.from_numpy(ref).reshape(-1))
        print(f"FLD {mode} B {B} {k}: kernel {e:.3e} bound 4.000e-06")
        assert e <= 4e-6, (k, e)


class _Captured(Exception):
    pass


def _stacks_of_forward(m, xx, dtype):
    """The three tensors LES.forward hands its encoders (the forward is ended after the third)."""
    from turbdiff_amd.models import tfnet

    seen = []

    def record(self, x, c_enc=None, add4=None):
        seen.append(x)
        if len(seen) == 3:
            raise _Captured
        return x, x, x, x

    real = tfnet.Encoder.forward
    tfnet.Encoder.forward = record
    try:
        with pytest.raises(_Captured), torch.no_grad():
            m(xx, {}, dtype=dtype)
    finally:
        tfnet.Encoder.forward = real
    return seen


# one shape past each bound of fld_shape that a tensor of a test's size can have: (B, (T, L, F), grid)
REFUSED = [(1, (9, 1, 1), FC.HOST_GRID, "T > 8"), (1, (2, 1, 9), FC.HOST_GRID, "F > 8"), (1, (8, 1, 5), FC.HOST_GRID, "T F > 32")]
# and the two bounds on the grid, which only a grid of gigabytes passes: (grid, supported)
GRID_BOUNDS = [((2, 2**30, 1), False),        # V = 2^31
               ((1, 1, 2**28), False),        # V < 2^31 in 2^24 tiles: 2^32 threads along the launch's x axis
               ((1, 1, 2**28 - 16), True)]    # 2^24 - 1 tiles: the last grid of that kind the library takes


def test_refusals_write_nothing_and_the_model_takes_the_torch_route(monkeypatch):
    from turbdiff_amd import _lib as L
    from turbdiff_amd import ops
    from turbdiff_amd.models import tfnet

    lib = L.load()
    monkeypatch.setattr(tfnet, "FUSE_DECOMPOSE", True)
    cases = [(B, cfg, grid, torch.float32, L.F32, -2) for B, cfg, grid, _ in REFUSED] + [(1, SHIPPED, FC.HOST_GRID, torch.float16, L.F16, -3)]
    for B, (T, Ln, Fn), grid, dtype, code, want_rc in cases:
        t0 = time.perf_counter()
        V = grid[0] * grid[1] * grid[2]
        assert FC.supported(B, T, Ln, Fn, grid) == (want_rc == -3)
        n = T - Ln + 1
        cp = FC.up8(n * Fn)
        g = torch.Generator().manual_seed(T * Fn)
        xx = torch.randn(B, T, Fn, *grid, generator=g).to(DEV)
        S, w = (torch.randn(1, 1, 3, 3, 3, generator=g) / 27 ** 0.5).to(DEV), (torch.randn(1, Ln, 1, 1, 1, generator=g) / Ln ** 0.5).to(DEV)
        outs = [torch.full((B, *grid, cp), 7.0, dtype=dtype, device=DEV) for _ in range(3)]
        gxx = torch.full_like(xx, 7.0)
        gs, gw = torch.full((27,), 7.0, device=DEV), torch.full((Ln,), 7.0, device=DEV)
        ws = torch.full(((27 + Ln) * B * V,), 7.0, dtype=torch.float64, device=DEV)
        if want_rc == -2:
            assert L.query("tdx_flow_decompose_workspace_bytes", B, T, Ln, Fn, *grid) == 0
        shape = (B, T, Ln, Fn, *grid)
        rc = lib.tdx_flow_decompose_fwd(L.ptr(xx), L.ptr(S), L.ptr(w), *(L.ptr(o) for o in outs), *shape, code, L.stream())
        assert rc == want_rc, (T, Ln, Fn, dtype, rc)
        rc = lib.tdx_flow_decompose_bwd(L.ptr(xx), L.ptr(S), L.ptr(w), *(L.ptr(o) for o in outs), L.ptr(gxx), L.ptr(gs), L.ptr(gw),
                                        *shape, code, L.ptr(ws), L.stream())
        assert rc == want_rc, (T, Ln, Fn, dtype, rc)
        torch.cuda.synchronize()
        for t in (*outs, gxx, gs, gw, ws):
            assert torch.all(t == 7.0)
        assert not ops.flow_decompose_supported(xx, S, w, dtype)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.flow_decompose(xx, S, w, dtype)

        # LES.forward: the torch route, and what it feeds the encoders still matches float64
        m = tfnet.LES(n_features=Fn, c_local_features=8, c_global_features=0, context_window=T, kernel_size=3, dropout_rate=0,
                      temporal_filtering_length=Ln).to(DEV)
        with torch.no_grad():
            m.spatial_filter.weight.copy_(S)
            m.temporal_filter.weight.copy_(w)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "flow_decompose", lambda *a: pytest.fail("the kernels' route was taken"))
            seen = _stacks_of_forward(m, xx, dtype)
        for got, ref in zip(seen, FC.decompose_ref(xx.cpu(), S.cpu().reshape(3, 3, 3), w.cpu())):
            e = rel_l2(got, FC.to_nvc(ref))
            print(f"FLD refused B {B} {(T, Ln, Fn)} {grid} {dtype}: torch route {e:.3e}")
            assert got.dtype == dtype and got.shape == (B, *grid, cp) and e < (1e-5 if dtype == torch.float32 else 1e-3)
        torch.cuda.synchronize()
        print(f"FLD refused B {B} {(T, Ln, Fn)} {grid} {dtype}: {time.perf_counter() - t0:.2f} s")


def test_refusals_at_the_bounds_on_the_grid():
    """V >= 2^31 and 2^24 tiles or more.  A refused call launches nothing, so the entries get the shape with sentinel buffers
    of a few elements (a wrong launch would show in them or fault); the one supported grid here is only asked about, never
    run.  flow_decompose_supported needs a tensor of the shape: allocated, never filled."""
    from turbdiff_amd import _lib as L
    from turbdiff_amd import ops

    lib = L.load()
    S, w = torch.randn(1, 1, 3, 3, 3, device=DEV), torch.ones(1, 1, 1, 1, 1, device=DEV)
    for grid, ok in GRID_BOUNDS:
        shape = (1, 1, 1, 1, *grid)
        assert FC.supported(1, 1, 1, 1, grid) == ok
        assert (L.query("tdx_flow_decompose_workspace_bytes", 1, 1, 1, 1, *grid) > 0) == ok, grid
        xx = torch.empty(1, 1, 1, *grid, device=DEV)
        assert ops.flow_decompose_supported(xx, S, w, torch.float32) == ok, grid
        del xx
        if ok:
            continue
        bufs = [torch.full((64,), 7.0, device=DEV) for _ in range(8)]
        ws = torch.full((64,), 7.0, dtype=torch.float64, device=DEV)
        x, outs, gxx, gs, gw = bufs[0], bufs[1:4], bufs[4], bufs[5], bufs[6]
        rc = lib.tdx_flow_decompose_fwd(L.ptr(x), L.ptr(S), L.ptr(w), *(L.ptr(o) for o in outs), *shape, L.F32, L.stream())
        assert rc == -2, (grid, rc)
        rc = lib.tdx_flow_decompose_bwd(L.ptr(x), L.ptr(S), L.ptr(w), *(L.ptr(o) for o in outs), L.ptr(gxx), L.ptr(gs), L.ptr(gw),
                                        *shape, L.F32, L.ptr(ws), L.stream())
        assert rc == -2, (grid, rc)
        torch.cuda.synchronize()
        assert all(torch.all(t == 7.0) for t in (*bufs, ws)), grid


def test_supported_call_takes_the_kernels_when_the_switch_is_on(monkeypatch):
    from turbdiff_amd import ops
    from turbdiff_amd.models import tfnet

    m = tfnet.LES(**TC.MODEL_KW).to(DEV)
    xx = torch.randn(1, TC.T, TC.F_, *FC.HOST_GRID, device=DEV)
    calls = []
    real = ops.flow_decompose
    monkeypatch.setattr(ops, "flow_decompose", lambda *a: calls.append(1) or real(*a))
    for on in (True, False):
        monkeypatch.setattr(tfnet, "FUSE_DECOMPOSE", on)
        del calls[:]
        seen = _stacks_of_forward(m, xx, torch.bfloat16)
        assert len(calls) == int(on) and all(s.shape == (1, *FC.HOST_GRID, 16) and s.dtype == torch.bfloat16 for s in seen)


# ---------------------------------------------------------------------------------------------------- model

@functools.lru_cache(maxsize=None)
def _model_quantities(mode, on):
    import test_tfnet_gpu as TG
    from turbdiff_amd.models import tfnet

    old = tfnet.FUSE_DECOMPOSE
    tfnet.FUSE_DECOMPOSE = on
    try:
        return TG._model_quantities.__wrapped__(mode, True)
    finally:
        tfnet.FUSE_DECOMPOSE = old


def test_model_f32_against_the_reference():
    import test_tfnet_gpu as TG

    G = TG.G
    q, qoff = _model_quantities("f32", True), _model_quantities("f32", False)
    names, zero = TG._compared("train/")
    names.append("eval/y")
    assert "train/dx" in names and "train/grad/spatial_filter.weight" in names and "train/grad/temporal_filter.weight" in names
    failures = []
    for k in names:
        e, eoff, bound = TG._err(q[k], G[k]), TG._err(qoff[k], G[k]), TG._f32_bound(k)
        print(f"FLD LES f32 {k}: on {e:.3e} off {eoff:.3e} bound {bound:.3e}")
        if not e <= bound:
            failures.append((k, e, bound))
    for k in zero:  # zero in exact arithmetic: against the same block's BatchNorm-bias gradient, as test_tfnet_gpu.py does
        bn_bias = k.replace(".0.bias", ".1.bias")
        noise, scale, bound = q[k].norm().item(), torch.from_numpy(G[bn_bias]).norm().item(), TG._f32_bound(bn_bias)
        print(f"FLD LES f32 {k}: on {noise / scale:.3e} off {qoff[k].norm().item() / scale:.3e} bound {bound:.3e}")
        if not noise <= bound * scale:
            failures.append((k, noise / scale, bound))
    assert not failures, failures


def test_model_bf16_on_no_worse_than_off():
    import test_tfnet_gpu as TG

    G = TG.G
    qon, qoff = _model_quantities("bf16", True), _model_quantities("bf16", False)
    names, _ = TG._compared("train/")
    names.append("eval/y")
    failures = []
    for k in names:
        e, eoff = TG._err(qon[k], G[k]), TG._err(qoff[k], G[k])
        bound = max(1.5 * eoff, TG.BF16_NORM_FLOOR) if "/gradnorm/" in k else 1.5 * eoff
        print(f"FLD LES bf16 {k}: on {e:.3e} off {eoff:.3e} ratio {e / eoff if eoff > 0 else 0.0:.2f} bound {bound:.3e}")
        if not e <= bound:
            failures.append((k, e, eoff))
    assert not failures, failures


def test_trainer_three_fit_steps_on_both_routes(monkeypatch):
    import test_tfnet_gpu as TG
    from turbdiff_amd.models import tfnet

    res = {}
    for on in (True, False):
        monkeypatch.setattr(tfnet, "FUSE_DECOMPOSE", on)
        torch.manual_seed(0)
        t = TG._task("bf16")
        batch = TG._batch(2)
        before = [p.detach().clone() for p in (t.model.spatial_filter.weight, t.model.temporal_filter.weight)]
        losses = [t.fit_step(batch).item() for _ in range(3)]
        t.train()
        with torch.no_grad():
            final = t.training_step(batch).item()
        moved = [not torch.equal(a, b) for a, b in zip(before, (t.model.spatial_filter.weight, t.model.temporal_filter.weight))]
        print(f"FLD trainer bf16 FUSE_DECOMPOSE={on}: losses {losses} final {final:.6f} filters moved {moved}")
        assert final < losses[0], (on, losses, final)
        assert all(moved), (on, moved)
        res[on] = losses
    assert abs(res[True][0] - res[False][0]) <= 1e-2 * abs(res[False][0]), res
