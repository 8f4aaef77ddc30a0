"""The activation codes of the GroupNorm kernels (TDX_ACT_GELU / RELU / SOFTPLUS / TANH; csrc/tdx_act.h) on the GPU: the two
streaming entries against the float64 reference and derived bounds of tests/act_reference.py, the two fused tails against the
launches they replace (torch.equal), ops.resnet_block against a float64 composition with the unfused route as the yardstick,
and whole models against vectors of the unmodified reference (tests/golden/actfn.npz, make_golden_actfn.py)."""

import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import act_reference as A
import gn_cases as cases
import gn_reference as R
from conftest import assert_grad_close, rel_l2
from step_inputs import rnd

pytestmark = pytest.mark.gpu

NEW = [A.GELU, A.RELU, A.SOFTPLUS, A.TANH]
BOUNDED = [A.GELU, A.SOFTPLUS, A.TANH]
DTYPES = cases.DTYPES
FLAGS = [(film, res) for film in (False, True) for res in (False, True)]
BOTH_BRANCHES = (3, 512, 8, 150)  # with FiLM, n > 20 at 54 (seed 0) and 19 (seed 1) of its 230 400 elements
OVER_THRESHOLD = {0: 54, 1: 19}


def _sid(shape):
    return "x".join(map(str, shape))


def _act_ids(codes):
    return [A.NAMES[c] for c in codes]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed=0):
    return {k: v.to(dev()) for k, v in R.dyadic_inputs(shape, seed=seed, narrow=True).items()}


# (shape, seed): every small shape, and the second seed of the shape that has both Softplus branches
CASES = [(s, 0) for s in cases.SMALL] + [(BOTH_BRANCHES, 1)]
CASE_IDS = [f"{_sid(s)}-seed{seed}" for s, seed in CASES]


def _lanes(shape):
    """(n_t + rows) of the streaming grid: the roundings a term of P or Q passes through (gn_reference, act = 1)"""
    B, C, G, V = shape
    blocks, stride, _, _ = cases.lane_paths(B, C, V)
    return -(-V // stride) + stride // blocks


def _apply(L, x, p, film, res, act, G):
    B, V, C = x.shape
    y = torch.empty_like(x)
    L.call("tdx_gn_apply", L.ptr(x), L.ptr(p["stats"]), L.ptr(p["gamma"]), L.ptr(p["beta"]), L.ptr(p["scale"] if film else None),
           L.ptr(p["shift"] if film else None), L.ptr(res), L.ptr(y), B, V, C, G, int(act), L.dtype_code(x.dtype), L.stream())
    return y


def _bwd(L, x, dy, p, film, act, G):
    B, V, C = x.shape
    d = x.device
    ws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, C), dtype=torch.uint8, device=d)
    dx, dgamma, dbeta = torch.empty_like(x), torch.empty(C, device=d), torch.empty(C, device=d)
    dscale, dshift = (torch.empty(B, C, device=d), torch.empty(B, C, device=d)) if film else (None, None)
    L.call("tdx_gn_bwd", L.ptr(x), L.ptr(dy), L.ptr(p["stats"]), L.ptr(p["gamma"]), L.ptr(p["beta"]),
           L.ptr(p["scale"] if film else None), L.ptr(p["shift"] if film else None), L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta),
           L.ptr(dscale), L.ptr(dshift), B, V, C, G, int(act), L.dtype_code(x.dtype), L.ptr(ws), L.stream())
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dscale=dscale, dshift=dshift)


def _worst(got, ref, bound):
    """the largest |got - ref| / bound and where, for the message of a failed assertion"""
    ratio = (got.double() - ref).abs() / bound
    i = int(ratio.argmax())
    return f"worst at flat index {i}: got {got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}, " \
           f"bound {bound.flatten()[i].item():.3e} ({ratio.flatten()[i].item():.3f} of it)"


def _within(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


def _pre(p, film):
    sc, sh = (p["scale"], p["shift"]) if film else (None, None)
    n, _ = R.pre_activation(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh)
    assert n.abs().max().item() <= R.N_MAX and torch.equal(n.float().double(), n)  # exact in float32: only f(n) errs
    return sc, sh, n


def _assert_branches(act, shape, seed, film, n):
    """The conditions the reference alone decides, before anything is launched."""
    if act == A.RELU and shape[3] > 5:
        assert bool((n == 0).any()), "no n == 0: ReLU's derivative at 0 is not exercised"
    if act == A.SOFTPLUS and shape == BOTH_BRANCHES and film:
        assert n.numel() == 230400 and int((n > A.THRESHOLD).sum()) == OVER_THRESHOLD[seed] and bool((n <= A.THRESHOLD).any())


# ------------------------------------------------------------------------------------------ 1, 2: tdx_gn_apply / tdx_gn_bwd


@pytest.mark.parametrize("shape,seed", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("act", BOUNDED, ids=_act_ids(BOUNDED))
def test_apply_within_the_derived_bound(act, shape, seed):
    from turbdiff_amd import _lib as L

    G = shape[2]
    p = _inputs(shape, seed)
    for film, res in FLAGS:
        sc, sh, n = _pre(p, film)
        _assert_branches(act, shape, seed, film, n)
        r = p["res"] if res else None
        ref = A.apply(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh, r, act)
        for name, dt in DTYPES.items():
            y = _apply(L, p["x"].to(dt), p, film, None if r is None else r.to(dt), act, G)
            bound = A.apply_bound(n, r, ref, dt, act)
            assert _within(y, ref, bound), f"{name} film={film} res={res}: {_worst(y, ref, bound)}"


@pytest.mark.parametrize("shape,seed", CASES, ids=CASE_IDS)
def test_apply_with_relu_is_the_reference_rounded_once(shape, seed):
    from turbdiff_amd import _lib as L

    G = shape[2]
    p = _inputs(shape, seed)
    for film, res in FLAGS:
        sc, sh, n = _pre(p, film)
        ref = A.apply(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh, p["res"] if res else None, A.RELU)
        assert torch.equal(ref.float().double(), ref)  # exact in float32: the store to T is the one rounding
        for name, dt in DTYPES.items():
            y = _apply(L, p["x"].to(dt), p, film, p["res"].to(dt) if res else None, A.RELU, G)
            want = ref.float().to(dt)
            assert torch.equal(y, want), f"{name} film={film} res={res}: {int((y != want).sum())} of {y.numel()} elements differ"


@pytest.mark.parametrize("shape,seed", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("act", BOUNDED, ids=_act_ids(BOUNDED))
def test_backward_within_the_derived_bounds(act, shape, seed):
    from turbdiff_amd import _lib as L

    B, C, G, V = shape
    p = _inputs(shape, seed)
    for film in (False, True):
        sc, sh, n = _pre(p, film)
        _assert_branches(act, shape, seed, film, n)
        ref = A.bwd(p["x"], p["dy"], p["stats"], p["gamma"], p["beta"], sc, sh, act)
        for name, dt in DTYPES.items():
            bounds = A.bwd_bounds(ref, p["dy"], p["gamma"], p["beta"], _lanes(shape), G, V, dt, act)
            got = _bwd(L, p["x"].to(dt), p["dy"].to(dt), p, film, act, G)
            for key in ("dx", "dgamma", "dbeta") + (("dscale", "dshift") if film else ()):
                want = getattr(ref, key)
                assert _within(got[key], want, bounds[key]), f"{name} film={film} {key}: {_worst(got[key], want, bounds[key])}"


@pytest.mark.parametrize("shape,seed", CASES, ids=CASE_IDS)
def test_backward_with_relu_exact_sums_and_two_roundings(shape, seed):
    """dn = dy or 0 (0 at n == 0, as torch): P and Q are exact as with act = 0 (tests/test_act_reference.py holds the
    preconditions), the four parameter gradients equal the reference cast to float32, dx is two float32 roundings away."""
    from turbdiff_amd import _lib as L

    G = shape[2]
    p = _inputs(shape, seed)
    for film in (False, True):
        sc, sh, n = _pre(p, film)
        _assert_branches(A.RELU, shape, seed, film, n)
        ref = A.bwd(p["x"], p["dy"], p["stats"], p["gamma"], p["beta"], sc, sh, A.RELU)
        for name, dt in DTYPES.items():
            got = _bwd(L, p["x"].to(dt), p["dy"].to(dt), p, film, A.RELU, G)
            for key in ("dgamma", "dbeta") + (("dscale", "dshift") if film else ()):
                want = getattr(ref, key).float()
                assert torch.equal(got[key], want), \
                    f"{name} film={film} {key}: {int((got[key] != want).sum())} of {want.numel()} differ, " \
                    f"by up to {(got[key].double() - want.double()).abs().max().item()!r}"
            bound = R.dx_rounding(ref.terms, ref.dx, dt)
            assert _within(got["dx"], ref.dx, bound), f"{name} film={film} dx: {_worst(got['dx'], ref.dx, bound)}"


# ------------------------------------------------------------------------------------------------- 3: the two tail identities


def _tail_operands(B, C, G, V, dt, d):
    """h spans every function's tails (|n| up to ~40, past Softplus's threshold)"""
    h = (8 * rnd(B, V, C, seed=7)).to(d).to(dt)
    stats = torch.stack((rnd(B, G, seed=8) * 0.1, rnd(B, G, seed=9).abs() + 0.5), dim=-1).contiguous().to(d)
    return h, stats, rnd(C, seed=10).to(d), rnd(C, seed=11).to(d)


@pytest.mark.parametrize("case", cases.ENCODED, ids=[_sid(c) for c in cases.ENCODED])
@pytest.mark.parametrize("act", NEW, ids=_act_ids(NEW))
def test_apply_encoded_act_equals_encode_then_apply_bitwise(act, case):
    """include/tdx.h: tdx_gn_apply_encoded_act == tdx_encode_fwd + tdx_gn_apply(res = its output, act), bit for bit"""
    from turbdiff_amd import _lib as L

    B, D, with_c, G, V = case
    d = dev()
    C = 2 * D if with_c else D
    x, wx, bx = rnd(B, 4, V, seed=1).to(d), rnd(D, 4, seed=3).to(d), rnd(D, seed=4).to(d)
    c, wc, bc = (rnd(4, V, seed=2).to(d), rnd(D, 4, seed=5).to(d), rnd(D, seed=6).to(d)) if with_c else (None, None, None)
    Fc = 4 if with_c else 0
    for name, dt in DTYPES.items():
        code = L.dtype_code(dt)
        h, stats, gamma, beta = _tail_operands(B, C, G, V, dt, d)
        skip = torch.empty(B, V, C, device=d, dtype=dt)
        L.call("tdx_encode_fwd", L.ptr(x), 4, L.ptr(wx), L.ptr(bx), L.ptr(c), Fc, L.ptr(wc), L.ptr(bc), L.ptr(skip), B, V, D, code,
               L.stream())
        want = torch.empty_like(h)
        L.call("tdx_gn_apply", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), None, None, L.ptr(skip), L.ptr(want), B, V, C, G,
               act, code, L.stream())
        got = torch.empty_like(h)
        L.call("tdx_gn_apply_encoded_act", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(x), 4, L.ptr(wx), L.ptr(bx),
               L.ptr(c), Fc, L.ptr(wc), L.ptr(bc), L.ptr(got), B, V, D, G, code, act, L.stream())
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ"


@pytest.mark.parametrize("case", cases.DECODE, ids=[_sid(c) for c in cases.DECODE])
@pytest.mark.parametrize("act", NEW, ids=_act_ids(NEW))
def test_apply_decode_act_equals_apply_then_decode_bitwise(act, case):
    """include/tdx.h: tdx_gn_apply_decode_act == tdx_gn_apply(res, act) + tdx_decode_fwd, bit for bit"""
    from turbdiff_amd import _lib as L

    B, C, G, V = case
    d = dev()
    w, bias = rnd(4, C, seed=12).to(d), rnd(4, seed=13).to(d)
    for name, dt in DTYPES.items():
        code = L.dtype_code(dt)
        h, stats, gamma, beta = _tail_operands(B, C, G, V, dt, d)
        r = rnd(B, V, C, seed=2).to(d).to(dt)
        y = torch.empty_like(h)
        L.call("tdx_gn_apply", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), None, None, L.ptr(r), L.ptr(y), B, V, C, G, act,
               code, L.stream())
        want = torch.empty(B, 4, V, device=d)
        L.call("tdx_decode_fwd", L.ptr(y), L.ptr(w), L.ptr(bias), L.ptr(want), B, V, C, 4, code, L.stream())
        got = torch.empty_like(want)
        L.call("tdx_gn_apply_decode_act", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(r), L.ptr(w), L.ptr(bias),
               L.ptr(got), B, V, C, G, 4, code, act, L.stream())
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} elements differ"


# ------------------------------------------------------------------------------------------------------ 4: an unknown code


@pytest.mark.parametrize("act", [6, -1])
def test_unknown_activation_code_is_a_bad_argument(act):
    """Before this family every non-zero `act` silently meant SiLU: now TDX_EINVAL, and nothing is launched (the outputs
    keep their fill)."""
    from turbdiff_amd import _lib as L

    shape = (1, 8, 1, 5)
    B, C, G, V = shape
    p = _inputs(shape)
    with pytest.raises(RuntimeError, match="TDX_EINVAL"):
        _apply(L, p["x"], p, True, p["res"], act, G)
    with pytest.raises(RuntimeError, match="TDX_EINVAL"):
        _bwd(L, p["x"], p["dy"], p, True, act, G)
    d = dev()
    out = torch.full((B, V, C), 7.0, device=d)
    wx, bx = rnd(C, 4, seed=3).to(d), rnd(C, seed=4).to(d)
    with pytest.raises(RuntimeError, match="TDX_EINVAL"):
        L.call("tdx_gn_apply_encoded_act", L.ptr(p["x"]), L.ptr(p["stats"]), L.ptr(p["gamma"]), L.ptr(p["beta"]),
               L.ptr(rnd(B, 4, V, seed=1).to(d)), 4, L.ptr(wx), L.ptr(bx), None, 0, None, None, L.ptr(out), B, V, C, G, L.F32, act,
               L.stream())
    dec = torch.full((B, 4, V), 7.0, device=d)
    with pytest.raises(RuntimeError, match="TDX_EINVAL"):
        L.call("tdx_gn_apply_decode_act", L.ptr(p["x"]), L.ptr(p["stats"]), L.ptr(p["gamma"]), L.ptr(p["beta"]), L.ptr(p["res"]),
               L.ptr(rnd(4, C, seed=12).to(d)), L.ptr(rnd(4, seed=13).to(d)), L.ptr(dec), B, V, C, G, 4, L.F32, act, L.stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dec == 7.0).all())


# ------------------------------------------------------------------------------------------------------ 5: ops.resnet_block

GRID = (10, 6, 5)  # small, odd, two streaming blocks per sample at 16 and 32 channels
C_DIM = 8


def _reference_block(blk, x, c, gy):
    """float64 CPU composition of the reference's ResnetBlock (ddpm.py:180-197) and its gradients w.r.t. x, c and every
    parameter: F.conv3d on replicate padding, F.group_norm, the torch module."""
    ref = blk_copy = type(blk)(blk.block1.conv.in_channels, blk.dim_out, c_dim=C_DIM, actfn=type(blk.block1.act),
                               norm_klass=lambda ch: nn.GroupNorm(8, ch)).double()
    blk_copy.load_state_dict({k: v.detach().cpu().double() for k, v in blk.state_dict().items()})
    xd = x.detach().cpu().double().permute(0, 4, 1, 2, 3).requires_grad_()  # NCDHW
    cd = c.detach().cpu().double().requires_grad_()
    scale, shift = ref.project_onto_scale_shift(cd).chunk(2, dim=1)

    def block(b, h, film):
        h = F.conv3d(F.pad(h, (1,) * 6, mode="replicate"), b.conv.weight, b.conv.bias)
        h = F.group_norm(h, b.norm.num_groups, b.norm.weight, b.norm.bias, b.norm.eps)
        if film is not None:
            h = h * (film[0][:, :, None, None, None] + 1) + film[1][:, :, None, None, None]
        return b.act(h)

    h = block(ref.block2, block(ref.block1, xd, (scale, shift)), None)
    skip = xd if isinstance(ref.conv, nn.Identity) else F.conv3d(xd, ref.conv.weight, ref.conv.bias)
    y = h + skip
    y.backward(gy.detach().cpu().double().permute(0, 4, 1, 2, 3))
    out = {"y": y.detach().permute(0, 2, 3, 4, 1), "x": xd.grad.permute(0, 2, 3, 4, 1), "c": cd.grad}
    out.update({name: q.grad for name, q in ref.named_parameters()})
    return out


def _run_block(blk, x, c, gy):
    xa, ca = x.clone().requires_grad_(), c.clone().requires_grad_()
    blk.zero_grad(set_to_none=True)
    y = blk(xa, ca)
    y.backward(gy)
    out = {"y": y.detach(), "x": xa.grad, "c": ca.grad}
    out.update({name: q.grad.clone() for name, q in blk.named_parameters()})
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cout", [16, 32], ids=["identity", "projected"])
@pytest.mark.parametrize("act", NEW, ids=_act_ids(NEW))
def test_resnet_block_no_worse_than_the_unfused_route(act, cout, dtype, monkeypatch, capsys):
    """ops.resnet_block(act) -- one autograd node, the activation inside the GroupNorm kernels -- against the float64 CPU
    composition; the yardstick is the route of before in the same run (FUSE_ACTFNS = False: act = 0 pass, torch module,
    torch add), which shares every conv and statistics kernel.  Gate: per tensor, rel-L2 error <= 1.5 x the unfused
    route's (the 1.5 covers the order-dependent atomics of the weight gradients).  Both errors are printed per tensor.

    As measured on an MI355X (fused / unfused rel-L2 of the output and the input gradient; smallest .. largest ratio over the 13-15
    tensors and where the largest is -- the 16- and 32-element bias gradients scatter most, on both sides of 1):
        gelu     16->16 bf16  y 2.78e-03 / 3.26e-03   x-grad 3.45e-03 / 3.93e-03   ratios 0.78 .. 1.44 (block2.conv.bias)
        gelu     16->16 f32   y 2.99e-07 / 3.02e-07   x-grad 3.45e-07 / 3.45e-07   ratios 0.69 .. 1.26 (block2.conv.bias)
        gelu     16->32 bf16  y 3.66e-03 / 4.52e-03   x-grad 4.91e-03 / 5.67e-03   ratios 0.77 .. 1.26 (block1.conv.bias)
        gelu     16->32 f32   y 5.55e-07 / 5.60e-07   x-grad 6.40e-07 / 6.45e-07   ratios 0.85 .. 1.09 (block2.conv.bias)
        relu     16->16 bf16  y 2.64e-03 / 2.88e-03   x-grad 2.72e-02 / 2.72e-02   ratios 0.92 .. 1.00 (x)
        relu     16->16 f32   y 2.88e-07 / 2.88e-07   x-grad 2.49e-07 / 2.49e-07   ratios 1.00 .. 1.00 (y)
        relu     16->32 bf16  y 3.45e-03 / 3.72e-03   x-grad 3.28e-02 / 3.28e-02   ratios 0.93 .. 1.00 (x)
        relu     16->32 f32   y 4.56e-07 / 4.56e-07   x-grad 4.75e-07 / 4.75e-07   ratios 0.84 .. 1.03 (block1.norm.bias)
        softplus 16->16 bf16  y 2.42e-03 / 2.92e-03   x-grad 2.68e-03 / 2.99e-03   ratios 0.49 .. 0.94 (project_onto_scale_shift.weight)
        softplus 16->16 f32   y 2.72e-07 / 2.70e-07   x-grad 2.20e-07 / 2.14e-07   ratios 0.80 .. 1.47 (block2.norm.bias)
        softplus 16->32 bf16  y 2.61e-03 / 3.29e-03   x-grad 3.17e-03 / 3.81e-03   ratios 0.62 .. 1.01 (project_onto_scale_shift.bias)
        softplus 16->32 f32   y 3.40e-07 / 3.38e-07   x-grad 3.59e-07 / 3.58e-07   ratios 0.74 .. 1.19 (block2.norm.bias)
        tanh     16->16 bf16  y 2.41e-03 / 2.68e-03   x-grad 3.69e-03 / 4.97e-03   ratios 0.32 .. 1.43 (block2.conv.bias)
        tanh     16->16 f32   y 2.31e-07 / 2.31e-07   x-grad 4.11e-07 / 4.10e-07   ratios 0.87 .. 1.36 (c)
        tanh     16->32 bf16  y 3.18e-03 / 3.49e-03   x-grad 4.71e-03 / 6.19e-03   ratios 0.63 .. 1.00 (conv.weight)
        tanh     16->32 f32   y 3.99e-07 / 3.99e-07   x-grad 6.40e-07 / 6.42e-07   ratios 0.98 .. 1.10 (c)
    """
    from turbdiff_amd import _lib as L
    from turbdiff_amd.models import ddpm as D

    d = dev()
    torch.manual_seed(act * 100 + cout)
    blk = D.ResnetBlock(16, cout, c_dim=C_DIM, actfn=A.MODULES[act], norm_klass=lambda ch: nn.GroupNorm(8, ch)).to(d)
    with torch.no_grad():
        for b in (blk.block1, blk.block2):
            b.norm.weight.add_(0.2 * torch.randn_like(b.norm.weight))
            b.norm.bias.add_(0.2 * torch.randn_like(b.norm.bias))
    x = rnd(2, *GRID, 16, seed=1).to(d).to(dtype)
    c = rnd(2, C_DIM, seed=2).to(d)
    gy = rnd(2, *GRID, cout, seed=3).to(d).to(dtype)
    want = _reference_block(blk, x, c, gy)

    seen = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a, **k: (seen.append((name, a)), orig(name, *a, **k))[1])
    hook = blk.block1.act.register_forward_hook(lambda *a: pytest.fail("the torch activation ran on the fused route"))
    hook2 = blk.block2.act.register_forward_hook(lambda *a: pytest.fail("the torch activation ran on the fused route"))
    assert blk.fused()
    fused = _run_block(blk, x, c, gy)
    hook.remove()
    hook2.remove()
    code = L.dtype_code(dtype)
    acts = [a[-3] for name, a in seen if name == "tdx_gn_apply"] + [a[-4] for name, a in seen if name == "tdx_gn_bwd"]
    assert acts == [act] * 4, acts  # two apply passes, two backwards, each with the block's code
    assert "tdx_conv1_fwd_gn" not in [name for name, _ in seen]  # that fusion evaluates SiLU only
    seen.clear()
    monkeypatch.setattr(D, "FUSE_ACTFNS", False)
    assert not blk.fused()
    plain = _run_block(blk, x, c, gy)
    assert {a[-3] for name, a in seen if name == "tdx_gn_apply"} == {0} and code is not None

    rows, bad = [], []
    for key in want:
        if want[key].double().norm().item() < 1e-6:  # a conv bias in front of a GroupNorm: mathematically zero
            continue
        ef, ep = rel_l2(fused[key].float(), want[key]), rel_l2(plain[key].float(), want[key])
        rows.append(f"{key:40s} fused {ef:.3e}  unfused {ep:.3e}  ratio {ef / ep if ep else float('inf'):.3f}")
        if not ef <= 1.5 * ep:
            bad.append(rows[-1])
    with capsys.disabled():
        print(f"\nresnet_block {A.NAMES[act]} 16->{cout} {dtype}: rel-L2 against float64\n  " + "\n  ".join(rows))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------- 6: model level

MODEL_TAGS = {"relu": nn.ReLU, "softplus": nn.Softplus, "tanh": nn.Tanh}


@pytest.mark.parametrize("tag", list(MODEL_TAGS))
def test_model_against_the_reference_through_the_fused_route(golden, tag, monkeypatch):
    """DenoisingModel(actfn=...) against vectors of the unmodified reference (tests/golden/actfn.npz) with the gates of
    test_hip_model.py::test_constructor_options_golden (1e-4, 1e-4, 2e-3), fp32.  No Block's torch activation runs, and the
    no-grad forward ends in the decode tail with the activation's code."""
    from turbdiff_amd import _lib as L
    from turbdiff_amd.models import ddpm as D
    from turbdiff_amd.models.conditioning import Conditioning

    g, opt = golden("actfn"), golden("options")
    net = D.DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=10, dim=8,
                           u_net_levels=2, norm_type="group", actfn=MODEL_TAGS[tag])
    sd = dict(golden("model_cfg1").sub("sd/"))
    sd.update(g.sub(f"{tag}/sd/"))
    net.load_state_dict(sd, strict=True)
    diff = D.GaussianDiffusion(net, timesteps=10, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True).to(dev())

    def never(module, *a):
        raise AssertionError(f"the torch module {module} of a Block ran: the activation belongs inside the GroupNorm kernels")

    blocks = [m for m in net.modules() if isinstance(m, D.Block)]
    assert len(blocks) == 14
    for b in blocks:
        b.act.register_forward_hook(never)
    seen = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a, **k: (seen.append(name), orig(name, *a, **k))[1])

    x, t = opt["x"].to(dev()), opt["t"].to(dev())
    C = {Conditioning.Type.CELL_TYPE: opt["c_local"].to(dev())}
    md = SimpleNamespace(cell_idx=opt["cell_idx"].to(dev()))
    with torch.no_grad():
        eps = diff.model(x, t, C)
    assert "tdx_gn_apply_decode_act" in seen and "tdx_gn_apply_encoded_act" in seen
    assert "tdx_gn_apply_decode" not in seen and "tdx_gn_apply_encoded" not in seen and "tdx_decode_fwd" not in seen
    assert rel_l2(eps.cpu(), g[f"{tag}/eps_hat"]) < 1e-4
    loss, _ = diff.p_losses(x, t, C, md, None, noise=g[f"{tag}/noise"].to(dev()))
    loss.backward()
    assert abs(loss.item() - g[f"{tag}/loss"].item()) < 1e-4 * abs(g[f"{tag}/loss"].item())
    for name, p in diff.model.named_parameters():
        ref = g[f"{tag}/gnorm/{name}"].item()
        got = p.grad.norm().item()
        assert abs(got - ref) < 2e-3 * ref + 2e-6, (name, got, ref)
        if f"{tag}/grad/{name}" in g.z.files:
            assert_grad_close(name, p.grad.cpu(), g[f"{tag}/grad/{name}"], 2e-3)
