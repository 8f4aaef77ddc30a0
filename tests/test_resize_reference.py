"""The four kernels of csrc/tdx_resize.hip against the float64 reference of tests/resize_reference.py, element by element, on
every route the host picks (tests/resize_cases.py restates the routing and lists the shapes).  On the dyadic rows the kernels'
arithmetic is exact and the answer is the reference rounded once to the storage type (torch.equal); on the others every
element is held to the bound derived in the docstring of resize_reference.py.  No tolerance is a measured number and no
element is left out of a comparison.

Without a GPU: the reference against float64 F.interpolate and its autograd, the adjoint identity, the exactness preconditions
of every dyadic row, the route of every row and what the table reaches as a whole, E_a against the float32 taps, and the
restated routing against the library's own plan query (tdx_resize_plan) on every row, the earlier tests' shapes and 300
generated ones.
"""

from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import resize_cases as cases
import resize_reference as R

CASES = cases.CASES
IDS = [cases.case_id(c) for c in CASES]
DYADIC = [c for c in CASES if c.dyadic]
INEXACT = [c for c in CASES if not c.dyadic]
DTYPES = R.DTYPES


def _ids(rows):
    return [cases.case_id(c) for c in rows]


def _row(B, C, src, dst):
    return next(c for c in CASES if (c.B, c.C, c.src, c.dst) == (B, C, src, dst))


ZERO_DY = [_row(1, 8, (9, 9, 9), (17, 17, 17)), _row(1, 8, (3, 3, 3), (17, 17, 17)), _row(2, 16, (6, 3, 4), (13, 7, 9))]
LARGE_ADD = [_row(1, 8, (5, 9, 17), (9, 17, 33)), _row(1, 8, (2, 2, 2), (9, 9, 9)), _row(1, 8, (3, 3, 3), (17, 17, 17)),
             _row(1, 128, (6, 3, 7), (12, 6, 11)), _row(1, 8, (9, 9, 9), (5, 5, 5))]
UNREAD = _row(1, 8, (9, 9, 9), (5, 5, 5))

# ------------------------------------------------------------------------------------------------------------ without a GPU

# fp64 source positions clear of integers, or on them exactly (ratio 1/2, the two ends): float64 picks the same taps either way
CLEAR = [((5, 4, 3), (9, 9, 17)), ((13, 7, 6), (6, 3, 3)), ((6, 3, 4), (13, 7, 9)), ((1, 3, 4), (4, 1, 7)), ((7, 7, 7), (5, 5, 5))]


@pytest.mark.parametrize("src,dst", CLEAR, ids=[f"{s}-{d}" for s, d in CLEAR])
def test_reference_is_interpolate_and_its_autograd(src, dst):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, *src, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(2, *dst, 3, generator=g, dtype=torch.float64)
    add = torch.randn(2, *src, 3, generator=g, dtype=torch.float64)
    xa = x.permute(0, 4, 1, 2, 3).clone().requires_grad_()
    ya = F.interpolate(xa, size=dst, mode="trilinear", align_corners=True)
    ya.backward(dy.permute(0, 4, 1, 2, 3))
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    y = R.forward(x, dst)
    assert close(y, ya.detach().permute(0, 2, 3, 4, 1))
    dx = R.adjoint(dy, src)
    assert close(dx, xa.grad.permute(0, 2, 3, 4, 1))
    assert close(R.adjoint(dy, src, add), xa.grad.permute(0, 2, 3, 4, 1) + add)
    lhs, rhs = (y * dy).sum().item(), (x * dx).sum().item()  # <W x, g> = <x, W^T g>
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), (y * dy).abs().sum().item())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adjoint_identity_on_every_row_geometry(case):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, *case.src, 2, generator=g, dtype=torch.float64)
    dy = torch.randn(1, *case.dst, 2, generator=g, dtype=torch.float64)
    y, dx = R.forward(x, case.dst), R.adjoint(dy, case.src)
    assert abs((y * dy).sum().item() - (x * dx).sum().item()) <= 1e-12 * (y * dy).abs().sum().item()


EXACT = [(c, 1) for c in DYADIC] + [(c, 1024) for c in LARGE_ADD if c.dyadic]


@pytest.mark.parametrize("case,add_scale", EXACT, ids=[f"{cases.case_id(c)}-add{k}" for c, k in EXACT])
def test_dyadic_rows_meet_their_preconditions(case, add_scale):
    p = R.dyadic_inputs(case.src, case.dst, case.B, case.C, add_scale=add_scale)
    R.assert_exact(case.src, case.dst, p)
    assert p["dy"].abs().max().item() >= 1 and p["add"].abs().max().item() == 4 * add_scale


@pytest.mark.parametrize("case", INEXACT, ids=_ids(INEXACT))
def test_inexact_rows_are_inexact(case):
    """some float32 weight of the row differs from W_a: the row does test the bound, not exact arithmetic"""
    assert any(not torch.equal(torch.from_numpy(cases.axis_weights(cases.make_axis(i, o))).double(), R.axis_matrix(i, o))
               for i, o in zip(case.src, case.dst))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_row_takes_the_route_it_was_written_for(case):
    _, got = cases.routed(case)
    assert got == cases.expected(case), f"{case.why}: routed {got}"
    assert set(case.dtypes) <= set(DTYPES) and {"f32", "bf16"} & set(case.dtypes)


def test_the_table_reaches_every_kernel_route():
    seen = cases.coverage([(c.B, c.C, c.src, c.dst) for c in CASES])
    assert seen["fwd"] == {cases.PAIRS, cases.GATHER}
    assert seen["bwd"] == {2, 4, 6, 12, cases.GENERIC}
    assert seen["pairs_at_64"] == {(2, 8, 8), (4, 8, 8)}
    # at 32 voxels per pass (a multiple of the tile's z extent), at 85 (not one) and at 4 (half a z row)
    assert {24, 64, 512} <= seen["multi_pass_fwd"] and {24, 64, 512} <= seen["multi_pass_bwd"]
    assert (1, 1, 1) in seen["partial"] and (0, 0, 0) in seen["partial"] and seen["multi_partial_yz"]
    assert seen["gather_up"] and seen["max_span"] == cases.RS_KMAX  # the gather kernel up-samples too; K12's last candidate is used
    # every K and the generic adjoint run in float32 and bf16 at least
    for k in (2, 4, 6, 12, cases.GENERIC):
        assert any(c.bwd == k and {"f32", "bf16"} <= set(c.dtypes) for c in CASES)
    # every dyadic ratio the exact cases were asked for
    ratios = {(i - 1, o - 1) for c in DYADIC for i, o in zip(c.src, c.dst)}
    have = {Fraction(a, b) for a, b in ratios if b and a}
    assert {Fraction(1, 2), Fraction(1, 4), Fraction(1, 8), Fraction(3, 8), Fraction(3, 2), Fraction(2)} <= have
    assert any(a == 0 for a, b in ratios) and any(b == 0 for a, b in ratios)  # in == 1 and out == 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_error_matrices_cover_the_float32_taps(case):
    """|w~ - W_a| <= E_a + 2 u w~: the float32 weights as the kernels compute them (numpy float32) against the reference; the
    2 u w~ are the roundings of fl(1 - f~) and of its sum with f~ on a shared entry, which the bounds count among the R
    roundings of a term."""
    for i, o in zip(case.src, case.dst):
        Wf = torch.from_numpy(cases.axis_weights(cases.make_axis(i, o))).double()
        W, E = R.axis_matrix(i, o), R.axis_error(i, o)
        excess = (Wf - W).abs() - E - 2.0 * R.U * Wf
        assert excess.max().item() <= 0.0, f"axis {i} -> {o}: float32 weight outside E by {excess.max().item():.3e}"
        assert E.max().item() <= 2.0 * R.U * max(i - 1, 0) * (1.0 + R.U)  # and E is no more than delta


# ------------------------------------------------------------------------ the library's own answers (no GPU: nothing launches)

CODES = {"f32": 0, "bf16": 1, "f16": 3}  # TDX_F32, TDX_BF16, TDX_F16
EINVAL, ESHAPE, EDTYPE = -1, -2, -3  # TDX_EINVAL, TDX_ESHAPE, TDX_EDTYPE


def _ask(B, C, src, dst, dname):
    """tdx_resize_plan answers what resize_cases.route restates: both kernels, their tiles and tile counts, K, the spans"""
    from turbdiff_amd import _lib as L

    q = L.resize_plan(B, C, src, dst, CODES[dname])
    r = cases.route(B, C, src, dst)
    what = (B, C, src, dst, dname, q)
    grid = lambda h: (tuple(q[f"{h}_t{a}"] for a in "xyz"), tuple(q[f"{h}_n{a}"] for a in "xyz"))
    assert q["status"] == 0, what
    assert (q["fwd_kernel"], *grid("fwd")) == (r.fwd, r.fwd_tiles.tile, r.fwd_tiles.count), what
    if r.bwd == cases.GENERIC:
        assert (q["bwd_kernel"], q["bwd_k"], *grid("bwd")) == ("generic", 0, (0, 0, 0), (0, 0, 0)), what
    else:
        assert (q["bwd_kernel"], q["bwd_k"], *grid("bwd")) == ("tiled", r.bwd, r.bwd_tiles.tile, r.bwd_tiles.count), what
    assert tuple(q[f"span_{a}"] for a in "xyz") == r.spans, what
    return r


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_library_plans_every_row_as_restated(case):
    for dname in DTYPES:  # the format moves nothing
        r = _ask(case.B, case.C, case.src, case.dst, dname)
        assert (r.fwd, r.fwd_tiles.tile, r.bwd, None if r.bwd_tiles is None else r.bwd_tiles.tile, r.spans) == cases.expected(case)


def _generated(n=300, seed=30):
    """(B, C, src, dst): extents 1..40, every width class of make_tiles, B = 64 for every tenth so that the ~1024-workgroup
    rule of make_tiles is met from both sides"""
    g = torch.Generator().manual_seed(seed)
    draw = lambda hi, k=1: [int(v) for v in torch.randint(0, hi, (k,), generator=g)]
    widths = (8, 16, 24, 64, 128, 512)
    return [(64 if i % 10 == 9 else 1 + draw(2)[0], widths[draw(6)[0]], tuple(1 + v for v in draw(40, 3)), tuple(1 + v for v in draw(40, 3)))
            for i in range(n)]


def test_library_plans_earlier_and_generated_shapes_as_restated():
    shapes = _generated()
    assert len(shapes) == 300
    routes = [_ask(*s, ("f32", "bf16", "f16")[i % 3]) for i, s in enumerate(cases.EARLIER + shapes)][len(cases.EARLIER):]
    assert {r.fwd for r in routes} == {cases.PAIRS, cases.GATHER}
    assert {r.bwd for r in routes} == {2, 4, 6, 12, cases.GENERIC}
    # tiles that the workgroup rule shrank, and tiles it left alone although the tensor is wide enough to have a choice
    shrunk = [cases.make_tiles(*dst, C, B)[0] != cases.make_tiles(*dst, C, 0)[0] for B, C, _, dst in shapes]
    assert any(shrunk) and any(not s and B == 64 and C <= 64 for s, (B, C, _, _) in zip(shrunk, shapes))


def test_library_plan_statuses():
    import ctypes

    from turbdiff_amd import _lib as L

    status = lambda B, C, src, dst, code=L.BF16: L.resize_plan(B, C, src, dst, code)["status"]
    assert status(1, 8, (3, 3, 3), (5, 5, 5)) == 0
    assert status(1, 12, (3, 3, 3), (5, 5, 5)) == ESHAPE and status(1, 8 * 257, (3, 3, 3), (5, 5, 5)) == ESHAPE
    assert status(1, 8 * 256, (3, 3, 3), (5, 5, 5)) == 0
    for bad in ((0, 8, (3, 3, 3), (5, 5, 5)), (1, 8, (3, 0, 3), (5, 5, 5)), (1, 8, (3, 3, 3), (5, 5, 0)), (1, 0, (3, 3, 3), (5, 5, 5)),
                (1, 12, (3, 3, 3), (0, 5, 5))):  # the last: a bad extent comes before a bad width
        assert status(*bad) == EINVAL
    assert L.load().tdx_resize_plan(1, 3, 3, 3, 5, 5, 5, 8, L.BF16, None) == EINVAL
    # a code that is no tensor format (2: TDX_F32_SPLIT, a pack code): what tdx_resize_fwd / _bwd return for it, before any launch
    x, y = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    at = lambda buf: ctypes.cast(buf, ctypes.c_void_p)
    assert L.load().tdx_resize_fwd(at(x), at(y), 1, 1, 1, 1, 1, 1, 1, 8, 2, None) == EDTYPE
    assert L.load().tdx_resize_bwd(at(y), None, at(x), 1, 1, 1, 1, 1, 1, 1, 8, 2, None) == EDTYPE
    assert status(1, 8, (1, 1, 1), (1, 1, 1), 2) == EDTYPE and status(1, 12, (1, 1, 1), (1, 1, 1), 2) == ESHAPE
    plan = L.resize_plan(1, 12, (3, 3, 3), (5, 5, 5), L.BF16)
    assert all(v == 0 for k, v in plan.items() if k not in ("status", "fwd_kernel", "bwd_kernel"))  # an error leaves zeros


# ---------------------------------------------------------------------------------------------------------------- on the GPU


def _dev():
    return torch.device("cuda:0")


def _assert_route(case):
    _, got = cases.routed(case)
    assert got == cases.expected(case), f"{cases.case_id(case)} no longer takes its route: {got}"
    for dname in case.dtypes:  # and the library names the row's kernels and tiles itself
        _ask(case.B, case.C, case.src, case.dst, dname)


def _where(t, flat):
    return tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), t.shape))


def _assert_equal(got, ref, dt, what):
    """got == the reference rounded once to dt, every element"""
    assert torch.equal(ref.float().double(), ref), f"{what}: the reference is not exact in float32"
    want = ref.float().to(dt)
    if torch.equal(got, want):
        return
    diff = (got.double() - want.double()).abs()
    i = int(diff.argmax())
    raise AssertionError(f"{what}: {int((got != want).sum())} of {got.numel()} elements differ; worst at {_where(got, i)}: "
                         f"got {got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}")


def _assert_within(got, ref, bound, what):
    diff = (got.double() - ref).abs()
    bad = diff > bound
    n = int(bad.sum())
    if n == 0:
        return
    i = int((diff - bound).argmax())
    raise AssertionError(f"{what}: {n} of {got.numel()} elements outside the bound; worst at {_where(got, i)}: "
                         f"got {got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}, "
                         f"off by {diff.flatten()[i].item():.3e}, bound {bound.flatten()[i].item():.3e}")


def _inputs(case, dt, zero_dy=False, add_scale=1):
    """x, dy, add on the GPU in dt (values that dt holds exactly, as float64 for the reference)"""
    if case.dyadic:
        p = R.dyadic_inputs(case.src, case.dst, case.B, case.C, add_scale=add_scale)
        R.assert_exact(case.src, case.dst, p)
    else:
        g = torch.Generator().manual_seed(7)
        p = dict(x=torch.randn(case.B, *case.src, case.C, generator=g), dy=torch.randn(case.B, *case.dst, case.C, generator=g),
                 add=add_scale * torch.randn(case.B, *case.src, case.C, generator=g))
    if zero_dy:
        p["dy"] = torch.zeros_like(p["dy"])
    return {k: v.to(_dev()).to(dt) for k, v in p.items()}


def _check(case, got, ref, dt, what, bound):
    if case.dyadic:
        _assert_equal(got, ref, dt, what)
    else:
        _assert_within(got, ref, bound(), what)


def _run(case, dtypes, zero_dy=False, add_scale=1, all_uses=True):
    from turbdiff_amd import ops

    _assert_route(case)
    route = cases.route(case.B, case.C, case.src, case.dst)
    for name in dtypes:
        dt = DTYPES[name]
        p = _inputs(case, dt, zero_dy, add_scale)
        x, dy, add = p["x"], p["dy"], p["add"]
        tag = f"{cases.case_id(case)} {name}"
        y_ref, dx_ref, dxa_ref = R.forward(x, case.dst), R.adjoint(dy, case.src), R.adjoint(dy, case.src, add)
        fwd_bound = lambda: R.forward_bound(x, case.dst, route, y_ref, dt)
        bwd_bound = lambda: R.adjoint_bound(dy, case.src, route, dx_ref, dt)
        add_bound = lambda: R.adjoint_bound(dy, case.src, route, dxa_ref, dt, add)

        # both outputs used: the adjoint takes add = g_skip
        leaf = x.clone().requires_grad_()
        skip, y = ops.skip_and_resize(leaf, case.dst)
        assert torch.equal(skip, x)
        _check(case, y.detach(), y_ref, dt, f"{tag} forward ({route.fwd})", fwd_bound)
        torch.autograd.backward([skip, y], [add, dy])
        _check(case, leaf.grad, dxa_ref, dt, f"{tag} adjoint + add ({route.bwd})", add_bound)
        if zero_dy:
            assert torch.equal(leaf.grad, add), f"{tag}: dy = 0, yet dx is not add bit for bit"
        if case is UNREAD:
            mask = R.unread(case.src, case.dst).to(x.device)
            assert int(mask.sum()) > 0 and torch.equal(leaf.grad[:, mask], add[:, mask]), f"{tag}: unread inputs must get add"
        if not all_uses:
            continue

        # ops.resize: the same forward, the adjoint without add
        leaf = x.clone().requires_grad_()
        y2 = ops.resize(leaf, case.dst)
        assert torch.equal(y2, y), f"{tag}: resize and skip_and_resize disagree"
        y2.backward(dy)
        _check(case, leaf.grad, dx_ref, dt, f"{tag} adjoint ({route.bwd})", bwd_bound)
        if case is UNREAD:
            assert torch.equal(leaf.grad[:, mask], torch.zeros_like(leaf.grad[:, mask])), f"{tag}: unread inputs must get 0"
        dx_plain = leaf.grad

        # the skip unused: the adjoint without add, through the other node
        leaf = x.clone().requires_grad_()
        skip, y = ops.skip_and_resize(leaf, case.dst)
        y.backward(dy)
        assert torch.equal(leaf.grad, dx_plain), f"{tag}: skip unused"

        # the resized output unused: the gradient is g_skip itself
        leaf = x.clone().requires_grad_()
        skip, y = ops.skip_and_resize(leaf, case.dst)
        skip.backward(add)
        assert torch.equal(leaf.grad, add), f"{tag}: resized output unused"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_element_of_forward_adjoint_and_fused_add(case):
    _run(case, case.dtypes)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ZERO_DY, ids=_ids(ZERO_DY))
def test_zero_dy_returns_add_bit_for_bit(case):
    _run(case, case.dtypes, zero_dy=True, all_uses=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE_ADD, ids=_ids(LARGE_ADD))
def test_add_three_orders_of_magnitude_above_dy(case):
    """add is 1024 times the scale of dy: the bound grows by u |add| only, so a dropped add is off by ~10^3 and a doubled one
    likewise, while a wrong dy term (~1) still stands 4 orders of magnitude above the bound."""
    _run(case, case.dtypes, add_scale=1024, all_uses=False)
