"""The 1x1 convolution kernels (csrc/tdx_conv1.hip, tdx_conv1_mfma.hip, tdx_conv1_mfma_f32.hip) against the float64 reference of
tests/conv1_reference.py, element by element, on every kernel route of tests/conv1_cases.py.  On the exact inputs the reference
rounded at the route's rounding points is THE answer (torch.equal); elsewhere every element is held to a bound derived in the
docstring of conv1_reference.py.  No tolerance is a measured number and no element is left out.

Without a GPU: the reference against float64 F.conv3d and its autograd, the route and split plan every row is listed for
(against the restated host code of conv1_cases, and that restatement against the library's own answers: tdx_conv1_fwd_plan,
tdx_conv1_bwd_weight_plan), the exactness preconditions of every exact row, where the two rounding forms differ, and what the
table reaches.  On the GPU every call that a row's route is asserted for asks the library first, immediately before the launch.
"""

import ctypes
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv1_cases as cases
import conv1_reference as R
import gn_reference as G

DT = R.DTYPES
DNAME = {dt: name for name, dt in DT.items()}
MARGIN = 1024   # elements behind every forward output
SENTINEL = -768.0  # exact in bf16 and fp16
OFF, PAD_C, PAD_R = 6, 3, 2  # the gradient block starts at column OFF of a buffer PAD_C columns and PAD_R rows larger


def _names(table):
    return [c.name for c in table]


# ----------------------------------------------------------------------------------------------- comparisons (CPU and GPU)


def _share_left_out(mask, like):
    return 0.0 if mask is None else 1.0 - float(mask.expand_as(like).double().mean())


def _assert_equal(got, want, what, mask=None):
    """Every element, bit for bit.  `mask` is None everywhere in this file: a later edit that passes one must leave out nothing."""
    assert _share_left_out(mask, want) == 0.0, f"{what}: a mask leaves elements out of the comparison"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    if not torch.equal(got, want):
        bad = (got != want).flatten()
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {i}: "
                             f"got {got.flatten()[i].item()!r}, reference {want.flatten()[i].item()!r}")


def _assert_within(got, ref, bound, what, mask=None):
    assert _share_left_out(mask, ref) == 0.0, f"{what}: a mask leaves elements out of the comparison"
    assert got.shape == ref.shape
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        i = int((err / bound).argmax())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside their bound, worst at flat index {i}: "
                             f"got {got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}, "
                             f"bound {bound.flatten()[i].item():.3e}")


# ------------------------------------------------------------------------------------------------------------ without a GPU


@pytest.mark.parametrize("C1,C2,Cout,rows", [(5, 0, 7, 11), (8, 3, 4, 30), (32, 32, 16, 9)])
def test_reference_is_conv3d_and_its_autograd(C1, C2, Cout, rows):
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x1, x2, w, bias, add, dy = rn(rows, C1), (rn(rows, C2) if C2 else None), rn(C1 + C2, Cout), rn(Cout), rn(rows, Cout), rn(rows, Cout)
    x = R._cat(x1, x2).clone().requires_grad_()
    wp, bp = w.t().reshape(Cout, C1 + C2, 1, 1, 1).clone().requires_grad_(), bias.clone().requires_grad_()
    y = F.conv3d(x.t().reshape(1, C1 + C2, rows, 1, 1), wp, bp).reshape(Cout, rows).t() + add
    y.backward(dy)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert close(R.forward(x1, x2, w, bias, add)[1], y.detach())
    dW, db = R.wgrad(x.detach(), dy)
    assert close(dW, wp.grad.reshape(Cout, -1).t()) and close(db, bp.grad)
    w2 = w.t().contiguous()  # the parameter's (Cout, Cin) layout: the data gradient is a forward on its column blocks
    gx1 = R.forward(dy, None, R.weight_block(w2, 0, C1), None, None)[1]
    assert close(gx1, x.grad[:, :C1])
    if C2:
        assert close(R.forward(dy, None, R.weight_block(w2, C1, C2), None, None)[1], x.grad[:, C1:])


def test_tail_reference_is_silu_of_group_norm():
    B, V, C, Gr = 2, 13, 12, 3
    g = torch.Generator().manual_seed(2)
    h = torch.randn(B, V, C, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    n, s = R.tail(h, G.stats(h, Gr, 1e-5), gamma, beta, Gr)
    want = F.silu(F.group_norm(h.transpose(1, 2), Gr, gamma, beta, 1e-5).transpose(1, 2))
    assert torch.allclose(s, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", cases.FWD, ids=_names(cases.FWD))
def test_forward_rows_take_their_route_and_are_exact(case):
    c = case
    for dt in c.dtypes:
        assert cases.fwd_route(dt, c.C1, c.C2, c.Cout, c.ldw, c.col, c.add, c.direct).route == c.route, dt
    assert c.ldw >= c.col + c.Cout
    for narrow in ((False, True) if c.add else (False,)):
        R.assert_exact(R.exact_inputs(c.rows, c.C1, c.C2, c.Cout, narrow=narrow), c.bias, c.add, narrow)


def test_one_shape_is_listed_for_both_rounding_forms():
    v, h = (cases.by_name(cases.FWD, n) for n in cases.SAME_INPUTS)
    assert (v.route, h.route, v.direct, h.direct) == ("V", "H", True, False) and v.add and h.add and v.bias and h.bias
    assert v[3:7] == h[3:7] and v[9:11] == h[9:11] and set(v.dtypes) == set(h.dtypes) == set(cases.H16)  # the same tensors


def test_c6_data_gradient_splits_the_routes():
    """x2's data gradient of a layer with C1 = 6: w starts at column 6 of rows of 38 floats"""
    assert cases.fwd_route("bf16", 64, 0, 32, 38, 6, False) == cases.Route("H", "conv1_mfma_fwd_kernel<1,bf16>")
    assert cases.fwd_route("f32", 64, 0, 32, 38, 6, False).route == "V"
    assert cases.fwd_route("f32", 64, 0, 32, 40, 8, False).route == "F"  # aligned: the fp32 MFMA kernel again
    assert cases.fwd_route("f32", 64, 0, 32, 40, 6, False).route == "V"  # ldw fine, pointer not


@pytest.mark.parametrize("case", cases.FWD, ids=_names(cases.FWD))
def test_rounding_forms_differ_on_the_dense_family_with_an_addend_only(case):
    c = case
    for narrow in ((False, True) if c.add else (False,)):
        p = R.exact_inputs(c.rows, c.C1, c.C2, c.Cout, narrow=narrow)
        y0, _ = R.forward(p["x1"], p["x2"], p["w"], p["bias"] if c.bias else None, None)
        add = p["add"] if c.add else None
        for name, dt in DT.items():
            differ = not torch.equal(R.rounded_once(y0, add, dt), R.rounded_twice(y0, add, dt))
            # a row of a few elements need not hold a case where two roundings and one disagree: 1000 elements or more must
            must = c.add and not narrow and name != "f32"
            if must and y0.numel() >= 1000:
                assert differ, f"{name}: the dense family with an addend must pin H's two roundings against one"
            if not must:
                assert not differ, f"{name} narrow={narrow}: the two forms must coincide here"


@pytest.mark.parametrize("case", cases.TAIL, ids=_names(cases.TAIL))
def test_tail_rows_take_their_route_and_are_exact(case):
    c = case
    for dt in cases.H16:
        r = cases.gn_route(dt, c.C1, c.C2, c.Cout)
        assert r.route == "H" and r.kernel.startswith(f"conv1_mfma_fwd_kernel<{2 if c.Cout % 64 == 0 else 1},")
    assert c.Cout % c.G == 0
    p = R.exact_inputs(c.B * c.V, c.C1, c.C2, c.Cout)
    R.assert_exact(p, True, False)
    t = R.tail_inputs(c.B, c.V, c.Cout, c.G)
    G.assert_exact(dict(x=t["h"], stats=t["stats"], gamma=t["gamma"], beta=t["beta"], res=torch.zeros_like(t["h"])), False, True)


def test_tail_table_reaches_its_edges():
    T = {c.name: c for c in cases.TAIL}
    assert {c.V for c in cases.TAIL} == {27, 40, 100, 256, 300}
    assert {c.Cout // c.G for c in cases.TAIL} >= {1, 4, 8} and any(c.G == 1 for c in cases.TAIL)
    assert {c.Cout % 64 == 0 for c in cases.TAIL} == {True, False} and {c.C2 > 0 for c in cases.TAIL} == {True, False}
    stride = lambda c: 256 // ((64 if c.Cout % 64 == 0 else 32) // 8)  # rows between a thread's consecutive chunks
    assert any(c.V < stride(c) for c in cases.TAIL if c.Cout % 64 == 0) and any(c.V < stride(c) for c in cases.TAIL if c.Cout % 64)
    assert any(256 // c.V >= 2 for c in cases.TAIL)  # several samples share a tile
    assert any((c.B * c.V) % 256 == 0 for c in cases.TAIL)
    partial = [c for c in cases.TAIL if (c.B * c.V) % 256]
    assert any(((c.B * c.V) // 256 * 256) % c.V for c in partial)  # the partial last tile starts inside a sample
    assert any((c.Cout // c.G) == 4 for c in cases.TAIL)  # an 8-channel chunk spans two groups
    assert cases.gn_route("f32", 64, 0, 64) == "TDX_EDTYPE" and cases.gn_route("bf16", 40, 0, 64) == "TDX_ESHAPE"
    assert cases.gn_route("bf16", 64, 0, 64, direct=True) == "TDX_ESHAPE"
    assert set(cases.TAIL_INEXACT) <= set(T)


@pytest.mark.parametrize("case", cases.WGRAD, ids=_names(cases.WGRAD))
def test_weight_gradient_rows_take_their_route_and_plan(case):
    c = case
    for dt in c.dtypes:
        for tr in (0, 1):
            assert cases.wgrad_route(dt, c.Cin, c.Cout, tr, c.direct).route == c.route
    assert cases.plan(c.route, c.Cin, c.Cout, c.rows).steps == c.steps
    kind, plan = cases.det_plan(c.route, c.Cin, c.Cout, c.rows, cases.ARENA)
    assert kind == "slabs" and plan.steps == c.steps  # the arena never caps these shapes: the same splits, one slab each
    if c.name in cases.NO_ARENA:
        kind, plan = cases.det_plan(c.route, c.Cin, c.Cout, c.rows, 0)
        assert kind == "single" and plan.steps == cases.NO_ARENA_STEPS[c.name]
    R.assert_exact(R.exact_inputs(c.rows, c.Cin, 0, c.Cout), True, False)


def test_weight_gradient_table_reaches_its_edges():
    W = cases.WGRAD
    rows = {r: {c.rows for c in W if c.route == r} for r in "VHF"}
    assert rows["H"] | rows["F"] | rows["V"] >= {1, 31, 32, 33, 255, 256, 257}
    assert any(c.rows > 4096 for c in W if c.route == "V") and any(c.Cout == 4 for c in W if c.route == "V")
    assert any((c.Cin, c.Cout) == (40, 72) for c in W) and any(c.direct for c in W)
    for r in "HF":  # at least two loop trips for some but not all splits: the pipelined loop prefetches and drains
        assert any(max(c.steps) >= 2 and min(c.steps) == 1 and len(c.steps) >= 2 for c in W if c.route == r), r
    assert any(c.Cin == 160 for c in W if c.route == "F") and any(c.Cin == 256 for c in W if c.route == "F")
    # the smallest row count with nsplit < chunks at (1024, 1024): 256 tiles give nsplit = 2, so three chunks: 513 rows or more
    assert cases.plan_h(1024, 1024, 512).steps == (1, 1) and cases.plan_h(1024, 1024, 513).steps == (2, 1)
    # the vector kernel's row blocks are re-sized only when max_split binds: the single-split branch without an arena
    assert cases.plan_v(4097).steps == (128, 1) and cases.plan_v(4097, 1).steps == (129,)
    assert {cases.by_name(W, n).route for n in cases.NO_ARENA} == {"V", "H", "F"}


def _kernels_reached():
    reached = set()
    for c in cases.FWD:
        for dt in c.dtypes:
            k = cases.fwd_route(dt, c.C1, c.C2, c.Cout, c.ldw, c.col, c.add, c.direct).kernel
            reached.add((k, "add" if c.add else "plain") if k.startswith("conv1_mfma_fwd") else k)
    for c in cases.TAIL:
        for dt in cases.H16:
            reached.add((cases.gn_route(dt, c.C1, c.C2, c.Cout).kernel, "gn"))
    for c in cases.WGRAD:
        for dt in c.dtypes:
            for tr in (0, 1):
                reached.add(cases.wgrad_route(dt, c.Cin, c.Cout, tr, c.direct).kernel)
    return reached


def test_table_reaches_every_template_instantiation():
    """what the three launchers and the two vector-ALU dispatches can launch"""
    every = {f"conv1_fwd_kernel<{t}>" for t in cases.ALL} | {f"conv1_wgrad_kernel<{t}>" for t in cases.ALL}
    every |= {(f"conv1_mfma_fwd_kernel<{nt},{t}>", a) for nt in (1, 2) for t in cases.H16 for a in ("plain", "add", "gn")}
    every |= {f"conv1_wgrad_mfma_kernel<{m},{n},{tr},{t}>" for m in (1, 2) for n in (1, 2) for tr in (0, 1) for t in cases.H16}
    every |= {f"conv1_f32_mfma_fwd_kernel<{nt},{a}>" for nt in (1, 2) for a in (0, 1)}
    every |= {f"conv1_f32_mfma_wgrad_kernel<{nt},{tr}>" for nt in (1, 2) for tr in (0, 1)}
    assert _kernels_reached() == every
    pairs = {(c.route, dt) for c in cases.FWD for dt in c.dtypes} | {(c.route, dt) for c in cases.WGRAD for dt in c.dtypes}
    assert pairs == {("V", "f32"), ("V", "bf16"), ("V", "f16"), ("H", "bf16"), ("H", "f16"), ("F", "f32")}


def test_forward_table_reaches_its_edges():
    for r, T in cases.TILE_ROWS.items():
        rows = {c.rows for c in cases.FWD if c.route == r}
        assert rows >= {1, T - 1, T, T + 1} and any(x > 2 * T and x % T for x in rows), r
    for r in "HF":
        assert {c.Cout for c in cases.FWD if c.route == r} >= {32, 96, 64, 192, 160}
        assert {(c.C1, c.C2) for c in cases.FWD if c.route == r} >= {(32, 96), (64, 64), (1024, 0)}
        assert {(c.bias, c.add) for c in cases.FWD if c.route == r} == set(itertools.product((True, False), repeat=2))
        assert {c.col for c in cases.FWD if c.route == r and c.ldw > c.Cout} >= {0, 32}
    v = [c for c in cases.FWD if c.route == "V"]
    assert {c.Cout for c in v} >= {4, 72} and any(c.C1 + c.C2 == 4 for c in v) and any((c.C1, c.C2) == (40, 24) for c in v)
    assert any(c.direct and "f32" in c.dtypes for c in v) and any(c.direct and "bf16" in c.dtypes for c in v)
    assert any(c.col == 6 for c in v) and any(c.col == 6 for c in cases.FWD if c.route == "H")
    assert set(cases.FWD_INEXACT) <= set(_names(cases.FWD)) and set(cases.WGRAD_INEXACT) <= set(_names(cases.WGRAD))


def test_both_weight_gradient_entries_run_in_every_mode():
    """tdx_conv1_bwd_weight has no accumulate argument (it always overwrites: accumulate 0); tdx_conv1_bwd_weight_oc runs with
    0 and 1.  Every row runs all three with TDX_DETERMINISTIC unset and set (slabs in the arena); the NO_ARENA rows run all
    three again on the single-split branch, one row per route."""
    assert {(e, a) for e, _, a in ENTRIES} == {("tdx_conv1_bwd_weight", 0), ("tdx_conv1_bwd_weight_oc", 0), ("tdx_conv1_bwd_weight_oc", 1)}
    assert {tr for _, tr, _ in ENTRIES} == {0, 1}
    for c in cases.WGRAD:
        assert cases.det_plan(c.route, c.Cin, c.Cout, c.rows, cases.ARENA)[0] == "slabs"
    for n in cases.NO_ARENA:
        c = cases.by_name(cases.WGRAD, n)
        assert cases.det_plan(c.route, c.Cin, c.Cout, c.rows, 0)[0] == "single"


def test_no_comparison_may_leave_elements_out():
    a = torch.zeros(4, 4)
    _assert_equal(a, a.clone(), "all")
    _assert_within(a, a.double(), torch.ones(4, 4, dtype=torch.float64), "all")
    mask = torch.ones(4, 4, dtype=torch.bool)
    _assert_equal(a, a.clone(), "full mask", mask)
    mask[0, 0] = False
    for check in (lambda: _assert_equal(a, a.clone(), "masked", mask),
                  lambda: _assert_within(a, a.double(), torch.ones(4, 4, dtype=torch.float64), "masked", mask)):
        with pytest.raises(AssertionError, match="leaves elements out"):
            check()


@pytest.mark.parametrize("layer", cases.LAYERS, ids=lambda l: "x".join(map(str, l[:4])))
def test_layers_are_exact(layer):
    C1, C2, Cout, rows, bias = layer
    R.assert_exact(R.exact_inputs(rows, C1, C2, Cout), bias, False)


# ------------------------------------------------------------------------ the library's own answers (no GPU: nothing launches)

KIND = {"vector": "V", "h16": "H", "f32": "F"}  # _lib.CONV1_KERNELS -> the routes of conv1_cases
STATUS = {"TDX_ESHAPE": -2, "TDX_EDTYPE": -3}
DIRECT = {False: None, True: "direct"}  # TDX_CONV1_IMPL


def _code(L, dname):
    return L.dtype_code(DT[dname])


def _ask_forward(L, c, dname, w_mod16, direct):
    """tdx_conv1_fwd_plan answers what conv1_cases.fwd_route restates; the template instantiation follows from its ints"""
    q = L.conv1_fwd_plan(c.C1, c.C2, c.Cout, c.ldw, w_mod16, c.add, False, _code(L, dname))
    want = cases.fwd_route(dname, c.C1, c.C2, c.Cout, c.ldw, w_mod16 // 4, c.add, direct)  # col: w is a float pointer
    name = {"V": f"conv1_fwd_kernel<{dname}>", "H": f"conv1_mfma_fwd_kernel<{q['nt']},{dname}>",
            "F": f"conv1_f32_mfma_fwd_kernel<{q['nt']},{int(bool(c.add))}>"}[KIND[q["kernel"]]]
    assert (q["status"], KIND[q["kernel"]], name) == (0, want.route, want.kernel), (c.name, dname, q)
    assert q["tile_rows"] == cases.TILE_ROWS[want.route] and (q["nt"] == 0) == (want.route == "V")
    return want.route


def _ask_tail(L, C1, C2, Cout, dname, direct):
    """tdx_conv1_fwd_plan(gn_tail) answers what conv1_cases.gn_route restates: the kernel, or the error of tdx_conv1_fwd_gn"""
    q = L.conv1_fwd_plan(C1, C2, Cout, Cout, 0, True, True, _code(L, dname))
    want = cases.gn_route(dname, C1, C2, Cout, direct)
    if isinstance(want, str):
        assert q["status"] == STATUS[want], (C1, C2, Cout, dname, q)
    else:
        assert (q["status"], KIND[q["kernel"]], f"conv1_mfma_fwd_kernel<{q['nt']},{dname}>", q["tile_rows"]) == (0, "H", want.kernel, 256)
    return want


def _steps(q, rows):
    """the loop trips of every split, from the ints of the library's plan"""
    n, step, per = q["nsplit"], q["step_rows"], q["rows_per_split"]
    if per == 0:  # split s takes the chunks s, s + n, ...
        return tuple(cases.ceil_div(cases.ceil_div(rows, step) - s, n) for s in range(n))
    return tuple(cases.ceil_div(min(rows, (s + 1) * per) - s * per, step) for s in range(n))


def _ask_wgrad(L, c, dname, tr, direct, det, arena_bytes):
    """tdx_conv1_bwd_weight_plan answers what conv1_cases restates: wgrad_route, and plan / det_plan for the splits.  Returns
    (route, how the splits merge, steps)."""
    q = L.conv1_bwd_weight_plan(c.Cin, c.Cout, c.rows, tr, _code(L, dname))
    want = cases.wgrad_route(dname, c.Cin, c.Cout, tr, direct)
    merge, plan = cases.det_plan(want.route, c.Cin, c.Cout, c.rows, arena_bytes) if det else ("atomics", cases.plan(want.route, c.Cin, c.Cout, c.rows))
    name = {"V": f"conv1_wgrad_kernel<{dname}>", "H": f"conv1_wgrad_mfma_kernel<{q['mt']},{q['nt']},{int(tr)},{dname}>",
            "F": f"conv1_f32_mfma_wgrad_kernel<{q['nt']},{int(tr)}>"}[KIND[q["kernel"]]]
    what = (c.name, dname, tr, direct, det, arena_bytes, q)
    assert (q["status"], KIND[q["kernel"]], name) == (0, want.route, want.kernel), what
    assert (q["nsplit"], _steps(q, c.rows)) == plan, what
    assert q["nslab"] == (plan.nsplit if merge == "slabs" else 0) and (merge != "single" or plan.nsplit == 1), what
    assert q["step_rows"] == (256 if want.route == "H" else 32) and (q["rows_per_split"] == 0) == (want.route == "H"), what
    return want.route, merge, plan.steps


@pytest.mark.parametrize("arena", (True, False), ids=("arena", "no_arena"))
@pytest.mark.parametrize("det", (0, 1))
@pytest.mark.parametrize("direct", (False, True))
def test_library_routes_every_forward_and_tail_row_as_restated(direct, det, arena, monkeypatch):
    """(neither TDX_DETERMINISTIC nor the arena may move a forward route)"""
    from test_conv3_wgrad_reference import _fake_arena
    from turbdiff_amd import _lib as L

    _set_env(monkeypatch, "TDX_CONV1_IMPL", DIRECT[direct])
    _set_env(monkeypatch, "TDX_DETERMINISTIC", "1" if det else None)
    with _fake_arena(L, arena):
        _forward_and_tail_rows(L, direct)


def _forward_and_tail_rows(L, direct):
    for c in cases.FWD:
        for dname in cases.ALL:
            for mod in sorted({4 * c.col % 16, 0, 4, 8}):  # the row's own alignment of w, and others
                route = _ask_forward(L, c, dname, mod, direct)
                if dname in c.dtypes and direct == c.direct and mod == 4 * c.col % 16:
                    assert route == c.route, (c.name, dname)
    for c in cases.TAIL:
        for dname in cases.ALL:
            want = _ask_tail(L, c.C1, c.C2, c.Cout, dname, direct)
            assert (want if isinstance(want, str) else want.route) == ("TDX_EDTYPE" if dname == "f32" else "TDX_ESHAPE" if direct else "H")
    assert _ask_tail(L, 40, 0, 64, "bf16", direct) == "TDX_ESHAPE" and _ask_tail(L, 64, 0, 48, "f16", direct) == "TDX_ESHAPE"
    plan = (ctypes.c_int * L.CONV1_PLAN_INTS)()
    assert L.load().tdx_conv1_fwd_plan(32, 0, 32, 32, 0, 0, 0, L.BF16, None) == -1
    assert L.load().tdx_conv1_fwd_plan(32, 0, 32, 32, 0, 0, 0, 2, plan) == -3  # TDX_F32_SPLIT is a pack code, no tensor format


@pytest.mark.parametrize("arena", (True, False), ids=("arena", "no_arena"))
@pytest.mark.parametrize("det", (0, 1))
@pytest.mark.parametrize("direct", (False, True))
def test_library_plans_every_weight_gradient_row_as_restated(direct, det, arena, monkeypatch):
    from test_conv3_wgrad_reference import _fake_arena
    from turbdiff_amd import _lib as L

    _set_env(monkeypatch, "TDX_CONV1_IMPL", DIRECT[direct])
    _set_env(monkeypatch, "TDX_DETERMINISTIC", "1" if det else None)
    with _fake_arena(L, arena):  # 96 MiB claimed, as cases.ARENA
        for c in cases.WGRAD:
            for dname in cases.ALL:
                for tr in (0, 1):
                    route, merge, steps = _ask_wgrad(L, c, dname, tr, direct, det, cases.ARENA if arena else 0)
                    if dname not in c.dtypes or direct != c.direct:
                        continue
                    assert route == c.route and merge == ("atomics" if not det else "slabs" if arena else "single")
                    if arena or not det:
                        assert steps == c.steps
                    elif c.name in cases.NO_ARENA:
                        assert steps == cases.NO_ARENA_STEPS[c.name]
        plan = (ctypes.c_int * L.CONV1_PLAN_INTS)()
        assert L.load().tdx_conv1_bwd_weight_plan(32, 32, 1, 0, L.BF16, None) == -1
        assert L.load().tdx_conv1_bwd_weight_plan(32, 32, 0, 0, L.BF16, plan) == -1
        assert L.load().tdx_conv1_bwd_weight_plan(32, 32, 1, 0, 2, plan) == -3


# ---------------------------------------------------------------------------------------------------------------- on the GPU


def _dev():
    return torch.device("cuda:0")


def _to(p, d):
    return {k: (None if v is None else v.to(d)) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _exact(rows, C1, C2, Cout, narrow=False):
    return _to(R.exact_inputs(rows, C1, C2, Cout, narrow=narrow), _dev())


def _set_env(monkeypatch, name, value):
    if value:
        monkeypatch.setenv(name, value)
    else:
        monkeypatch.delenv(name, raising=False)


def _set_deterministic(monkeypatch, det):
    from turbdiff_amd import _lib as L

    _set_env(monkeypatch, "TDX_DETERMINISTIC", "1" if det else None)
    assert L.deterministic() == bool(det)


def _as(t, dt):
    return None if t is None else t.to(dt).contiguous()


def _forward(L, c, p, dt, bias, add, ask=True):
    """tdx_conv1_fwd into a buffer with a sentinel margin; the weight block sits at column c.col of a (Cin, ldw) matrix whose
    other columns hold 3.0 (a kernel that strays into them misses the reference).  ask: the library's own route for this very
    call, pointer included, must be the row's (False: a library from before the query, as the recorder of the pinned bits runs)."""
    d = _dev()
    wm = torch.full((c.C1 + c.C2, c.ldw), 3.0, device=d)
    wm[:, c.col:c.col + c.Cout] = p["w"]
    buf = torch.full((c.rows * c.Cout + MARGIN,), SENTINEL, dtype=dt, device=d)
    x1, x2 = _as(p["x1"], dt), _as(p["x2"], dt)
    if ask:
        assert bool(c.add) == (add is not None)
        assert _ask_forward(L, c, DNAME[dt], (L.ptr(wm) + 4 * c.col) % 16, c.direct) == c.route
    L.call("tdx_conv1_fwd", L.ptr(x1), c.C1, L.ptr(x2), c.C2, L.ptr(wm) + 4 * c.col, c.ldw, L.ptr(bias), L.ptr(_as(add, dt)),
           L.ptr(buf), c.rows, c.Cout, L.dtype_code(dt), L.stream())
    assert bool((buf[c.rows * c.Cout:] == SENTINEL).all()), "the margin behind y was written"
    return buf[: c.rows * c.Cout].view(c.rows, c.Cout)


def _w_as_read(route, w, dt):
    return w.to(dt) if route == "H" else w


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.FWD, ids=_names(cases.FWD))
def test_forward_on_exact_inputs_is_the_reference_rounded_as_its_route_rounds(case, monkeypatch):
    from turbdiff_amd import _lib as L

    c = case
    _set_env(monkeypatch, "TDX_CONV1_IMPL", "direct" if c.direct else None)
    for narrow in ((False, True) if c.add else (False,)):
        p = _exact(c.rows, c.C1, c.C2, c.Cout, narrow)
        bias, add = (p["bias"] if c.bias else None), (p["add"] if c.add else None)
        y0, _ = R.forward(p["x1"], p["x2"], p["w"], bias, None)
        for name in c.dtypes:
            dt = DT[name]
            assert cases.fwd_route(name, c.C1, c.C2, c.Cout, c.ldw, c.col, c.add, c.direct).route == c.route
            assert torch.equal(p["w"].to(dt).float(), p["w"])  # H's staging rounds nothing away
            got = _forward(L, c, p, dt, bias, add)
            _assert_equal(got, R.rounded(c.route, y0, add, dt), f"{c.name} {name} narrow={narrow}")


@pytest.mark.gpu
@pytest.mark.parametrize("dname", cases.H16)
def test_one_set_of_tensors_rounds_once_on_the_vector_kernel_and_twice_on_the_mfma_kernel(dname, monkeypatch):
    """The same x1, x2, w, bias and add through conv1_fwd_kernel<T> (TDX_CONV1_IMPL=direct) and through conv1_mfma_fwd_kernel:
    each equals its own rounding form, and the two outputs differ."""
    from turbdiff_amd import _lib as L

    v, h = (cases.by_name(cases.FWD, n) for n in cases.SAME_INPUTS)
    dt = DT[dname]
    p = _exact(v.rows, v.C1, v.C2, v.Cout)
    y0, _ = R.forward(p["x1"], p["x2"], p["w"], p["bias"], None)
    got = {}
    for c in (v, h):
        _set_env(monkeypatch, "TDX_CONV1_IMPL", "direct" if c.direct else None)
        assert cases.fwd_route(dname, c.C1, c.C2, c.Cout, c.ldw, c.col, c.add, c.direct).route == c.route
        got[c.route] = _forward(L, c, p, dt, p["bias"], p["add"])
    _assert_equal(got["V"], R.rounded_once(y0, p["add"], dt), f"{dname} vector-ALU kernel: one rounding")
    _assert_equal(got["H"], R.rounded_twice(y0, p["add"], dt), f"{dname} MFMA kernel: two roundings")
    assert not torch.equal(got["V"], got["H"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.FWD_INEXACT)
def test_forward_on_gaussian_inputs_within_the_derived_bound(name, monkeypatch):
    from turbdiff_amd import _lib as L

    c = cases.by_name(cases.FWD, name)
    _set_env(monkeypatch, "TDX_CONV1_IMPL", "direct" if c.direct else None)
    for dname in c.dtypes:
        dt = DT[dname]
        p = _to(R.gaussian_inputs(c.rows, c.C1, c.C2, c.Cout, dt), _dev())
        bias, add = (p["bias"] if c.bias else None), (p["add"] if c.add else None)
        w = _w_as_read(c.route, p["w"], dt)
        y0, y = R.forward(p["x1"], p["x2"], w, bias, add)
        got = _forward(L, c, p, dt, bias, add)
        _assert_within(got, y, R.forward_bound(c.route, p["x1"], p["x2"], w, bias, add, y0, y, dt), f"{c.name} {dname}")


@pytest.mark.gpu
@pytest.mark.parametrize("dname", cases.ALL)
@pytest.mark.parametrize("layer", cases.LAYERS, ids=lambda l: "x".join(map(str, l[:4])))
def test_layer_through_autograd_is_exact(layer, dname, monkeypatch):
    """ops.conv1 and its backward: y, gx1, gx2, dW in the parameter's (Cout, Cin) layout (two column blocks for two inputs),
    dbias; TDX_DETERMINISTIC set and unset give the same bits."""
    from turbdiff_amd import ops

    C1, C2, Cout, rows, has_bias = layer
    dt = DT[dname]
    p = _exact(rows, C1, C2, Cout)
    bias = p["bias"] if has_bias else None
    from turbdiff_amd import _lib as L

    fr = cases.fwd_route(dname, C1, C2, Cout, Cout, 0, False).route
    assert _ask_forward(L, cases._fwd(str(layer), fr, (dname,), C1, C2, Cout, rows, has_bias, False, "ops.conv1"), dname, 0, False) == fr
    y0, _ = R.forward(p["x1"], p["x2"], p["w"], bias, None)
    w2 = p["w"].t().contiguous()
    dW, db = R.wgrad(R._cat(p["x1"], p["x2"]), p["dy"])
    want = dict(y=R.rounded(fr, y0, None, dt), gw=dW.t().float().contiguous(), gb=db.float() if has_bias else None)
    for key, col, C in (("gx1", 0, C1), ("gx2", C1, C2)):
        want[key] = R.rounded("V", R.forward(p["dy"], None, R.weight_block(w2, col, C), None, None)[0], None, dt) if C else None
    for det in (0, 1):
        _set_deterministic(monkeypatch, det)
        x1 = p["x1"].detach().to(dt).clone().requires_grad_()
        x2 = p["x2"].detach().to(dt).clone().requires_grad_() if C2 else None
        wp = w2.clone().reshape(Cout, C1 + C2, 1, 1, 1).requires_grad_()
        bp = bias.detach().clone().requires_grad_() if has_bias else None
        y = ops.conv1(x1, wp, bp, x2)
        y.backward(p["dy"].to(dt))
        got = dict(y=y.detach(), gx1=x1.grad, gx2=x2.grad if C2 else None, gw=wp.grad.reshape(Cout, -1), gb=bp.grad if has_bias else None)
        for key, w_ in want.items():
            if w_ is not None:
                _assert_equal(got[key].contiguous(), w_, f"{layer} {dname} deterministic={det} {key}")


# ---- the fused tail


def _tail_calls(L, c, p, t, dt):
    """(fused, two launches): tdx_conv1_fwd_gn, and tdx_conv1_fwd into a temporary + tdx_gn_apply(act = 1) with that residual"""
    d = _dev()
    rows = c.B * c.V
    x1, x2, h = _as(p["x1"], dt), _as(p["x2"], dt), _as(t["h"], dt)
    buf = torch.full((rows * c.Cout + MARGIN,), SENTINEL, dtype=dt, device=d)
    code, st = L.dtype_code(dt), L.stream()
    L.call("tdx_conv1_fwd_gn", L.ptr(x1), c.C1, L.ptr(x2), c.C2, L.ptr(p["w"]), c.Cout, L.ptr(p["bias"]), L.ptr(h), L.ptr(t["stats"]),
           L.ptr(t["gamma"]), L.ptr(t["beta"]), c.G, L.ptr(buf), c.B, c.V, c.Cout, code, st)
    assert bool((buf[rows * c.Cout:] == SENTINEL).all()), "the margin behind y was written"
    res, y2 = torch.empty(rows, c.Cout, dtype=dt, device=d), torch.empty(c.B, c.V, c.Cout, dtype=dt, device=d)
    L.call("tdx_conv1_fwd", L.ptr(x1), c.C1, L.ptr(x2), c.C2, L.ptr(p["w"]), c.Cout, L.ptr(p["bias"]), None, L.ptr(res), rows, c.Cout, code, st)
    L.call("tdx_gn_apply", L.ptr(h), L.ptr(t["stats"]), L.ptr(t["gamma"]), L.ptr(t["beta"]), None, None, L.ptr(res), L.ptr(y2),
           c.B, c.V, c.Cout, c.G, 1, code, st)
    return buf[: rows * c.Cout].view(c.B, c.V, c.Cout), y2, res


@pytest.mark.gpu
@pytest.mark.parametrize("dname", cases.H16)
@pytest.mark.parametrize("case", cases.TAIL, ids=_names(cases.TAIL))
def test_fused_tail_on_exact_inputs(case, dname):
    """Exact conv inputs and dyadic GroupNorm inputs: y0 = round_T(acc + bias) and n are exact, so the fused kernel may be off
    by silu_f's own error, one float32 addition and the store; the two-launch form computes the same silu_f(n) and adds it to
    the same y0: conv1_reference.tail_two_launch_bound."""
    from turbdiff_amd import _lib as L

    c, dt = case, DT[dname]
    assert cases.gn_route(dname, c.C1, c.C2, c.Cout).route == "H"
    rows = c.B * c.V
    p = _exact(rows, c.C1, c.C2, c.Cout)
    t = _to(R.tail_inputs(c.B, c.V, c.Cout, c.G), _dev())
    y0 = R.rounded_twice(R.forward(p["x1"], p["x2"], p["w"], p["bias"], None)[0], None, dt).double().view(c.B, c.V, c.Cout)
    n, s = R.tail(t["h"], t["stats"], t["gamma"], t["beta"], c.G)
    assert n.abs().max().item() <= R.N_MAX and torch.equal(n.float().double(), n)
    y = y0 + s
    assert _ask_tail(L, c.C1, c.C2, c.Cout, dname, False).route == "H"
    fused, two, res = _tail_calls(L, c, p, t, dt)
    _assert_equal(res, y0.to(dt).view(rows, c.Cout), f"{c.name} {dname}: the two-launch form's residual")
    _assert_within(fused, y, R.tail_bound(t["h"], t["stats"], t["gamma"], t["beta"], n, 0.0, y0, y, dt), f"{c.name} {dname} fused")
    _assert_within(fused, two.double(), R.tail_two_launch_bound(s, y, dt), f"{c.name} {dname} fused against two launches")


@pytest.mark.gpu
@pytest.mark.parametrize("dname", cases.H16)
@pytest.mark.parametrize("name", cases.TAIL_INEXACT)
def test_fused_tail_on_gaussian_inputs_within_the_derived_bound(name, dname):
    from turbdiff_amd import _lib as L

    c, dt = cases.by_name(cases.TAIL, name), DT[dname]
    rows = c.B * c.V
    p = _to(R.gaussian_inputs(rows, c.C1, c.C2, c.Cout, dt), _dev())
    t = _to(R.tail_inputs(c.B, c.V, c.Cout, c.G, exact=False, dt=dt), _dev())
    w = p["w"].to(dt)
    y0, _ = R.forward(p["x1"], p["x2"], w, p["bias"], None)
    y0_bound = R.forward_bound("H", p["x1"], p["x2"], w, p["bias"], None, y0, y0, dt).view(c.B, c.V, c.Cout)
    y0 = y0.view(c.B, c.V, c.Cout)
    n, s = R.tail(t["h"], t["stats"], t["gamma"], t["beta"], c.G)
    assert n.abs().max().item() <= R.N_MAX
    y = y0 + s
    assert _ask_tail(L, c.C1, c.C2, c.Cout, dname, False).route == "H"
    fused, _, _ = _tail_calls(L, c, p, t, dt)
    _assert_within(fused, y, R.tail_bound(t["h"], t["stats"], t["gamma"], t["beta"], n, y0_bound, y0, y, dt), f"{c.name} {dname}")


@pytest.mark.gpu
def test_fused_tail_refuses_fp32_and_ineligible_shapes(monkeypatch):
    from turbdiff_amd import _lib as L

    d = _dev()
    B, V, G_ = 2, 10, 4
    for dname, C1, Cout, direct, want in (("f32", 64, 64, False, -3), ("bf16", 40, 64, False, -2), ("f16", 64, 48, False, -2),
                                          ("bf16", 64, 64, True, -2)):
        dt = DT[dname]
        assert cases.gn_route(dname, C1, 0, Cout, direct) == {-3: "TDX_EDTYPE", -2: "TDX_ESHAPE"}[want]
        _set_env(monkeypatch, "TDX_CONV1_IMPL", "direct" if direct else None)
        assert STATUS[_ask_tail(L, C1, 0, Cout, dname, direct)] == want
        x, h = torch.zeros(B, V, C1, dtype=dt, device=d), torch.zeros(B, V, Cout, dtype=dt, device=d)
        w, bias, stats = torch.zeros(C1, Cout, device=d), torch.zeros(Cout, device=d), torch.ones(B, G_, 2, device=d)
        y = torch.full((B, V, Cout), SENTINEL, dtype=dt, device=d)
        rc = L.load().tdx_conv1_fwd_gn(L.ptr(x), C1, None, 0, L.ptr(w), Cout, L.ptr(bias), L.ptr(h), L.ptr(stats), L.ptr(bias), L.ptr(bias),
                                       G_, L.ptr(y), B, V, Cout, L.dtype_code(dt), L.stream())
        assert rc == want and bool((y == SENTINEL).all())


# ---- the weight gradient

ENTRIES = [("tdx_conv1_bwd_weight", 0, 0), ("tdx_conv1_bwd_weight_oc", 1, 0), ("tdx_conv1_bwd_weight_oc", 1, 1)]  # entry, transposed, accumulate


def _wgrad_call(L, entry, tr, acc, x, dy, Cin, Cout, rows, dt, pre_w, pre_b):
    """One call into a block at column OFF of a copy of pre_w (PAD_R rows and OFF + PAD_C columns larger than the result) and
    the head of a copy of pre_b (8 longer than Cout), or no bias gradient (pre_b None).  Returns the whole buffers."""
    bw = pre_w.clone()
    bb = None if pre_b is None else pre_b.clone()
    ldw = bw.shape[1]
    args = [L.ptr(x), Cin, L.ptr(dy), Cout, bw.data_ptr() + 4 * OFF, ldw, L.ptr(bb)]
    if entry.endswith("_oc"):
        args.append(acc)
    L.call(entry, *args, rows, L.dtype_code(dt), L.stream())
    return bw, bb


def _wgrad_expected(tr, acc, dW, db, pre_w, pre_b):
    """what the buffers must hold: the block overwritten or added to, every other element as it was"""
    blk = dW.t() if tr else dW
    ew = pre_w.double().clone()
    view = ew[: blk.shape[0], OFF:OFF + blk.shape[1]]
    view.copy_(view + blk if acc else blk)
    eb = None
    if pre_b is not None:
        eb = pre_b.double().clone()
        eb[: db.numel()] = eb[: db.numel()] + db if acc else db
    return ew, eb


def _prefills(Cin, Cout, tr, exact=True):
    nrow, ncol = (Cout, Cin) if tr else (Cin, Cout)
    d = _dev()
    return R.prefill((nrow + PAD_R, OFF + ncol + PAD_C), tr, exact).to(d), R.prefill((Cout + 8,), 2 + tr, exact).to(d)


def _ask_wgrad_row(L, c, dname, tr, det):
    """the library's own plan for the call about to be made on this stream, with the arena that call will see: the row's route,
    its way of merging and its steps"""
    L.ensure_scratch()
    route, merge, steps = _ask_wgrad(L, c, dname, tr, c.direct, det, L.SCRATCH_BYTES)
    assert (route, merge) == (c.route, "atomics" if not det else "slabs" if L.SCRATCH_BYTES else "single")
    assert steps == (cases.NO_ARENA_STEPS[c.name] if merge == "single" else c.steps)


def _run_exact_wgrad(L, c, monkeypatch, dets):
    p = _exact(c.rows, c.Cin, 0, c.Cout)
    dW, db = R.wgrad(p["x1"], p["dy"])
    _set_env(monkeypatch, "TDX_CONV1_IMPL", "direct" if c.direct else None)
    for dname in c.dtypes:
        dt = DT[dname]
        x, dy = _as(p["x1"], dt), _as(p["dy"], dt)
        for entry, tr, acc in ENTRIES:
            assert cases.wgrad_route(dname, c.Cin, c.Cout, tr, c.direct).route == c.route
            pre_w, pre_b = _prefills(c.Cin, c.Cout, tr)
            for with_bias in (True, False):
                ew, eb = _wgrad_expected(tr, acc, dW, db, pre_w, pre_b if with_bias else None)
                for det in dets:
                    _set_deterministic(monkeypatch, det)
                    _ask_wgrad_row(L, c, dname, tr, det)
                    bw, bb = _wgrad_call(L, entry, tr, acc, x, dy, c.Cin, c.Cout, c.rows, dt, pre_w, pre_b if with_bias else None)
                    what = f"{c.name} {dname} {entry} accumulate={acc} dbias={with_bias} deterministic={det}"
                    _assert_equal(bw, ew.float(), what + ": dW and the buffer around it")
                    if with_bias:
                        _assert_equal(bb, eb.float(), what + ": dbias and the elements behind it")


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.WGRAD, ids=_names(cases.WGRAD))
def test_weight_gradient_on_exact_inputs_is_the_reference(case, monkeypatch):
    """Both entries, accumulate 0 and 1 onto a non-zero integer prefill, with and without dbias, TDX_DETERMINISTIC unset and set
    (slabs in the arena): the block is THE integer sum (hence the two modes bit-equal), and every element of the larger buffer
    outside the block -- the columns past ncol, the columns before the block, the rows past nrow -- is what it was."""
    from turbdiff_amd import _lib as L

    c = case
    assert cases.det_plan(c.route, c.Cin, c.Cout, c.rows, L.SCRATCH_BYTES)[0] == "slabs"  # the slabs and their ordered sum really run
    _run_exact_wgrad(L, c, monkeypatch, (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NO_ARENA)
def test_weight_gradient_without_an_arena_takes_one_split(name, monkeypatch):
    """TDX_DETERMINISTIC with no scratch arena bound (TDX_SCRATCH_MB=0): max_split = 1, one contributor per element adds
    straight into the zeroed or accumulated block; the vector kernel's row block is re-sized to hold all rows."""
    from turbdiff_amd import _lib as L

    c = cases.by_name(cases.WGRAD, name)
    old = L.SCRATCH_BYTES
    try:
        L.SCRATCH_BYTES, L._ACTIVE = 0, None  # the next arena user binds "no arena"
        assert cases.det_plan(c.route, c.Cin, c.Cout, c.rows, L.SCRATCH_BYTES) == ("single", cases.Plan(1, cases.NO_ARENA_STEPS[name]))
        _run_exact_wgrad(L, c, monkeypatch, (1,))
        assert L._ACTIVE is not None  # the calls went through a binding, and it was "no arena"
    finally:
        L.SCRATCH_BYTES, L._ACTIVE = old, None  # and the next one gets its stream's arena back
    L.ensure_scratch()
    assert (L.scratch_arena() is not None) == (old > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.WGRAD_INEXACT)
def test_weight_gradient_on_gaussian_inputs_within_the_derived_bound(name, monkeypatch):
    """Every element within gamma_rows sum |x dy|, or gamma_(rows + 1) (sum |x dy| + |prefill|) with accumulate, the prefill
    being the element accumulated onto; two deterministic runs give the same bits."""
    from turbdiff_amd import _lib as L

    c = cases.by_name(cases.WGRAD, name)
    for dname in c.dtypes:
        dt = DT[dname]
        p = _to(R.gaussian_inputs(c.rows, c.Cin, 0, c.Cout, dt), _dev())
        x, dy = _as(p["x1"], dt), _as(p["dy"], dt)
        dW, db = R.wgrad(p["x1"], p["dy"])
        for entry, tr, acc in ENTRIES:
            pre_w, pre_b = _prefills(c.Cin, c.Cout, tr, exact=False)
            ew, eb = _wgrad_expected(tr, acc, dW, db, pre_w, pre_b)
            onto = pre_w[: ew.shape[0] - PAD_R, OFF:ew.shape[1] - PAD_C]  # the block accumulated onto, as the entry lays it out
            bW, bB = R.wgrad_bound(p["x1"], p["dy"], onto.t() if tr else onto, pre_b[: c.Cout]) if acc else R.wgrad_bound(p["x1"], p["dy"])
            bound_w = torch.zeros_like(ew)  # 0 outside the block: those elements must be untouched
            blk = bW.t() if tr else bW
            bound_w[: blk.shape[0], OFF:OFF + blk.shape[1]] = blk
            bound_b = torch.zeros_like(eb)
            bound_b[: c.Cout] = bB
            runs = []
            for det in (0, 1, 1):
                _set_deterministic(monkeypatch, det)
                _ask_wgrad_row(L, c, dname, tr, det)
                bw, bb = _wgrad_call(L, entry, tr, acc, x, dy, c.Cin, c.Cout, c.rows, dt, pre_w, pre_b)
                what = f"{c.name} {dname} {entry} accumulate={acc} deterministic={det}"
                _assert_within(bw, ew, bound_w, what + " dW")
                _assert_within(bb, eb, bound_b, what + " dbias")
                runs.append((bw, bb))
            _assert_equal(runs[1][0], runs[2][0], f"{c.name} {dname} {entry}: dW of two deterministic runs")
            _assert_equal(runs[1][1], runs[2][1], f"{c.name} {dname} {entry}: dbias of two deterministic runs")
