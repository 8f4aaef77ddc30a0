"""The seven weight-gradient kernels of the 3x3x3 convolution (tdx_conv3_bwd_weight: csrc/tdx_conv3_direct.hip and tdx_conv3_wgrad_*.hip)
against the float64 reference of tests/conv3_wgrad_reference.py, element by element, on every row of tests/conv3_wgrad_cases.py.
On the exact inputs the reference cast to float32 is THE answer (torch.equal, whatever the kernel, the K split and the merge);
on Gaussian inputs every element is held to a bound derived in the docstring of conv3_wgrad_reference.py.  No tolerance is a
measured number and no element is left out.  Every row names the kernel it is for, and the library's plan query
(tdx_conv3_bwd_weight_plan: the host function the launch itself uses) is asked before each launch that this kernel runs.

Without a GPU: the reference against float64 F.conv3d over F.pad(mode="replicate") and its autograd; the exactness
preconditions of every exact row; every row's plan against the restated host rules of conv3_wgrad_cases and against the
library, with an arena bound and without one; the plan of the shipped model's layers (a pin of current behaviour); what the table
reaches; and planted defects of the reference, each of which the exact inputs must be able to see.
"""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import conv3_wgrad_cases as cases
import conv3_wgrad_reference as R

DT = R.DTYPES
MARGIN = 1024     # floats behind dW
SENTINEL = -768.0
IMPL_NAMES = {cases.AUTO: None, cases.DIRECT: "direct", cases.MFMA: "mfma", cases.SPLIT: "split"}
CASE_IDS = [c.name for c in cases.CASES]


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
    ok = err <= bound  # a NaN (an unwritten element) is not within any bound
    if not bool(ok.all()):
        i = int(torch.where(ok, torch.zeros_like(err), err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).argmax())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside their bound, worst at flat index {i}: "
                             f"got {got.flatten()[i].item()!r}, reference {ref.flatten()[i].item()!r}, "
                             f"bound {bound.flatten()[i].item():.3e}")


# ------------------------------------------------------------------------------------------------------------ without a GPU


@pytest.mark.parametrize("B,grid,C1,C2,Cout", [(2, (3, 4, 5), 3, 0, 2), (1, (1, 2, 6), 2, 3, 4), (2, (5, 1, 1), 4, 0, 3), (1, (2, 2, 2), 1, 1, 1)])
def test_reference_is_conv3d_over_replicate_padding_and_its_autograd(B, grid, C1, C2, Cout):
    """Integer inputs in float64: both sides are exact, so the comparison is torch.equal"""
    g = torch.Generator().manual_seed(1)
    ri = lambda *s: torch.randint(-9, 10, s, generator=g).double()
    x1, x2, dy = ri(B, *grid, C1), (ri(B, *grid, C2) if C2 else None), ri(B, *grid, Cout)
    w = torch.zeros(Cout, C1 + C2, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    xc = R._cat(x1, x2).permute(0, 4, 1, 2, 3)
    F.conv3d(F.pad(xc, (1,) * 6, mode="replicate"), w, b).backward(dy.permute(0, 4, 1, 2, 3))
    dW, db = R.wgrad(x1, x2, dy)
    assert dW.dtype == torch.float64 and torch.equal(dW, w.grad) and torch.equal(db, b.grad)
    # the planted forms are what they say: zero padding is F.conv3d(padding=1)
    wz = torch.zeros_like(w).requires_grad_()
    F.conv3d(xc, wz, None, padding=1).backward(dy.permute(0, 4, 1, 2, 3))
    assert torch.equal(R.wgrad(x1, x2, dy, zero_pad=True)[0], wz.grad)


@pytest.mark.parametrize("case", cases.CASES, ids=CASE_IDS)
def test_exact_rows_meet_their_preconditions(case):
    c = case
    rows = c.B * c.grid[0] * c.grid[1] * c.grid[2]
    assert rows <= 20000 and 27 * rows * (c.C1 + c.C2) * c.Cout <= 3e9, "a row stays small"
    for fam in R.FAMILIES:
        dtypes = tuple(d for d in c.dtypes if fam in cases.families(d))  # the storage formats that run this family
        assert dtypes or fam != "ints"
        if dtypes:
            R.assert_exact(R.exact_inputs(c.B, c.grid, c.C1, c.C2, c.Cout, fam), fam, dtypes)


def test_assert_exact_refuses_what_is_not_exact():
    p = R.exact_inputs(1, (3, 3, 3), 8, 0, 8, "wide-x")
    with pytest.raises(AssertionError):
        R.assert_exact(p, "wide-x", ("f32", "bf16"))  # 10 significant bits do not survive bf16
    q = dict(p, dy=R.exact_inputs(1, (3, 3, 3), 8, 0, 8, "wide-dy")["dy"])
    with pytest.raises(AssertionError, match="lo x lo"):
        R.assert_exact(q, "wide-x", ("f32",))
    big = {k: (None if v is None else v * 2.0**12) for k, v in R.exact_inputs(2, (9, 9, 9), 8, 0, 8, "ints").items()}
    with pytest.raises(AssertionError, match="2\\^24"):
        R.assert_exact(big, "ints", ("f32",))


def _clear_switches(monkeypatch):
    from turbdiff_amd import _lib as L

    for v in L.switch_names() + ("TDX_CONV_IMPL",):  # the library's own list, and the Python-side override
        monkeypatch.delenv(v, raising=False)


def _set_case_env(monkeypatch, c):
    _clear_switches(monkeypatch)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)


def _expected(c):
    return (c.kernel, c.tile, c.depth, c.nsplit, c.nslab, c.sum_unpack)


def _plan_key(p):
    return (p["kernel"], p["tile"], p["depth"], p["nsplit"], p["nslab"], p["sum_unpack"])


def _assert_plan(L, c, dname, arena):
    """the library's plan for the row as the environment and the arena are now = the restated rules; with the row's own arena
    setting also what the row names"""
    got = L.conv3_bwd_weight_plan(c.C1, c.C2, c.Cout, c.B, *c.grid, cases.CODE[dname], c.impl)
    assert got == cases.case_plan(c, dname, arena)._asdict(), (c.name, dname, arena)
    assert got == L.conv3_bwd_weight_plan(c.C1, c.C2, c.Cout, c.B, *c.grid, cases.CODE[dname], c.impl | L.WS_CLEAN)
    if arena == c.arena:
        assert got["status"] == cases.OK and _plan_key(got) == _expected(c), (c.name, dname, got)
    return got


class _fake_arena:
    """tdx_set_scratch only stores the pointer and the plan query only asks whether one is bound: a host buffer with a claimed
    size stands in for the arena.  Nothing is launched inside."""

    def __init__(self, L, bound):
        self.L, self.bound = L, bound
        self.buf = ctypes.create_string_buffer(256)

    def __enter__(self):
        assert self.L.load().tdx_set_scratch(ctypes.addressof(self.buf) if self.bound else None, (96 << 20) if self.bound else 0) == 0

    def __exit__(self, *exc):
        self.L.load().tdx_set_scratch(None, 0)
        self.L._ACTIVE = None  # a later GPU test in this process binds its real arena again


@pytest.mark.parametrize("case", cases.CASES, ids=CASE_IDS)
def test_rows_take_their_kernel_and_plan(case, monkeypatch):
    from turbdiff_amd import _lib as L

    _set_case_env(monkeypatch, case)
    for arena in (True, False):
        with _fake_arena(L, arena):
            for dname in case.dtypes:
                _assert_plan(L, case, dname, arena)


def test_plan_query_reports_the_status_of_refused_calls(monkeypatch):
    from turbdiff_amd import _lib as L

    _clear_switches(monkeypatch)
    q = lambda C1, C2, Co, dt, impl, grid=(4, 4, 4), B=1: L.conv3_bwd_weight_plan(C1, C2, Co, B, *grid, dt, impl)
    assert q(4, 0, 64, L.BF16, L.CONV_AUTO)["status"] == cases.ESHAPE          # C % 8
    assert q(32, 0, 32, L.F32, L.CONV_MFMA)["status"] == cases.OK               # fp32 tensors: the fp32-IEEE kernel
    assert q(8, 0, 40, L.F32, L.CONV_MFMA)["status"] == cases.EDTYPE            # no fp32 MFMA shape: TDX_CONV_MFMA means 16-bit
    assert q(8, 0, 40, L.BF16, L.CONV_MFMA)["status"] == cases.ESHAPE
    assert q(32, 0, 32, L.BF16, L.CONV_AUTO, B=0)["status"] == cases.EINVAL
    assert q(32, 0, 32, L.BF16, L.CONV_AUTO, grid=(4, 0, 4))["status"] == cases.EINVAL
    assert L.load().tdx_conv3_bwd_weight_plan(32, 0, 32, 1, 4, 4, 4, L.BF16, L.CONV_AUTO, None) == cases.EINVAL
    # a dtype code that is no tensor format (2 is TDX_F32_SPLIT, a pack code): every impl ends at the vector ALU's dispatch or at
    # the 16-bit check, TDX_EDTYPE; a channel count off 8 is refused first, as in the call
    for unknown in (L.F32_SPLIT, 4, -1):
        for impl in (L.CONV_AUTO, L.CONV_DIRECT, L.CONV_MFMA, L.CONV_SPLIT):
            for C1, Co in ((32, 32), (8, 40)):
                assert q(C1, 0, Co, unknown, impl) == cases.plan("?", impl, C1, 0, Co, 1, (4, 4, 4))._asdict()
                assert q(C1, 0, Co, unknown, impl)["status"] == cases.EDTYPE, (unknown, impl, C1)
        assert q(4, 0, 64, unknown, L.CONV_AUTO)["status"] == cases.ESHAPE
    for args in ((4, 0, 64, "bf16", cases.AUTO), (8, 0, 40, "f32", cases.MFMA), (8, 0, 40, "bf16", cases.MFMA)):
        C1, C2, Co, dname, impl = args
        assert q(C1, C2, Co, cases.CODE[dname], impl) == cases.plan(dname, impl, C1, C2, Co, 1, (4, 4, 4))._asdict()


def test_plan_of_the_shipped_layers_is_pinned(monkeypatch):
    """The plan of every 3x3x3 layer of the shipped model in each dtype / impl mode, without an arena and with one, as the
    library of the change that added the query gave it.  This freezes current behaviour -- it is not a comparison with a
    reference: a deliberate change of a planning rule updates cases.PIN."""
    from turbdiff_amd import _lib as L

    import test_abi_and_host as A

    assert list(cases.PIN) == [row[0] for row in A._CONV3_ROUTES], "the pin covers the shapes of the forward's routing pin, in its order"
    _clear_switches(monkeypatch)
    for column, arena in enumerate((False, True)):
        with _fake_arena(L, arena):
            for shape in cases.PIN:
                got = [cases.pin_word(L.conv3_bwd_weight_plan(*shape, cases.CODE[d], impl)) for d, impl in cases.PIN_MODES]
                assert got == cases.PIN[shape][column].split(), (shape, arena)
                for (d, impl), word in zip(cases.PIN_MODES, got):  # and the restated rules agree on these shapes too
                    assert cases.pin_word(cases.plan(d, impl, *shape[:4], shape[4:], None, arena)._asdict()) == word, (shape, d, impl)


def test_table_reaches_its_edges():
    C = cases.CASES
    of = lambda k: [c for c in C if c.kernel == k]
    rows = lambda c: c.B * c.grid[0] * c.grid[1] * c.grid[2]
    nb = lambda c, bx=4: c.B * cases.view(c.grid, bx)[1]
    ragged = lambda c, bx=4: any(e % b for e, b in zip((c.grid[p] for p in cases.PERMS[cases.view(c.grid, bx)[0]]), (bx, 8, 8)))
    assert {c.kernel for c in C} == set(cases.KERNELS)
    # ---- brick16
    b = of("brick16")
    assert {(d, c.tile) for c in b for d in c.dtypes} == {(d, t) for d in cases.H16 for t in (1, 2)}
    by_switch = [c for c in b if c.env.get("TDX_WGRAD_RING") == "0" and c.env.get("TDX_WGRAD_SMALL_ROWS") == "0"]
    assert any(c.C1 + c.C2 >= 128 for c in by_switch)  # ring and small refused through their switches on a shape they would take
    assert cases.case_plan(cases.by_name("b16_prefetch_256")._replace(env={}), "bf16").kernel == "small"
    by_shape = [c for c in b if not c.env and c.arena]
    assert any(c.C1 + c.C2 < 128 and nb(c) < 4 for c in by_shape)
    assert any(c.B == 1 and c.grid == (4, 8, 8) for c in b) and any(c.grid == (5, 9, 9) for c in b)
    assert {cases.view(c.grid, 4)[0] for c in b if c.env.get("TDX_CONV3_PERM") != "0"} == {0, 1, 2}
    off = [c for c in b if c.env.get("TDX_CONV3_PERM") == "0"]
    assert off and all(cases.view(c.grid, 4)[0] != 0 for c in off)  # the switch changes the bricks of its row
    assert any((c.C1, c.C2) == (16, 0) for c in b) and any(c.C1 == 32 and c.C2 == 32 for c in b) and any(c.Cout == 96 for c in b)
    assert any(nb(c) >= 2 * c.nsplit and (c.C1, c.Cout) == (256, 256) for c in b)  # a workgroup walks >= 2 bricks: the prefetch
    assert any(1 in c.grid for c in b) and any(2 in c.grid for c in b)
    # ---- small
    s = of("small")
    geom = lambda c: cases.small_geom(c.C1, c.C2, c.Cout, c.B, c.grid, {**cases.ENV, **cases.case_env(c)})
    assert {(d, c.tile) for c in s for d in c.dtypes} == {(d, t) for d in cases.H16 for t in (1, 2)}
    assert any(geom(c)[0] > 1 and c.B % geom(c)[0] for c in s) and any(geom(c)[0] == 1 and geom(c)[2] == 1 for c in s)
    assert any(geom(c)[2] > 1 and c.grid[0] % geom(c)[1] for c in s)  # x slabs, the last one ragged
    assert any((geom(c)[0] * geom(c)[1] * c.grid[1] * c.grid[2]) % 16 for c in s) and any(geom(c)[4] for c in s)
    assert any(c.C2 for c in s) and any(c.sum_unpack for c in s)
    # ---- ring
    r = of("ring")
    assert {(d, c.tile) for c in r for d in c.dtypes} == {(d, t) for d in cases.H16 for t in (1, 2)}
    assert all(c.arena for c in r)
    assert any(not c.env for c in r) and any(c.env == cases.CUS8 for c in r)  # both branches of the split rule
    assert all(nb(c) >= 4 * c.nsplit for c in r) and any(nb(c) == 4 * c.nsplit for c in r)
    assert any(ragged(c) for c in r) and any(not ragged(c) for c in r)
    assert any((c.C1, c.C2) == (16, 0) for c in r) and any(c.C2 for c in r)
    short = cases.by_name("ring_one_brick_short")
    assert short.kernel == "brick16" and nb(short) == 4 * 8 - 1 and short.env == cases.CUS8
    assert cases.case_plan(short._replace(B=short.B + 1), "bf16").kernel == "ring"
    bare = cases.by_name("ring_without_arena")
    assert bare.kernel == "brick16" and not bare.arena and cases.case_plan(bare, "bf16", arena=True).kernel == "ring"
    # ---- fp32 routes
    f = of("brick_f32")
    assert {(c.tile, c.depth) for c in f} == {(1, 4), (2, 2)}
    assert any(c.C1 % 32 and c.tile == 1 for c in f) and any(c.C1 % 32 and c.tile == 2 for c in f) and any(c.C2 for c in f)
    sp, sr = of("split"), of("split_ring")
    assert all(c.depth == 4 for c in sp) and all(c.depth == 2 for c in sr)
    assert any(not c.env for c in sr) and any(c.env == cases.CUS8 for c in sr)
    assert any(nb(c, 2) == 4 * c.nsplit for c in sr)
    s_short = cases.by_name("split_ring_one_brick_short")
    assert s_short.kernel == "split" and nb(s_short, 2) == 4 * 8 - 1 and s_short.env == cases.CUS8
    assert any(c.C1 % 32 for c in sp) and any(c.C2 for c in sp) and any(c.C1 % 32 for c in sr)
    assert cases.families("f32") == R.FAMILIES and cases.families("bf16") == cases.families("f16") == ("ints",)
    assert all(c.dtypes == ("f32",) for c in f + sp + sr)  # so every row of the fp32 kernels runs the wide families
    # ---- direct
    d = of("direct")
    assert any((c.C1, c.Cout) == (8, 40) and set(c.dtypes) == {"f32", "bf16", "f16"} and c.impl == cases.AUTO for c in d)
    assert any(c.impl == cases.DIRECT and cases.h16_supported(c.C1, c.C2, c.Cout) and "bf16" in c.dtypes for c in d)
    assert any(c.nsplit > 1 and not c.nslab for c in d)
    # ---- merges
    mf = [c for c in C if c.kernel != "direct"]
    assert any(0 < c.nslab <= 8 for c in mf) and any(c.nslab > 8 and c.sum_unpack for c in mf)
    assert {c.kernel for c in mf if c.nslab == 0} >= {"brick16", "brick_f32", "split", "split_ring"}  # atomics
    a16 = cases.by_name("b16_atomics_171_splits")
    assert a16.nsplit == cases.slab_capacity(a16.C1 + a16.C2, a16.Cout) + 1 and nb(a16) >= 171
    det = [c for c in C if c.env.get("TDX_DETERMINISTIC") == "1"]
    assert {c.kernel for c in det} >= {"brick16", "small", "ring", "brick_f32", "split_ring", "direct"}
    assert all(c.nslab == c.nsplit for c in det)  # never atomics
    held = cases.by_name("b16_deterministic_170")
    assert held.nsplit == cases.slab_capacity(96, 32) and held[4:9] == a16[4:9]  # the atomics row's shape, held to the capacity
    dd = cases.by_name("direct_deterministic")
    assert 8 < dd.nslab <= 64 and not dd.sum_unpack  # the tiled unpack walks the vector-ALU kernel's slabs, up to 64
    assert any(not c.bias for c in C)
    assert set(cases.WS_CLEAN_TWICE) <= set(CASE_IDS) and {cases.by_name(n).kernel for n in cases.WS_CLEAN_TWICE} == set(cases.KERNELS)
    assert {cases.by_name(n).kernel for n in cases.AUTOGRAD} == set(cases.KERNELS)


def _defects(c, p, family):
    """{name: (dW, dbias)} of the planted defects that apply to the row"""
    x1, x2, dy = p["x1"], p["x2"], p["dy"]
    B, (X, Y, Z) = c.B, c.grid
    dW, db = R.wgrad(x1, x2, dy)
    out = {"zero padding instead of clamp": R.wgrad(x1, x2, dy, zero_pad=True)}
    keep = torch.ones(B, X, Y, Z, dtype=torch.bool)
    keep[-1, -1, -1, -1] = False
    out["last voxel of the last sample dropped"] = R.wgrad(x1, x2, dy, keep=keep.flatten())
    for a, b in ((2, 3), (3, 4), (2, 4)):
        out[f"tap axes {a - 2} and {b - 2} swapped"] = (dW.transpose(a, b).contiguous(), db)
    keep = torch.ones(B, X, Y, Z, dtype=torch.bool)
    keep[0, X - 1, Y - 1, :] = False  # the last voxel row of sample 0: a row of a ragged brick where the grid has one
    out["one voxel row of a ragged brick dropped"] = R.wgrad(x1, x2, dy, keep=keep.flatten())
    if x2 is not None and c.C1 >= c.C2:
        out["x2 read at x1's channel offset"] = R.wgrad(x1, x1[..., :c.C2], dy)
    if family == "wide-x":
        out["xl dyh omitted"] = R.wgrad(R.drop_lo(x1), R.drop_lo(x2), dy)
    if family == "wide-dy":
        out["xh dyl omitted"] = R.wgrad(x1, x2, R.drop_lo(dy))
    return (dW, db), out


@pytest.mark.parametrize("name", cases.DEFECTS)
def test_planted_defects_are_visible_on_the_exact_inputs(name):
    """Each planted defect of the reference differs from the reference on the row's own exact inputs, as float32: the
    torch.equal of the GPU tests would fail for a kernel with that defect."""
    c = cases.by_name(name)
    assert any(e % b for e, b in zip(c.grid, (4, 8, 8))) and (c.C2 == 0 or c.C1 >= c.C2)
    for fam in sorted({f for d in c.dtypes for f in cases.families(d)}):
        (dW, db), planted = _defects(c, R.exact_inputs(c.B, c.grid, c.C1, c.C2, c.Cout, fam), fam)
        assert len(planted) == 6 + (c.C2 > 0) + (fam != "ints")
        for what, (w, b) in planted.items():
            assert not torch.equal(w.float(), dW.float()), f"{name} {fam}: {what} is invisible in dW"
            if "dropped" in what:
                assert not torch.equal(b.float(), db.float()), f"{name} {fam}: {what} is invisible in dbias"


def test_planted_defects_cover_the_list():
    fams = {f for n in cases.DEFECTS for d in cases.by_name(n).dtypes for f in cases.families(d)}
    assert fams == set(R.FAMILIES) and any(cases.by_name(n).C2 for n in cases.DEFECTS)


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
    unwritten = a.clone()
    unwritten[1, 2] = float("nan")
    with pytest.raises(AssertionError, match="1 of 16"):
        _assert_equal(unwritten, a, "an unwritten element")
    with pytest.raises(AssertionError, match="1 of 16"):
        _assert_within(unwritten, a.double(), torch.ones(4, 4, dtype=torch.float64), "an unwritten element")


# ---------------------------------------------------------------------------------------------------------------- on the GPU


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _exact(B, grid, C1, C2, Cout, family):
    """(inputs on the device, (dW, dbias) of the reference as float32): computed once, shared, never written"""
    p = {k: (None if v is None else v.to(_dev())) for k, v in R.exact_inputs(B, grid, C1, C2, Cout, family).items()}
    dW, db = R.wgrad(p["x1"], p["x2"], p["dy"])
    assert torch.equal(dW.float().double(), dW) and torch.equal(db.float().double(), db)
    return p, (dW.float(), db.float())


def _as(t, dt):
    return None if t is None else t.to(dt).contiguous()


def _bind_arena(L, c):
    """the arena of the launching stream, or none for a row that runs without one; returns how to launch"""
    if c.arena:
        L.ensure_scratch(_dev())
        return L.call
    assert L.load().tdx_set_scratch(None, 0) == 0
    L._ACTIVE = None  # the next `call` binds its arena again

    def bare(name, *args):
        rc = getattr(L.load(), name)(*args)
        assert rc == 0, f"{name} failed: {rc}"

    return bare


def _wgrad(L, c, dname, p, ws=None, bias=None):
    """tdx_conv3_bwd_weight for the row: asserts the plan (the kernel the row names) with the real arena bound, launches into
    NaN-filled outputs with a margin behind dW.  ws None: a workspace of its own filled with a non-zero pattern, the call
    zeroes its accumulators itself; else the given zeroed workspace with TDX_WS_CLEAN."""
    d, dt = _dev(), DT[dname]
    Cin = c.C1 + c.C2
    bias = c.bias if bias is None else bias
    x1, x2, dy = _as(p["x1"], dt), _as(p["x2"], dt), _as(p["dy"], dt)
    buf = torch.full((c.Cout * Cin * 27 + MARGIN,), float("nan"), device=d)
    buf[c.Cout * Cin * 27:] = SENTINEL
    db = torch.full((c.Cout,), float("nan"), device=d) if bias else None
    impl = c.impl
    if ws is None:
        ws = torch.full((L.query("tdx_conv3_bwd_weight_workspace_bytes", Cin, c.Cout, c.impl),), 0x7f, dtype=torch.uint8, device=d)
    else:
        impl |= L.WS_CLEAN
    with L._LAUNCH_LOCK:
        launch = _bind_arena(L, c)
        _assert_plan(L, c, dname, c.arena)
        launch("tdx_conv3_bwd_weight", L.ptr(x1), c.C1, L.ptr(x2), c.C2, L.ptr(dy), L.ptr(buf), L.ptr(db), c.B, *c.grid, c.Cout,
               L.dtype_code(dt), impl, L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert bool((buf[c.Cout * Cin * 27:] == SENTINEL).all()), "the margin behind dW was written"
    return buf[: c.Cout * Cin * 27].view(c.Cout, Cin, 3, 3, 3), db


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.CASES, ids=CASE_IDS)
def test_weight_gradient_on_exact_inputs_is_the_reference(case, monkeypatch):
    from turbdiff_amd import _lib as L

    c = case
    _set_case_env(monkeypatch, c)
    for dname in c.dtypes:
        for fam in cases.families(dname):
            p, (dW, db) = _exact(c.B, c.grid, c.C1, c.C2, c.Cout, fam)
            got_w, got_b = _wgrad(L, c, dname, p)
            _assert_equal(got_w, dW, f"{c.name} {dname} {fam} dW")
            if c.bias:
                _assert_equal(got_b, db, f"{c.name} {dname} {fam} dbias")


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.WS_CLEAN_TWICE)
def test_ws_clean_twice_on_one_zeroed_workspace(name, monkeypatch):
    """TDX_WS_CLEAN: the caller hands in zeroed accumulators and gets them back zeroed -- twice on one workspace, the second
    result equal to the first and to the reference; once more without a bias gradient."""
    from turbdiff_amd import _lib as L

    c = cases.by_name(name)
    _set_case_env(monkeypatch, c)
    Cin = c.C1 + c.C2
    p, (dW, db) = _exact(c.B, c.grid, c.C1, c.C2, c.Cout, "ints")
    for dname in c.dtypes:
        ws = torch.zeros(L.query("tdx_conv3_bwd_weight_workspace_bytes", Cin, c.Cout, c.impl), dtype=torch.uint8, device=_dev())
        for rep, bias in enumerate((True, True, False)):
            got_w, got_b = _wgrad(L, c, dname, p, ws=ws, bias=bias)
            assert int(ws[: (27 * Cin * c.Cout + c.Cout) * 4].count_nonzero()) == 0, f"{c.name} {dname} call {rep}: accumulators not left zero"
            _assert_equal(got_w, dW, f"{c.name} {dname} call {rep} dW")
            if bias:
                _assert_equal(got_b, db, f"{c.name} {dname} call {rep} dbias")


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.CASES, ids=CASE_IDS)
def test_weight_gradient_on_gaussian_inputs_within_the_derived_bound(case, monkeypatch):
    """Operands with full significands on every row and storage format: whatever the kernel, the K split and the merge"""
    from turbdiff_amd import _lib as L

    c = case
    _set_case_env(monkeypatch, c)
    for dname in c.dtypes:
        p = {k: (None if v is None else v.to(_dev())) for k, v in R.gaussian_inputs(c.B, c.grid, c.C1, c.C2, c.Cout, DT[dname]).items()}
        dW, db = R.wgrad(p["x1"], p["x2"], p["dy"])
        bw, bb = (R.split_bound if c.kernel in ("split", "split_ring") else R.wgrad_bound)(p["x1"], p["x2"], p["dy"])
        got_w, got_b = _wgrad(L, c, dname, p)
        _assert_within(got_w, dW, bw, f"{c.name} {dname} dW")
        if c.bias:
            _assert_within(got_b, db, bb, f"{c.name} {dname} dbias")


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.AUTOGRAD)
def test_one_row_per_kernel_through_autograd_is_exact(name, monkeypatch):
    """ops.conv3(...).backward: the weight and bias gradients the optimiser sees, on the kernel the row names"""
    from turbdiff_amd import _lib as L
    from turbdiff_amd import ops

    c = cases.by_name(name)
    _set_case_env(monkeypatch, c)
    if IMPL_NAMES[c.impl]:
        monkeypatch.setenv("TDX_CONV_IMPL", IMPL_NAMES[c.impl])
    assert c.arena and L.conv_impl() == c.impl
    p, (dW, db) = _exact(c.B, c.grid, c.C1, c.C2, c.Cout, "ints")
    for dname in c.dtypes:
        dt = DT[dname]
        w = torch.zeros(c.Cout, c.C1 + c.C2, 3, 3, 3, device=_dev(), requires_grad=True)
        b = torch.zeros(c.Cout, device=_dev(), requires_grad=True)
        with L._LAUNCH_LOCK:
            L.ensure_scratch(_dev())
            _assert_plan(L, c, dname, True)
        y = ops.conv3(_as(p["x1"], dt), w, b, _as(p["x2"], dt))
        y.backward(_as(p["dy"], dt))
        torch.cuda.synchronize()
        _assert_equal(w.grad, dW, f"{c.name} {dname} weight.grad")
        _assert_equal(b.grad, db, f"{c.name} {dname} bias.grad")
