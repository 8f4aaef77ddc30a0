"""The GroupNorm kernels of csrc/tdx_groupnorm.hip against the float64 reference of tests/gn_reference.py, at shapes with many
blocks per sample, on inputs for which the kernels' arithmetic is exact: the reference is then THE answer and every tolerance is
0 (torch.equal), 1 ulp of float32, or a bound derived in the docstring of gn_reference.py.  None is a measured number.

Without a GPU: the reference against float64 autograd of F.group_norm, the branch every shape is listed for (against the
restated grid rules gn_cases.lane_paths and gn_reference.stats_geometry), and the exactness preconditions of every exact case.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import gn_cases as cases
import gn_reference as R

TRIP, TAIL, BOTH = cases.TRIP, cases.TAIL, cases.BOTH

# (B, C, G, V): blocks per sample, voxel stride, spare threads, lane paths, slots of gn_bwd_group_kernel's t[] in use
MANY_BLOCKS = {
    (1, 512, 8, 9000): (512, 2048, 0, {BOTH, TRIP}, 8),  # GN_MAX_BLOCKS binds; lanes below voxel 808 run a trip AND the tail
    (1, 64, 8, 12000): (94, 3008, 0, {TRIP, TAIL}, 2),   # second slot partly filled
    (2, 24, 8, 300): (1, 85, 1, {TRIP, TAIL}, 1),        # groups of 3 channels straddle the 8-channel lane vector; a spare thread
    (2, 40, 8, 300): (2, 102, 1, {TAIL}, 1),             # groups of 5, two blocks
    (2, 32, 32, 70): (1, 64, 0, {TAIL}, 1),              # one channel per group
}
SHAPES = cases.SMALL + list(MANY_BLOCKS)

# tdx_gn_stats.  (B, C, G, V): per TDX_DETERMINISTIC (vpb, blocks, rows, spare threads, values per thread, block paths)
STATS = {
    (1, 8, 1, 5): {0: (32, 1, 256, 0, 1, {TAIL}), 1: (32, 1, 256, 0, 1, {TAIL})},              # vpb floor, rows > vpb
    (3, 512, 8, 150): {0: (32, 5, 4, 0, 8, {TRIP, BOTH}), 1: (32, 5, 4, 0, 8, {TRIP, BOTH})},  # rows = 4: two trips; a trip and the tail in the last block
    (1, 24, 3, 1500): {0: (32, 47, 85, 1, 1, {TAIL}), 1: (32, 47, 85, 1, 1, {TAIL})},          # spare thread
    (2, 8, 2, 70000): {0: (1024, 69, 256, 0, 4, {TRIP, TAIL}), 1: (1120, 63, 256, 0, 5, {BOTH, TRIP, TAIL})},  # 1024 cap; 64-block cap re-sizes vpb
    (1, 512, 8, 9000): {0: (96, 94, 4, 0, 24, {TRIP, BOTH}), 1: (160, 57, 4, 0, 40, {TRIP, BOTH})},  # wide rows, many blocks
    (2, 16, 2, 64): {0: (32, 2, 128, 0, 1, {TAIL}), 1: (32, 2, 128, 0, 1, {TAIL})},            # constant input: var == 0
    (1, 8, 8, 1): {0: (32, 1, 256, 0, 1, {TAIL}), 1: (32, 1, 256, 0, 1, {TAIL})},              # one element per group
}
CONSTANT = {(2, 16, 2, 64): 3}
OFFSET = [(3, 512, 8, 150), (2, 8, 2, 70000)]
NO_ARENA = (2, 8, 2, 70000)  # one block of 70016 voxels per sample: (70016, 1, 256, 0, 274, {BOTH})
ARENA = 96 << 20
EPS = R.f32(1e-5)
DTYPES = cases.DTYPES
FLAGS = [(film, res) for film in (False, True) for res in (False, True)]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ------------------------------------------------------------------------------------------------------------ without a GPU


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("film,res", FLAGS)
def test_reference_is_the_autograd_of_group_norm(film, res, act):
    B, C, G, V = 2, 24, 3, 37
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, r, dy = 1.5 * rn(B, V, C) + 0.3, rn(B, V, C), rn(B, V, C)
    gamma, beta, scale, shift = 1 + 0.3 * rn(C), 0.2 * rn(C), 0.5 * rn(B, C), 0.5 * rn(B, C)
    eps = 1e-5
    leaves = [t.clone().requires_grad_() for t in (x, gamma, beta, scale, shift, r)]
    xa, ga, ba, sa, ha, ra = leaves
    n = F.group_norm(xa.transpose(1, 2), G, ga, ba, eps).transpose(1, 2)
    if film:
        n = n * (1 + sa[:, None, :]) + ha[:, None, :]
    y = F.silu(n) if act else n
    y = y + ra if res else y
    y.backward(dy)

    st = R.stats(x, G, eps)
    sc, sh = (scale, shift) if film else (None, None)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert close(R.apply(x, st, gamma, beta, sc, sh, r if res else None, act), y.detach())
    ref = R.bwd(x, dy, st, gamma, beta, sc, sh, act, round_group_means=False)
    assert close(ref.dx, xa.grad) and close(ref.dgamma, ga.grad) and close(ref.dbeta, ba.grad)
    if film:
        assert close(ref.dscale, sa.grad) and close(ref.dshift, ha.grad)


def test_ulp_distance_and_spacing():
    a = torch.tensor([1.0, -1.0, 0.0, 1e-45, 3.0])
    b = torch.tensor([1.0 + 2.0**-23, -1.0 - 2.0**-22, -0.0, -1e-45, 3.0])
    assert R.ulp_distance(a, b).tolist() == [1, 2, 0, 2, 0]
    ref = torch.tensor([1.0, 1.5, 0.75, 2.0**-20, 0.0], dtype=torch.float64)
    assert R.ulp_of(ref, torch.bfloat16).tolist() == [2.0**-7, 2.0**-7, 2.0**-8, 2.0**-27, 2.0**-133]
    assert R.ulp_of(ref, torch.float16).tolist() == [2.0**-10, 2.0**-10, 2.0**-11, 2.0**-24, 2.0**-24]


@pytest.mark.parametrize("shape", list(MANY_BLOCKS), ids=_ids(MANY_BLOCKS))
def test_streaming_shapes_reach_their_branches(shape):
    B, C, G, V = shape
    blocks, stride, spare, paths, slots = MANY_BLOCKS[shape]
    assert cases.lane_paths(B, C, V) == (blocks, stride, spare, paths)
    assert -(-blocks // 64) == slots and blocks <= cases.MAX_BLOCKS
    if C // G in (3, 5):  # some group boundary falls inside a thread's 8 channels
        assert any((g * (C // G)) % 8 for g in range(G))


@pytest.mark.parametrize("shape", list(STATS), ids=_ids(STATS))
def test_statistics_shapes_reach_their_branches(shape):
    B, C, G, V = shape
    for det in (0, 1):
        geo = R.stats_geometry(B, V, C, bool(det), ARENA)
        assert tuple(geo[:6]) == STATS[shape][det] and geo.tables == bool(det)
        assert not det or geo.blocks <= 64
    assert max(STATS[s][1][1] for s in STATS) > 1  # gn_stats_merge_kernel adds more than one table somewhere
    B, C, G, V = NO_ARENA
    assert tuple(R.stats_geometry(B, V, C, True, 0)) == (70016, 1, 256, 0, 274, {BOTH}, False)
    assert R.stats_geometry(B, V, C, True, 1 << 10).tables is False  # an arena too small for the tables: the same fallback


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_exact_cases_meet_their_preconditions(shape, act):
    p = R.dyadic_inputs(shape, narrow=act)
    for dt in DTYPES.values():  # the inputs are the same numbers in every storage format
        assert all(torch.equal(p[k].to(dt).float(), p[k]) for k in ("x", "res", "dy"))
    for film in (False, True):
        R.assert_exact(p, film, act)


@pytest.mark.parametrize("shape", list(STATS), ids=_ids(STATS))
def test_exact_statistics_meet_their_preconditions(shape):
    B, C, G, V = shape
    x = R.integer_input(shape, constant=CONSTANT.get(shape))
    assert torch.equal(x, x.round()) and x.abs().max() <= 8
    assert all(torch.equal(x.to(dt).float(), x) for dt in DTYPES.values())
    per_thread = max(R.stats_geometry(B, V, C, det, a).per_thread for det, a in ((False, ARENA), (True, ARENA), (True, 0)))
    assert per_thread * 64 < 2**24  # a thread's float32 sum of x^2; block and grid sums are f64 sums of integers below 2^53
    assert (x.double() ** 2).sum().item() < 2.0**53


# ---------------------------------------------------------------------------------------------------------------- on the GPU


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(shape, narrow):
    return {k: v.to(_dev()) for k, v in R.dyadic_inputs(shape, narrow=narrow).items()}


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
           f"bound {bound.flatten()[i].item():.3e}"


def _within(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_apply_without_activation_is_the_reference_rounded_once(shape):
    from turbdiff_amd import _lib as L

    G = shape[2]
    p = _inputs(shape, False)
    for film, res in FLAGS:
        sc, sh = (p["scale"], p["shift"]) if film else (None, None)
        ref = R.apply(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh, p["res"] if res else None, False)
        assert torch.equal(ref.float().double(), ref)  # exact in float32: the store to T is the one rounding
        for name, dt in DTYPES.items():
            y = _apply(L, p["x"].to(dt), p, film, p["res"].to(dt) if res else None, False, G)
            want = ref.float().to(dt)
            assert torch.equal(y, want), f"{name} film={film} res={res}: {int((y != want).sum())} of {y.numel()} elements differ"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_apply_with_silu_within_the_derived_bound(shape):
    from turbdiff_amd import _lib as L

    G = shape[2]
    p = _inputs(shape, True)
    for film, res in FLAGS:
        sc, sh = (p["scale"], p["shift"]) if film else (None, None)
        r = p["res"] if res else None
        n, _ = R.pre_activation(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh)
        assert n.abs().max().item() <= R.N_MAX and torch.equal(n.float().double(), n)
        ref = R.apply(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh, r, True)
        for name, dt in DTYPES.items():
            y = _apply(L, p["x"].to(dt), p, film, None if r is None else r.to(dt), True, G)
            bound = R.apply_bound(n, r, ref, dt)
            assert _within(y, ref, bound), f"{name} film={film} res={res}: {_worst(y, ref, bound)}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_backward_without_activation_exact_sums_and_two_roundings(shape):
    from turbdiff_amd import _lib as L

    G = shape[2]
    p = _inputs(shape, False)
    for film in (False, True):
        sc, sh = (p["scale"], p["shift"]) if film else (None, None)
        ref = R.bwd(p["x"], p["dy"], p["stats"], p["gamma"], p["beta"], sc, sh, False)
        for name, dt in DTYPES.items():
            got = _bwd(L, p["x"].to(dt), p["dy"].to(dt), p, film, False, G)
            for key in ("dgamma", "dbeta") + (("dscale", "dshift") if film else ()):
                want = getattr(ref, key).float()
                assert torch.equal(got[key], want), \
                    f"{name} film={film} {key}: {int((got[key] != want).sum())} of {want.numel()} differ, " \
                    f"by up to {(got[key].double() - want.double()).abs().max().item()!r}"
            bound = R.dx_rounding(ref.terms, ref.dx, dt)
            assert _within(got["dx"], ref.dx, bound), f"{name} film={film} dx: {_worst(got['dx'], ref.dx, bound)}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_backward_with_silu_within_the_derived_bounds(shape):
    from turbdiff_amd import _lib as L

    B, C, G, V = shape
    p = _inputs(shape, True)
    for film in (False, True):
        sc, sh = (p["scale"], p["shift"]) if film else (None, None)
        ref = R.bwd(p["x"], p["dy"], p["stats"], p["gamma"], p["beta"], sc, sh, True)
        assert ref.terms["n"].abs().max().item() <= R.N_MAX
        for name, dt in DTYPES.items():
            bounds = R.bwd_bounds(ref, p["dy"], p["gamma"], p["beta"], _lanes(shape), G, V, dt)
            got = _bwd(L, p["x"].to(dt), p["dy"].to(dt), p, film, True, G)
            for key in ("dx", "dgamma", "dbeta") + (("dscale", "dshift") if film else ()):
                want = getattr(ref, key)
                assert _within(got[key], want, bounds[key]), f"{name} film={film} {key}: {_worst(got[key], want, bounds[key])}"


def _stats(L, x, G, eps=EPS):
    """tdx_gn_stats on a workspace of garbage; the [B][C][2] f64 table must be all zero afterwards (TDX_WS_CLEAN: what
    gn_stats_finalize read, it cleared)."""
    B, V, C = x.shape
    ws = torch.full((L.query("tdx_gn_workspace_bytes", B, C),), 0xFF, dtype=torch.uint8, device=x.device)
    out = torch.empty(B, G, 2, device=x.device)
    L.call("tdx_gn_stats", L.ptr(x), L.ptr(out), B, V, C, G, eps, L.dtype_code(x.dtype), L.ptr(ws), L.stream())
    table = ws[: B * C * 2 * 8].view(torch.int64)
    assert int(table.count_nonzero()) == 0, "the statistics table of the workspace was not left all-zero"
    return out


def _set_deterministic(monkeypatch, det):
    if det:
        monkeypatch.setenv("TDX_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("TDX_DETERMINISTIC", raising=False)


def _assert_one_ulp(got, want, what):
    dist = R.ulp_distance(got, want.float())
    assert int(dist.max()) <= 1, f"{what}: mean / rstd up to {int(dist.max())} ulp from the reference\n{got.cpu()}\n{want.cpu()}"


@pytest.mark.gpu
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("shape", list(STATS), ids=_ids(STATS))
def test_statistics_of_integer_input_within_one_ulp(shape, det, monkeypatch):
    from turbdiff_amd import _lib as L

    B, C, G, V = shape
    _set_deterministic(monkeypatch, det)
    assert L.deterministic() == bool(det)
    assert R.stats_geometry(B, V, C, bool(det), L.SCRATCH_BYTES).tables == bool(det)  # the tables and their merge really run
    x = R.integer_input(shape, constant=CONSTANT.get(shape)).to(_dev())
    want = R.stats(x, G, EPS)
    if shape in CONSTANT or V == 1:
        assert torch.equal(want[..., 1], torch.full_like(want[..., 1], 1.0 / EPS**0.5))  # var == 0 exactly
    for name, dt in DTYPES.items():
        _assert_one_ulp(_stats(L, x.to(dt), G), want, f"{name} deterministic={det}")


@pytest.mark.gpu
def test_statistics_without_an_arena_take_one_block_per_sample(monkeypatch):
    """TDX_DETERMINISTIC with no scratch arena bound (TDX_SCRATCH_MB=0): one block per sample adds into the zeroed table."""
    from turbdiff_amd import _lib as L

    B, C, G, V = NO_ARENA
    _set_deterministic(monkeypatch, 1)
    x = R.integer_input(NO_ARENA).to(_dev())
    want = R.stats(x, G, EPS)
    old = L.SCRATCH_BYTES
    try:
        L.SCRATCH_BYTES, L._ACTIVE = 0, None  # the next arena user binds "no arena"
        for name, dt in DTYPES.items():
            _assert_one_ulp(_stats(L, x.to(dt), G), want, f"{name} no arena")
        assert L._ACTIVE is not None  # the calls went through a binding, and it was "no arena"
    finally:
        L.SCRATCH_BYTES, L._ACTIVE = old, None  # and the next one gets its stream's arena back
    L.ensure_scratch()
    assert (L.scratch_arena() is not None) == (old > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("shape", OFFSET, ids=_ids(OFFSET))
def test_statistics_of_offset_input_within_the_float32_accumulation_bound(shape, det, monkeypatch):
    """x ~ N(16, 1) in float32: E[x^2] - mean^2 loses mean^2 / var = 256 times the accumulation error of the float32 per-thread
    sums.  The bound (gn_reference.var_bound) is that worst case: it pins the precision the pass has, no better."""
    from turbdiff_amd import _lib as L

    B, C, G, V = shape
    _set_deterministic(monkeypatch, det)
    geo = R.stats_geometry(B, V, C, bool(det), L.SCRATCH_BYTES)
    assert geo.tables == bool(det)
    x = (16.0 + torch.randn(B, V, C, generator=torch.Generator().manual_seed(5))).to(_dev())
    assert x.min().item() > 0  # no sign change: a thread's sum of x errs by (n_t - 1) u relative
    xd = x.double().reshape(B, V, G, C // G)
    mean, var = xd.mean((1, 3)), xd.var((1, 3), unbiased=False)
    got = _stats(L, x, G).double()
    var_got = got[..., 1] ** -2 - EPS
    rel = (var_got - var).abs() / var
    bound = R.var_bound(geo.per_thread, mean, var)
    assert bool((rel <= bound).all()), f"var off by {rel.max().item():.3e} relative, bound {bound.min().item():.3e}"
    # the mean: (n_t - 1) u from the thread's sum, u from the cast
    assert bool(((got[..., 0] - mean).abs() <= geo.per_thread * R.U * mean.abs() * R.SLACK).all())
