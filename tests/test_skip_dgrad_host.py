"""Host side of the fused skip data gradient (tdx_conv3_bwd_data_skip), no GPU needed: the library's `supported` rule over a table
of shapes and switches (pure host code behind tdx_conv3_bwd_data_skip_supported; tdx_set_scratch only stores the pointer, so a
host buffer stands in for the arena, as in test_conv3_routing_is_pinned), its agreement with the static preconditions ops.py
asks the library behind, and the float64 reference of tests/skip_dgrad_reference.py against autograd of the defining
expression."""

import ctypes

import pytest
import torch

import skip_dgrad_reference as S

BF16, F16, F32 = "bf16", "f16", "f32"
DT = {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32}
BENCH = (6, 192, 64, 48)
# (C1, C2, Cout, (B, X, Y, Z), dtype, environment, arena?) -> supported
ROUTES = [
    ((64, 64, 32, BENCH, BF16, {}, True), 1),                         # up.3.block1 of the benchmark model
    ((64, 64, 32, BENCH, F16, {}, True), 1),
    ((128, 0, 32, BENCH, BF16, {}, True), 1),                         # one input tensor
    ((64, 64, 32, (6, 96, 32, 24), BF16, {}, True), 1),               # 864 bricks x 2 N tiles: still a ring launch
    ((64, 64, 32, BENCH, BF16, {"TDX_SKIP_DGRAD_FUSE": "0"}, True), 0),   # the A/B switch
    ((64, 64, 32, BENCH, BF16, {"TDX_SKIP_DGRAD_FUSE": "1"}, True), 1),
    ((64, 64, 32, BENCH, BF16, {}, False), 0),                        # no arena: the data gradient is not on the ring kernel
    ((64, 64, 32, BENCH, BF16, {"TDX_CONV3_RING": "0"}, True), 0),
    ((64, 64, 32, BENCH, BF16, {"TDX_RING_LOADERS": "0"}, True), 0),  # the loader-less A/B form has no skip term
    ((64, 64, 32, BENCH, F16, {"TDX_RING_LOADERS": "0"}, True), 1),   # fp16 runs the loader form whatever the switch says
    ((64, 64, 32, BENCH, F32, {}, True), 0),
    ((64, 64, 64, BENCH, BF16, {}, True), 0),                         # K = 64 (up.2.block1's kind)
    ((32, 0, 32, BENCH, BF16, {}, True), 0),                          # 32-wide output tiles
    ((32, 32, 32, BENCH, BF16, {}, True), 1),
    ((48, 48, 32, BENCH, BF16, {}, True), 0),                         # C1 + C2 = 96: not whole 64-wide tiles
    ((64, 64, 32, (6, 194, 50, 50), BF16, {}, True), 0),              # ring kernel + remainder slabs: no skip term there
    ((64, 64, 32, (6, 192, 64, 50), BF16, {}, True), 0),
    ((64, 64, 32, (6, 48, 16, 12), BF16, {}, True), 0),               # 4-deep bricks
    ((32, 32, 32, (2, 16, 16, 8), BF16, {}, True), 0),                # too few bricks for a persistent launch ...
    ((32, 32, 32, (2, 16, 16, 8), BF16, {"TDX_CONV3_RING": "2"}, True), 1),   # ... unless the tests' switch says "whenever legal"
    ((32, 32, 32, (1, 17, 8, 8), BF16, {"TDX_CONV3_RING": "2"}, True), 0),
    ((32, 32, 64, (1, 16, 8, 8), BF16, {"TDX_CONV3_RING": "2"}, True), 0),
    ((32, 32, 32, (1, 16, 8, 8), F32, {"TDX_CONV3_RING": "2"}, True), 0),
    ((12, 20, 32, BENCH, BF16, {}, True), 0),                         # channels that are no multiple of 8
]


def test_supported_rule_and_static_preconditions_agree(monkeypatch):
    from turbdiff_amd import _lib as L
    from turbdiff_amd import ops

    lib = L.load()
    switches = L.switch_names() + ("TDX_CONV_IMPL",)  # the library's own list, and the Python-side override
    fake = ctypes.create_string_buffer(256)  # zeroed; never dereferenced by the query
    try:
        for (C1, C2, Cout, grid, dn, envs, arena), want in ROUTES:
            for v in switches:
                monkeypatch.delenv(v, raising=False)
            for k, v in envs.items():
                monkeypatch.setenv(k, v)
            assert lib.tdx_set_scratch(ctypes.addressof(fake) if arena else None, (96 << 20) if arena else 0) == 0
            got = L.query("tdx_conv3_bwd_data_skip_supported", C1, C2, Cout, *grid, L.dtype_code(DT[dn]), L.CONV_AUTO)
            assert got == want, (C1, C2, Cout, grid, dn, envs, arena)
            static = ops.skip_dgrad_static(Cout, grid, DT[dn])
            assert static or not got, "the library serves a call ops.py never asks about"
            # what the caller cannot see is everything else: the switch, the arena, the route, the tile width
            if not static:
                assert dn == F32 or Cout != 32 or any(e % 8 for e in grid[1:])
    finally:
        lib.tdx_set_scratch(None, 0)
        L._ACTIVE = None  # a later GPU test in this process binds its real arena again


def test_static_preconditions():
    from turbdiff_amd import ops

    ok = (32, (2, 16, 16, 8), torch.bfloat16)
    assert ops.skip_dgrad_static(*ok) and ops.skip_dgrad_static(32, (2, 16, 16, 8), torch.float16)
    assert not ops.skip_dgrad_static(64, (2, 16, 16, 8), torch.bfloat16)
    assert not ops.skip_dgrad_static(32, (2, 16, 16, 8), torch.float32)
    assert not ops.skip_dgrad_static(32, (2, 16, 16, 8), torch.bfloat16, torch.bfloat16)
    for grid in ((2, 17, 16, 8), (2, 16, 12, 8), (2, 16, 16, 5), (2, 4, 3, 5)):
        assert not ops.skip_dgrad_static(32, grid, torch.bfloat16)


@pytest.mark.parametrize("C2", [8, 0])
def test_reference_is_autograd_of_the_defining_expression(C2):
    p = S.exact_inputs(2, (4, 3, 5), 8, C2, 16, seed=3)
    r = S.reference(p)
    S.assert_exact(p, r)
    want = S.direct(p)
    assert torch.equal(r["ref"], want)  # dyadic inputs: every float64 sum is exact, whatever its order
    # the pieces: ref = main + fold of the halo + skip; the bounds' magnitudes dominate what they bound
    assert bool((r["mag"] >= r["ref"].abs()).all()) and bool((r["fold_abs"] >= (r["ref"] - r["adj_main"] - r["skip"]).abs()).all())
    inner = S.interior((4, 3, 5))
    assert int(inner.sum()) == 2 * 1 * 3 and torch.equal((r["ref"] - r["adj_main"] - r["skip"])[:, inner], torch.zeros(2, 6, 8 + C2).double())


def test_fold_counts():
    f = S.fold_counts((8, 16, 8))
    assert f[0, 0, 0] == 7 and f[7, 15, 7] == 7 and f[0, 0, 3] == 3 and f[4, 15, 7] == 3 and f[0, 5, 3] == 1 and f[3, 5, 3] == 0
    assert int((f == 0).sum()) == 6 * 14 * 6 and int((f == 7).sum()) == 8


def test_bounds_count_the_roundings():
    p = S.exact_inputs(1, (8, 8, 8), 32, 32, 32, seed=5)
    r = S.reference(p)
    fused, two = S.bounds(r, torch.bfloat16)
    inner = S.interior((8, 8, 8))[None, :, :, :, None].expand_as(fused)
    assert bool((fused[inner] < two[inner]).all())
    f32_fused, f32_two = S.bounds(r, torch.float32)
    assert torch.equal(f32_fused, f32_two) and bool((f32_fused < fused).all())
