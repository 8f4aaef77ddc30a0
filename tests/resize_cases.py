"""The host routing of csrc/tdx_resize.hip restated in Python, and the table of shapes that tests/test_resize_reference.py runs.

`route(B, C, src, dst)` repeats what resize_plan decides for tdx_resize_fwd / tdx_resize_bwd before they launch: make_axis,
axis_taps, pair_taps / pair_window_ok, axis_range, axis_weight, axis_span / axis_max_span, make_tiles and the choice of K.  The
arithmetic is float32 through numpy scalars and arrays, operation for operation as in the C code (one float32 division for the
scale, one float32 product for the source index, truncation, the clamped second tap).  It is a pure function; no GPU, no
library: the independent model the error bounds of resize_reference.py are derived from.

The library is held against it by a test: test_resize_reference.py requires the library's plan query (tdx_resize_plan, which
calls the same resize_plan as the two entries) to equal `route` / `make_tiles` on every row of CASES, every shape of EARLIER and
300 generated shapes, without a GPU.  Every row of CASES names the route it was written for; the same module holds each row
against `route`, and every GPU test asserts the row's route and the library's plan again before it calls the library: a later
change of the routing, here or in the library, makes the row fail instead of quietly testing another kernel.
"""

from collections import namedtuple

import numpy as np

F32 = np.float32
RS_KMAX = 12
KS = (2, 4, 6, 12)
PAIRS, GATHER, GENERIC = "pairs", "gather", "generic"


# --------------------------------------------------------------------------------------------------------------- one axis


def make_axis(n_in, n_out):
    """(in, out, scale): scale = (float)(in - 1) / (float)(out - 1), 0 for out == 1"""
    return n_in, n_out, (F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0))


def axis_taps(axis):
    """i0, i1 (int64) and w1 (float32) of every output index, as axis_taps computes them"""
    n_in, n_out, scale = axis
    src = scale * np.arange(n_out, dtype=F32)  # float32 product
    i0 = np.minimum(src.astype(np.int32), n_in - 1).astype(np.int64)
    w1 = np.clip(src - i0.astype(F32), F32(0.0), F32(1.0)).astype(F32)
    i1 = i0 + (i0 + 1 < n_in)
    return i0, i1, w1


def axis_weights(axis):
    """out x in float32: axis_weight(a, o, i) for every pair (w = 0; if i0 == i: w += 1 - w1; if i1 == i: w += w1)"""
    n_in, n_out, _ = axis
    i0, i1, w1 = axis_taps(axis)
    W = np.zeros((n_out, n_in), dtype=F32)
    o = np.arange(n_out)
    W[o, i0] = F32(1.0) - w1
    W[o, i1] = W[o, i1] + w1  # float32 add; i1 == i0 at the clamped end
    return W


def pair_window_ok(axis):
    """the paired up-sampler's per-axis condition: the taps of outputs 2k and 2k + 1 lie in [base, base + 2], base = i0(2k)"""
    n_in, n_out, _ = axis
    if n_out < n_in:
        return False
    i0, i1, _ = axis_taps(axis)
    for o_even in range(0, n_out, 2):
        base = i0[min(o_even, n_out - 1)]
        for q in range(2):
            o = min(o_even + q, n_out - 1)
            if not (0 <= i0[o] - base <= 2 and 0 <= i1[o] - base <= 2):
                return False
    return True


def axis_range(axis, i):
    n_in, n_out, scale = axis
    if scale > 0:
        lo = max(0, int(np.floor(F32(i - 1) / scale)) - 1)
        hi = min(n_out - 1, int(np.ceil(F32(i + 1) / scale)) + 1)
        return lo, hi
    return 0, n_out - 1


def axis_span(axis, i, W=None):
    """(first, cnt): the first output with a non-zero weight on input i inside axis_range, and the count up to the last"""
    W = axis_weights(axis) if W is None else W
    lo, hi = axis_range(axis, i)
    hits = [o for o in range(lo, hi + 1) if W[o, i] != 0]
    if not hits:
        return hi + 1, 0
    return hits[0], hits[-1] - hits[0] + 1


def axis_max_span(axis):
    W = axis_weights(axis)
    return max(axis_span(axis, i, W)[1] for i in range(axis[0]))


# ------------------------------------------------------------------------------------------------------------------ tiles

Tiles = namedtuple("Tiles", "tile count partial passes")  # (tx, ty, tz); tiles per axis; partial tiles per axis; slot-loop trips


def make_tiles(X, Y, Z, C, samples):
    L = C >> 3
    vox = 256
    while vox > 8 and vox * L > 8 * 256:
        vox >>= 1
    one_pass = max(256 // L, 8)
    while samples > 0 and vox > one_pass and samples * X * Y * Z // vox < 1024:
        vox >>= 1
    tx, ty, tz = 4, 8, 8
    while tx * ty * tz > vox and tx > 1:
        tx >>= 1
    while tx * ty * tz > vox and ty > 1:
        ty >>= 1
    while tx * ty * tz > vox and tz > 1:
        tz >>= 1
    return (tx, ty, tz), tuple(-(-n // t) for n, t in zip((X, Y, Z), (tx, ty, tz)))


def _tiles(grid, C, B, slots_per_voxel):
    tile, count = make_tiles(*grid, C, B)
    per_pass = 256 // (C >> 3)
    slots = tile[0] * tile[1] * tile[2] // slots_per_voxel
    partial = tuple(int(n % t != 0) for n, t in zip(grid, tile))
    return Tiles(tile, count, partial, -(-slots // per_pass))


# ------------------------------------------------------------------------------------------------------------------ route

Route = namedtuple("Route", "fwd bwd fwd_tiles bwd_tiles spans")


def route(B, C, src, dst):
    """What tdx_resize_fwd and tdx_resize_bwd launch for x (B, *src, C) -> y (B, *dst, C):
    fwd `pairs` or `gather`; bwd 2 / 4 / 6 / 12 (the K of resize_bwd_kernel) or `generic`; the forward tiles (of the output
    grid; the pair kernel's slots are 2 x 2 x 2 blocks) and the adjoint's (of the input grid; None for the generic kernel) with
    the trips of the slot loop; the largest span (outputs reading one input) per axis."""
    assert C % 8 == 0 and C // 8 <= 256
    axes = [make_axis(i, o) for i, o in zip(src, dst)]
    tile, _ = make_tiles(*dst, C, B)
    paired = C <= 64 and not ((tile[0] | tile[1] | tile[2]) & 1) and all(o > i for i, o in zip(src, dst)) \
        and all(pair_window_ok(a) for a in axes)
    fwd_tiles = _tiles(dst, C, B, 8 if paired else 1)
    spans = tuple(axis_max_span(a) for a in axes)
    if max(spans) > RS_KMAX:
        return Route(PAIRS if paired else GATHER, GENERIC, fwd_tiles, None, spans)
    K = next(k for k in KS if spans[2] <= k)
    return Route(PAIRS if paired else GATHER, K, fwd_tiles, _tiles(src, C, B, 1), spans)


# ------------------------------------------------------------------------------------------------------------------ cases

F32_BF16 = ("f32", "bf16")
ALL = ("f32", "bf16", "f16")

Case = namedtuple("Case", "B C src dst dyadic fwd fwd_tile bwd bwd_tile spans dtypes why")


def _case(B, C, src, dst, dyadic, fwd, fwd_tile, bwd, bwd_tile, spans, why, dtypes=ALL):
    return Case(B, C, src, dst, dyadic, fwd, fwd_tile, bwd, bwd_tile, spans, dtypes, why)


# B, C, src, dst, dyadic ratios?, forward kernel and its tile, adjoint kernel and its tile, spans
CASES = [
    _case(1, 8, (9, 9, 9), (17, 17, 17), True, PAIRS, (4, 8, 8), 4, (4, 8, 8), (3, 3, 3),
          "pairs on 5 x 3 x 3 tiles, the last of each axis partial; K4 on 3 x 2 x 2 tiles"),
    _case(1, 8, (5, 9, 17), (9, 17, 33), True, PAIRS, (4, 8, 8), 4, (4, 8, 8), (3, 3, 3),
          "pairs, three different extents, partial tiles on each axis and 2 or more of them along y and z"),
    _case(1, 16, (5, 5, 3), (9, 9, 9), True, PAIRS, (2, 8, 8), 12, (2, 8, 8), (3, 3, 7),
          "pairs on the 2 x 8 x 8 tile; K12 with a z span of 7"),
    _case(1, 8, (2, 2, 2), (9, 9, 9), True, PAIRS, (4, 8, 8), 12, (4, 8, 8), (8, 8, 8),
          "K12 with spans 8, 8, 8; ratio 1/8: pair windows with one or two of three entries in use"),
    _case(1, 8, (12, 2, 12), (65, 3, 65), True, PAIRS, (4, 8, 8), 12, (4, 8, 8), (12, 2, 12),
          "K12 with all 12 candidates in use along x and z (ratio 11/64: spans of 11 and 12)"),
    _case(1, 8, (4, 4, 4), (9, 9, 9), True, PAIRS, (4, 8, 8), 6, (4, 8, 8), (5, 5, 5), "K6, ratio 3/8"),
    _case(1, 8, (3, 3, 3), (17, 17, 17), True, PAIRS, (4, 8, 8), GENERIC, None, (15, 15, 15), "generic adjoint, ratio 1/8"),
    _case(1, 24, (9, 5, 5), (17, 9, 9), True, GATHER, (1, 8, 8), 4, (1, 8, 8), (3, 3, 3),
          "C / 8 = 3: 85 voxels per pass, lane 255 idle; the odd tile rules the pair kernel out"),
    _case(1, 8, (9, 9, 9), (5, 5, 5), True, GATHER, (4, 8, 8), 2, (4, 8, 8), (1, 1, 1),
          "down-sampling by 2: K2, every odd input index is read by no output"),
    _case(1, 8, (7, 7, 7), (5, 5, 5), True, GATHER, (4, 8, 8), 2, (4, 8, 8), (1, 1, 1), "down-sampling by 3/2"),
    _case(1, 8, (1, 1, 1), (3, 4, 5), True, PAIRS, (4, 8, 8), 6, (4, 8, 8), (3, 4, 5), "in == 1: scale 0, every output reads input 0"),
    _case(1, 8, (4, 5, 6), (1, 1, 1), True, GATHER, (4, 8, 8), 2, (4, 8, 8), (1, 1, 1), "out == 1: only input 0 is read"),
    _case(2, 64, (33, 17, 17), (65, 33, 33), True, PAIRS, (2, 8, 8), 4, (1, 4, 8), (3, 3, 3),
          "pairs at the production width on the 2 x 8 x 8 tile, many tiles"),
    _case(2, 64, (32, 32, 16), (64, 64, 32), False, PAIRS, (4, 8, 8), 4, (1, 4, 8), (4, 4, 4),
          "pairs at C = 64 on the production 4 x 8 x 8 tile (B Vout = 262144), ratios 31/63, 31/63, 15/31"),
    _case(2, 16, (6, 3, 4), (13, 7, 9), False, PAIRS, (2, 8, 8), 6, (2, 8, 8), (5, 5, 5),
          "odd output extents on the pair kernel: the second output of the last pair is guarded; K6"),
    _case(1, 8, (4, 4, 4), (11, 11, 11), False, PAIRS, (4, 8, 8), 6, (4, 8, 8), (6, 6, 6),
          "K6 with all 6 candidates in use (ratio 3/10)"),
    _case(2, 64, (24, 16, 12), (48, 32, 43), False, PAIRS, (2, 8, 8), 12, (1, 4, 8), (4, 4, 8),
          "K12 at C = 64; pairs on the 2 x 8 x 8 tile (B Vout = 132096)"),
    _case(2, 512, (6, 4, 3), (3, 3, 3), True, GATHER, (1, 1, 8), 2, (1, 1, 8), (1, 1, 1),
          "wide channels: 4 voxels per pass; with Z = 3 the second trip over the 8-voxel tile writes nothing; ratios 5/2, 3/2, 1"),
    _case(1, 512, (2, 3, 9), (3, 2, 5), True, GATHER, (1, 1, 8), 2, (1, 1, 8), (2, 1, 1),
          "wide channels, both trips of the 8-voxel tile write (Z > 4 on both grids); ratios 1/2, 2, 2"),
    _case(1, 128, (6, 3, 7), (12, 6, 11), False, GATHER, (1, 2, 8), 4, (1, 2, 8), (4, 4, 3), "wide channels, up-sampling"),
    _case(2, 64, (32, 32, 32), (32, 32, 33), True, GATHER, (1, 8, 8), 2, (1, 8, 8), (1, 1, 2),
          "two trips of the slot loop in resize_fwd_kernel and in resize_bwd_kernel (B V >= 65536 on both written grids); ratios 1, 1, 31/32"),
    _case(2, 24, (32, 32, 64), (32, 32, 65), True, GATHER, (2, 8, 8), 2, (2, 8, 8), (1, 1, 2),
          "two trips with 85 voxels per pass: the second trip starts inside a z row of the tile (B V >= 131072); ratio 63/64",
          dtypes=F32_BF16),
    _case(1, 8, (12, 3, 3), (24, 6, 6), False, PAIRS, (4, 8, 8), 4, (4, 8, 8), (4, 4, 4), "the data grid's ratios, up"),
    _case(1, 8, (24, 6, 6), (12, 3, 3), False, GATHER, (4, 8, 8), 2, (4, 8, 8), (1, 1, 1), "the data grid's ratios, down"),
]


def case_id(c):
    return f"{c.B}x{c.C}-" + "x".join(map(str, c.src)) + "-" + "x".join(map(str, c.dst))


def expected(c):
    """(fwd, fwd tile, bwd, bwd tile, spans) of a row: what `route` must return for it"""
    return c.fwd, c.fwd_tile, c.bwd, c.bwd_tile, c.spans


def routed(c):
    r = route(c.B, c.C, c.src, c.dst)
    return r, (r.fwd, r.fwd_tiles.tile, r.bwd, None if r.bwd_tiles is None else r.bwd_tiles.tile, r.spans)


# the shapes of the tests that existed before this table (B, C, src, dst), for the coverage figures of docs/LAB_LOG.md
_TEST_RESIZE = [((13, 7, 6), (6, 3, 3)), ((6, 3, 3), (13, 7, 6)), ((12, 8, 9), (6, 4, 4)), ((6, 4, 4), (12, 8, 9)),
                ((3, 3, 3), (3, 3, 3)), ((5, 4, 3), (3, 3, 3)), ((3, 3, 3), (5, 4, 3))]
EARLIER = [(2, 16, s, d) for s, d in _TEST_RESIZE] + \
    [(2, 24, (5, 4, 3), (9, 9, 17)), (2, 8, (3, 3, 3), (20, 7, 30)), (2, 64, (13, 9, 10), (6, 4, 5)), (2, 512, (6, 4, 3), (3, 3, 3))]


def coverage(shapes):
    """what a list of (B, C, src, dst) reaches: the sets the coverage assertion and the lab log are written from"""
    seen = dict(fwd=set(), bwd=set(), pairs_at_64=set(), partial=set(), multi_partial_yz=False, multi_pass_fwd=set(),
                multi_pass_bwd=set(), gather_up=False, max_span=0)
    for B, C, src, dst in shapes:
        r = route(B, C, src, dst)
        seen["fwd"].add(r.fwd)
        seen["bwd"].add(r.bwd)
        if r.fwd == PAIRS and C == 64:
            seen["pairs_at_64"].add(r.fwd_tiles.tile)
        if r.fwd == GATHER:
            seen["gather_up"] |= all(o > i for i, o in zip(src, dst))
            if r.fwd_tiles.passes > 1:
                seen["multi_pass_fwd"].add(C)
        for t in (r.fwd_tiles, r.bwd_tiles):
            if t is not None:
                seen["partial"].add(t.partial)
                if t.partial[1] and t.partial[2] and t.count[1] >= 2 and t.count[2] >= 2:
                    seen["multi_partial_yz"] = True
        if r.bwd_tiles is not None:
            seen["max_span"] = max(seen["max_span"], r.spans[2])
            if r.bwd_tiles.passes > 1:
                seen["multi_pass_bwd"].add(C)
    return seen
