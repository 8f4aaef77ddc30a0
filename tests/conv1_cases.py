"""The host side of the 1x1 convolution family restated in Python, and the table of shapes tests/test_conv1_reference.py runs.

`fwd_route`, `gn_route` and `wgrad_route` repeat what conv1_route and conv1_wgrad_plan (csrc/tdx_conv1.hip) decide for tdx_conv1_fwd,
tdx_conv1_fwd_gn and the two weight-gradient entries; `plan_h`, `plan_f`, `plan_v` repeat the split rules of the three weight-gradient
kernels (conv1_wgrad_mfma_plan, conv1_wgrad_mfma_f32_plan, conv1_wgrad_vector_plan) and `det_plan` what conv1_wgrad_plan does with them
under TDX_DETERMINISTIC.  Pure functions: no GPU, no library -- the independent statement of the rules, which the library's own
answers (tdx_conv1_fwd_plan, tdx_conv1_bwd_weight_plan) are held against.

Routes: V = the vector-ALU kernels conv1_fwd_kernel<T> / conv1_wgrad_kernel<T> (64 x 64 tiles, any channel count, any T),
H = the 16-bit matrix-core kernels of tdx_conv1_mfma.hip (256-row tiles), F = the fp32 matrix-core kernels of
tdx_conv1_mfma_f32.hip (128-row forward tiles).  A route names the template instantiation too: `Route.kernel`.

Every row names the route and geometry it was written for; the CPU tests hold each row against the restated routing and the
GPU tests assert it again before they call the library, so that a later change of the routing fails the row instead of
quietly testing another kernel.  Shapes are the smallest that still reach the behaviour named in `why`.
"""

from collections import namedtuple

V, H, F = "V", "H", "F"
TILE_ROWS = {V: 64, F: 128, H: 256}  # forward tile heights: C1_BM, F1_ROWS, C1M_ROWS
H16 = ("bf16", "f16")
ARENA_HEAD, MAX_SLABS = 256, 256  # conv1_wgrad_plan: bytes skipped at the arena's head, most slabs
ARENA = 96 << 20  # the default TDX_SCRATCH_MB

Route = namedtuple("Route", "route kernel")


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- routing


def _mfma_ok(C1, C2, Cout):
    return C1 > 0 and C1 % 32 == 0 and C2 % 32 == 0 and Cout % 32 == 0


def fwd_route(dtype, C1, C2, Cout, ldw, col, add, direct=False):
    """conv1_route for tdx_conv1_fwd.  col: the first column of the weight block inside a 16-byte aligned matrix with rows of ldw floats (the
    pointer handed over is w + col: conv1_mfma_f32_supported wants it 16-byte aligned and ldw a multiple of 4)."""
    nt = 2 if Cout % 64 == 0 else 1
    if dtype in H16 and not direct and _mfma_ok(C1, C2, Cout):
        return Route(H, f"conv1_mfma_fwd_kernel<{nt},{dtype}>")
    if dtype == "f32" and not direct and _mfma_ok(C1, C2, Cout) and ldw % 4 == 0 and col % 4 == 0:
        return Route(F, f"conv1_f32_mfma_fwd_kernel<{nt},{int(bool(add))}>")
    return Route(V, f"conv1_fwd_kernel<{dtype}>")


def gn_route(dtype, C1, C2, Cout, direct=False):
    """tdx_conv1_fwd_gn: the kernel, or the error it returns (the caller then runs two launches)"""
    if dtype not in H16:
        return "TDX_EDTYPE"
    if direct or not _mfma_ok(C1, C2, Cout):
        return "TDX_ESHAPE"
    return Route(H, f"conv1_mfma_fwd_kernel<{2 if Cout % 64 == 0 else 1},{dtype}>")


def wgrad_route(dtype, Cin, Cout, transposed, direct=False):
    """conv1_wgrad_plan: the kernel"""
    ok = Cin % 32 == 0 and Cout % 32 == 0 and not direct
    tr, nt = int(bool(transposed)), 2 if Cout % 64 == 0 else 1
    if dtype in H16 and ok:
        return Route(H, f"conv1_wgrad_mfma_kernel<{2 if Cin % 64 == 0 else 1},{nt},{tr},{dtype}>")
    if dtype == "f32" and ok:
        return Route(F, f"conv1_f32_mfma_wgrad_kernel<{nt},{tr}>")
    return Route(V, f"conv1_wgrad_kernel<{dtype}>")


# --------------------------------------------------------------------------------------------------------- split planning

Plan = namedtuple("Plan", "nsplit steps")  # steps: loop trips (256-row chunks on H, 32-row slices on F and V) of every split


def plan_h(Cin, Cout, rows, max_split=0):
    """conv1_wgrad_mfma_plan: split s reduces the 256-row chunks s, s + nsplit, ..."""
    mt, nt = (2 if Cin % 64 == 0 else 1), (2 if Cout % 64 == 0 else 1)
    ntiles = (Cin // (32 * mt)) * (Cout // (32 * nt))
    nchunks = ceil_div(rows, 256)
    per_cu = 160 // ((mt + nt) * 16)
    nsplit = max(1, min(ceil_div(per_cu * 256, ntiles), nchunks))
    if max_split > 0:
        nsplit = min(nsplit, max_split)
    return Plan(nsplit, tuple(ceil_div(nchunks - s, nsplit) for s in range(nsplit)))


def _row_blocks(rows, per, nsplit):
    return Plan(nsplit, tuple(ceil_div(min(rows, (s + 1) * per) - s * per, 32) for s in range(nsplit)))


def plan_f(Cin, Cout, rows, max_split=0):
    """conv1_wgrad_mfma_f32_plan: split s reduces rows [s rps, (s + 1) rps) in 32-row slices"""
    nt = 2 if Cout % 64 == 0 else 1
    nsplit = min(ceil_div(1024, ceil_div(Cin, 128) * (Cout // (32 * nt))), ceil_div(rows, 256))
    if max_split > 0:
        nsplit = min(nsplit, max_split)
    nsplit = max(nsplit, 1)
    rps = ceil_div(ceil_div(rows, nsplit), 32) * 32
    return _row_blocks(rows, rps, ceil_div(rows, rps))


def plan_v(rows, max_split=0):
    """conv1_wgrad_vector_plan: 4096 rows per block, or ceil(rows / max_split) rounded up to the 32-row slice"""
    rpb = 4096
    if max_split > 0 and ceil_div(rows, rpb) > max_split:
        rpb = ceil_div(ceil_div(rows, max_split), 32) * 32
    return _row_blocks(rows, rpb, ceil_div(rows, rpb))


def plan(route, Cin, Cout, rows, max_split=0):
    return {H: plan_h, F: plan_f}[route](Cin, Cout, rows, max_split) if route != V else plan_v(rows, max_split)


def det_plan(route, Cin, Cout, rows, arena_bytes):
    """conv1_wgrad_plan under TDX_DETERMINISTIC: ("slabs", plan) when the arena holds two slabs or more, else
    ("single", plan with max_split = 1): one contributor per element straight into dw."""
    slab = ceil_div(Cin * Cout + Cout, 64) * 64
    room = (arena_bytes - ARENA_HEAD) // 4 // slab if arena_bytes > 0 else 0
    max_split = min(room, MAX_SLABS)
    if max_split >= 2:
        return "slabs", plan(route, Cin, Cout, rows, max_split)
    return "single", plan(route, Cin, Cout, rows, 1)


# ------------------------------------------------------------------------------------------------------------- the table

# dtypes: every storage format the row runs in (all take `route`); ldw / col: 0 / 0 = the compact matrix (ldw = Cout)
Fwd = namedtuple("Fwd", "name route dtypes C1 C2 Cout rows bias add ldw col direct why")


def _fwd(name, route, dtypes, C1, C2, Cout, rows, bias, add, why, ldw=0, col=0, direct=False):
    return Fwd(name, route, tuple(dtypes), C1, C2, Cout, rows, bias, add, ldw or Cout, col, direct, why)


ALL = ("f32", "bf16", "f16")
FWD = [
    # ---- V: 64-row x 64-column tiles, K slices of 32
    _fwd("v_4_4_r1", V, ALL, 4, 0, 4, 1, True, False, "Cin = 4, Cout = 4, one row: one thread row of one tile"),
    _fwd("v_seam_r63", V, ALL, 40, 24, 72, 63, True, True, "x1|x2 seam inside the second K slice; Cout = 72: a partial second column block; T - 1 rows"),
    _fwd("v_seam_r64", V, ALL, 40, 24, 72, 64, False, True, "exactly one row tile; no bias"),
    _fwd("v_seam_r65", V, ALL, 40, 24, 72, 65, True, False, "T + 1: a second row tile of one row; no add"),
    _fwd("v_4_72_r133", V, ALL, 4, 0, 72, 133, False, False, "2 T + 5 rows; neither bias nor add"),
    _fwd("v_direct_h", V, H16, 64, 64, 64, 133, True, True, "TDX_CONV1_IMPL=direct on a shape the 16-bit MFMA kernel would take", direct=True),
    _fwd("v_direct_f", V, ("f32",), 32, 96, 32, 65, True, True, "TDX_CONV1_IMPL=direct on a shape the fp32 MFMA kernel would take", direct=True),
    _fwd("v_dgrad_c6_x1", V, ALL, 64, 0, 6, 129, False, False, "data gradient of x1 of a layer with C1 = 6: Cout = 6, ldw = 38", ldw=38, col=0),
    _fwd("v_dgrad_c6_x2", V, ("f32",), 64, 0, 32, 129, False, False,
         "data gradient of x2 of a layer with C1 = 6: MFMA-eligible channels, but ldw = 38 and col = 6 fail the fp32 kernel's alignment clause", ldw=38, col=6),
    # ---- H: 256-row tiles, 32 NT columns per block
    _fwd("h_32_32_r1", H, H16, 32, 0, 32, 1, True, False, "NT = 1, one row"),
    _fwd("h_32+96_96_r255", H, H16, 32, 96, 96, 255, True, True, "NT = 1 with three column blocks; seam at a slice boundary; T - 1"),
    _fwd("h_64+64_64_r256", H, H16, 64, 64, 64, 256, False, True, "NT = 2; seam after two slices; exactly T; no bias"),
    _fwd("h_64+64_192_r257", H, H16, 64, 64, 192, 257, True, False, "NT = 2 with three column blocks; T + 1; no add"),
    _fwd("h_1024_32_r519", H, H16, 1024, 0, 32, 519, True, True, "Cin = 1024: 32 K slices; 2 T + 7 rows"),
    _fwd("h_32_160_r300", H, H16, 32, 0, 160, 300, True, True, "NT = 1 with five column blocks (Cout = 160)"),
    _fwd("h_same_as_v_direct_h", H, H16, 64, 64, 64, 133, True, True, "the shape, and so the tensors, of v_direct_h without the switch: two roundings where V gives one"),
    _fwd("h_dgrad_c6_x2", H, H16, 64, 0, 32, 257, False, False, "data gradient of x2 of a layer with C1 = 6: the MFMA kernel reads an unaligned w", ldw=38, col=6),
    _fwd("h_dgrad_x1", H, H16, 64, 0, 32, 129, False, False, "data gradient of x1 (32 + 64 -> 64): col = 0, ldw = 96 > Cout", ldw=96, col=0),
    _fwd("h_dgrad_x2", H, H16, 64, 0, 64, 129, False, True, "data gradient of x2: col = C1 = 32, ldw = 96; the addend of a fused block's backward", ldw=96, col=32),
    # ---- F: 128-row tiles
    _fwd("f_32_32_r1", F, ("f32",), 32, 0, 32, 1, True, False, "NT = 1 without add, one row"),
    _fwd("f_32+96_96_r127", F, ("f32",), 32, 96, 96, 127, True, True, "NT = 1 with add, three column blocks; T - 1"),
    _fwd("f_64+64_64_r128", F, ("f32",), 64, 64, 64, 128, False, True, "NT = 2 with add; exactly T; no bias"),
    _fwd("f_64+64_192_r129", F, ("f32",), 64, 64, 192, 129, True, False, "NT = 2 without add, three column blocks; T + 1"),
    _fwd("f_1024_32_r263", F, ("f32",), 1024, 0, 32, 263, True, True, "Cin = 1024; 2 T + 7 rows"),
    _fwd("f_32_160_r200", F, ("f32",), 32, 0, 160, 200, True, False, "NT = 1 with five column blocks"),
    _fwd("f_dgrad_x1", F, ("f32",), 64, 0, 32, 129, False, False, "data gradient, col = 0, ldw = 96", ldw=96, col=0),
    _fwd("f_dgrad_x2", F, ("f32",), 64, 0, 64, 129, False, True, "data gradient, col = C1 = 32 (a multiple of 4), ldw = 96", ldw=96, col=32),
]
SAME_INPUTS = ("v_direct_h", "h_same_as_v_direct_h")  # one set of tensors through V (one rounding) and through H (two)
FWD_INEXACT = ["v_seam_r65", "v_direct_h", "h_32+96_96_r255", "h_1024_32_r519", "h_dgrad_c6_x2", "f_64+64_64_r128", "f_1024_32_r263"]

# the fused tail y = silu(GroupNorm(h)) + bias + [x1 | x2] @ w (tdx_conv1_fwd_gn; H only).  A thread of the epilogue owns one
# 8-channel chunk and the rows tid / CHUNKS + i * 256 / CHUNKS: 32 apart at NT = 2 (64-channel passes), 64 apart at NT = 1
Tail = namedtuple("Tail", "name B V C1 C2 Cout G why")
TAIL = [
    Tail("t_v27", 12, 27, 64, 0, 64, 16, "V = 27 < 32: a thread's consecutive rows skip a whole sample; 9.5 samples in tile 0; 4 channels per group: a "
         "thread's chunk spans two groups; partial last tile"),
    Tail("t_v40", 7, 40, 32, 32, 32, 32, "NT = 1, two inputs; one channel per group; V = 40 < 64: rows 64 apart skip a sample"),
    Tail("t_v100", 4, 100, 32, 0, 96, 12, "NT = 1 with three column blocks; 8 channels per group; the partial last tile starts inside sample 2"),
    Tail("t_v256", 2, 256, 64, 64, 128, 1, "B V = 512 = two whole tiles, each exactly one sample; G = 1; NT = 2 with two column blocks; two inputs"),
    Tail("t_v300", 2, 300, 32, 0, 64, 16, "sample boundary inside tile 1, the partial last tile inside sample 1"),
]
TAIL_INEXACT = ["t_v27", "t_v100"]

# weight gradient: every row runs both entries (dw[ci][co] and dw[co][ci]), with and without dbias, accumulate 0 and 1,
# TDX_DETERMINISTIC unset and set.  steps / det_steps: the loop trips per split the restated planning gives (arena of 96 MiB)
Wgrad = namedtuple("Wgrad", "name route dtypes Cin Cout rows direct steps why")
WGRAD = [
    Wgrad("wv_40_72_r33", V, ALL, 40, 72, 33, False, (2,), "partial tiles in ci and co; a second 32-row slice of one row"),
    Wgrad("wv_6_4_r1", V, ALL, 6, 4, 1, False, (1,), "Cout = 4, one row"),
    Wgrad("wv_32_4_r257", V, H16, 32, 4, 257, False, (9,), "Cout = 4 keeps MFMA-eligible Cin on the vector kernel"),
    Wgrad("wv_40_72_r4097", V, ("f32", "bf16"), 40, 72, 4097, False, (128, 1), "rows > 4096: a second row block of one row"),
    Wgrad("wv_direct", V, ("f32", "bf16"), 64, 64, 255, True, (8,), "TDX_CONV1_IMPL=direct on an MFMA-eligible shape"),
    Wgrad("wh_32_32_r1", H, H16, 32, 32, 1, False, (1,), "MT = NT = 1, one row"),
    Wgrad("wh_64_32_r31", H, H16, 64, 32, 31, False, (1,), "MT = 2, NT = 1"),
    Wgrad("wh_32_64_r33", H, H16, 32, 64, 33, False, (1,), "MT = 1, NT = 2"),
    Wgrad("wh_64_64_r255", H, H16, 64, 64, 255, False, (1,), "MT = NT = 2; one row short of a chunk"),
    Wgrad("wh_96_160_r256", H, H16, 96, 160, 256, False, (1,), "MT = NT = 1 with 3 x 5 tiles; exactly one chunk"),
    Wgrad("wh_128_64_r257", H, H16, 128, 64, 257, False, (1, 1), "two ci tiles; a second chunk of one row, one chunk per split"),
    Wgrad("wh_64_192_r32", H, H16, 64, 192, 32, False, (1,), "three co tiles; 32 rows"),
    Wgrad("wh_1024_1024_r600", H, H16, 1024, 1024, 600, False, (2, 1), "256 tiles: nsplit = 2 < 3 chunks: split 0 pipelines two chunks, split 1 one"),
    Wgrad("wh_32_32_r2305", H, H16, 32, 32, 2305, False, (1,) * 10, "one tile: ten splits, ten contributors per element: what the two deterministic runs of "
          "the Gaussian rows compare is then an order of ten additions (the atomics' arrival order, were the slabs not used)"),
    Wgrad("wf_32_32_r1", F, ("f32",), 32, 32, 1, False, (1,), "NT = 1; three of four waves inactive"),
    Wgrad("wf_32_64_r31", F, ("f32",), 32, 64, 31, False, (1,), "NT = 2"),
    Wgrad("wf_160_32_r33", F, ("f32",), 160, 32, 33, False, (2,), "Cin = 160: the second ci block has one active wave; two slices"),
    Wgrad("wf_256_64_r255", F, ("f32",), 256, 64, 255, False, (8,), "Cin = 256: two full ci blocks"),
    Wgrad("wf_160_96_r256", F, ("f32",), 160, 96, 256, False, (8,), "three co blocks at NT = 1"),
    Wgrad("wf_64_64_r257", F, ("f32",), 64, 64, 257, False, (5, 4), "two splits; the last slice holds one row"),
    Wgrad("wf_32_32_r32", F, ("f32",), 32, 32, 32, False, (1,), "exactly one slice"),
    Wgrad("wf_32_32_r1793", F, ("f32",), 32, 32, 1793, False, (8,) * 7 + (1,), "8 splits of 256 rows: seven pipeline 8 slices, the last has one row"),
]
WGRAD_INEXACT = ["wv_40_72_r33", "wh_128_64_r257", "wh_1024_1024_r600", "wh_32_32_r2305", "wf_160_32_r33", "wf_64_64_r257", "wf_32_32_r1793"]
NO_ARENA = ["wv_40_72_r4097", "wh_1024_1024_r600", "wf_32_32_r1793"]  # TDX_DETERMINISTIC without an arena: the single-split branch
NO_ARENA_STEPS = {"wv_40_72_r4097": (129,), "wh_1024_1024_r600": (3,), "wf_32_32_r1793": (57,)}

# layers run through ops.conv1 and autograd: (C1, C2, Cout, rows, bias)
LAYERS = [(6, 32, 64, 257, True), (32, 64, 64, 129, True), (40, 24, 72, 65, False), (64, 0, 96, 300, True)]


def by_name(table, name):
    return next(c for c in table if c.name == name)
