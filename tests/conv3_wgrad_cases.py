"""The case table of tests/test_conv3_wgrad_reference.py: every kernel of tdx_conv3_bwd_weight, every merge, at the smallest
shapes at which each can still go wrong.  A row names its kernel and the plan it expects (tile width, brick depth, K splits,
slabs or atomics, which unpack) and the environment it needs; `plan` restates the host planning rules of csrc/
tdx_conv3_entry.hip and the seven *_plan functions in Python, and the tests hold every row against that restatement AND against
the library's own answer (tdx_conv3_bwd_weight_plan), with an arena bound and without one.

Limits of a row: B X Y Z <= 20 000 voxels and 27 rows Cin Cout <= 3e9 (the float64 reference stays around a second).
"""

from collections import namedtuple

F32, BF16, F16 = 0, 1, 3                      # TDX_F32 / TDX_BF16 / TDX_F16
AUTO, DIRECT, MFMA, SPLIT = 0, 1, 2, 3        # TDX_CONV_*
CODE = {"f32": F32, "bf16": BF16, "f16": F16}
H16 = ("bf16", "f16")
OK, EINVAL, ESHAPE, EDTYPE = 0, -1, -2, -3
KERNELS = ("direct", "brick16", "small", "ring", "brick_f32", "split", "split_ring")

# the library's switches a plan reads, at their defaults
ENV = {"TDX_DETERMINISTIC": 0, "TDX_WGRAD_RING": 1, "TDX_WGRAD_SMALL": 1, "TDX_WGRAD_SMALL_ROWS": 8000, "TDX_WGRAD_SPLIT_RING": 1,
       "TDX_CONV3_PERM": 1, "TDX_PERSISTENT_CUS": 256}

Plan = namedtuple("Plan", "status kernel tile depth nsplit nslab sum_unpack nbg xs gx ngroups max_slabs nbricks order",
                  defaults=(0,) * 7)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- the host rules, restated


def slab_capacity(Cin, Cout):
    """w3_slab_capacity: per-split slabs a workspace holds"""
    return max(8, min(512, (1 << 19) // (Cin * Cout)))


def h16_supported(C1, C2, Cout):
    return C1 > 0 and (C1 % 32 == 0 or (C2 == 0 and C1 % 16 == 0)) and C2 % 32 == 0 and Cout % 32 == 0


def f32_supported(C1, C2, Cout):  # conv3_wgrad_mfma_f32_supported and conv3_wgrad_mfma_split_supported: the same rule
    return C1 > 0 and (C1 % 32 == 0 or (C2 == 0 and C1 % 8 == 0)) and C2 % 32 == 0 and Cout % 32 == 0


PERMS = ((0, 1, 2), (1, 0, 2), (2, 0, 1))


def view(grid, bx, permute=True):
    """conv3_wgrad_view_order and conv3_wgrad_view: (index of the axis order chosen, bricks per sample) for bricks of
    bx x 8 x 8 -- the first order that leaves the fewest bricks"""
    best = None
    for k, perm in enumerate(PERMS if permute else PERMS[:1]):
        n = cdiv(grid[perm[0]], bx) * cdiv(grid[perm[1]], 8) * cdiv(grid[perm[2]], 8)
        if best is None or n < best[1]:
            best = (k, n)
    return best


def _merge(nsplit, max_slabs, det):
    """conv3_wgrad_plan_merge: (nsplit, nslab)"""
    if det and nsplit > max_slabs:
        nsplit = max_slabs if max_slabs > 0 else 1
    return nsplit, (nsplit if nsplit <= max_slabs else 0)


def small_geom(C1, C2, Cout, B, grid, env):
    """ws_geom of tdx_conv3_wgrad_small.hip: (nbg, xs, gx, ngroups, shrunk) or None"""
    X, Y, Z = grid
    Cin = C1 + C2
    if not env["TDX_WGRAD_SMALL"] or C1 % 32 or C2 % 32 or Cout % 32 or Cin < 128:
        return None
    if B * X * Y * Z > env["TDX_WGRAD_SMALL_ROWS"]:
        return None
    plane, V = Y * Z, X * Y * Z
    if plane > 256:
        return None
    if V <= 256:
        nbg, xs, gx = min(B, 256 // V), X, 1
    else:
        nbg, xs, gx = 1, 256 // plane, cdiv(X, 256 // plane)
    NT = 2 if Cout % 64 == 0 else 1

    def lds():
        entries = nbg * (xs + 2) * (Y + 2) * (Z + 2)
        xbytes = cdiv(entries * 64, 1024) * 1024
        grows = cdiv(nbg * xs * plane, 16) * 16
        return 2 * xbytes + 2 * NT * grows * 64 + (256 + xbytes // 64) * 4

    shrunk = False
    while lds() > 160 * 1024 and (nbg > 1 or xs > 1):
        shrunk = True
        if nbg > 1:
            nbg -= 1
        else:
            xs -= 1
            gx = cdiv(X, xs)
    if lds() > 160 * 1024:
        return None
    return nbg, xs, gx, cdiv(B, nbg) * gx, shrunk


def _persistent_split(ntiles, nbricks, env):
    cus = env["TDX_PERSISTENT_CUS"] & ~7
    nsplit = cdiv(256, ntiles) if cus >= 256 else max(cus // ntiles, 1)
    return max(1, min(nsplit, nbricks))


def plan(dtype, impl, C1, C2, Cout, B, grid, env=None, arena=True):
    """conv3_wgrad_plan: what tdx_conv3_bwd_weight launches.  dtype: "f32" / "bf16" / "f16" (any other name: a dtype code
    the library does not know); env: switch values that differ from ENV; arena: whether a scratch arena is bound."""
    env = {**ENV, **(env or {})}
    X, Y, Z = grid
    refuse = lambda s: Plan(s, "direct", 0, 0, 0, 0, 0)
    if not (B > 0 and X > 0 and Y > 0 and Z > 0 and C1 > 0 and C2 >= 0 and Cout > 0):
        return refuse(EINVAL)
    if C1 % 8 or C2 % 8 or Cout % 8:
        return refuse(ESHAPE)
    Cin, det, h16 = C1 + C2, bool(env["TDX_DETERMINISTIC"]), dtype in H16
    cap = slab_capacity(Cin, Cout)
    if dtype == "f32" and impl == SPLIT and f32_supported(C1, C2, Cout):
        fam = "split"
    elif dtype == "f32" and impl != DIRECT and f32_supported(C1, C2, Cout):
        fam = "f32"
    elif impl == MFMA or (impl == AUTO and h16 and h16_supported(C1, C2, Cout)):
        if not h16:
            return refuse(EDTYPE)
        if not h16_supported(C1, C2, Cout):
            return refuse(ESHAPE)
        fam = "h16"
    else:
        fam = "direct"

    def done(kernel, tile, depth, nsplit, max_slabs, bricks=(0, 0), small=(0, 0, 0, 0)):
        nsplit, nslab = _merge(nsplit, max_slabs, det)
        return Plan(OK, kernel, tile, depth, nsplit, nslab, int(nslab > 8), *small, max_slabs, B * bricks[1], bricks[0])

    if fam == "direct":
        if dtype not in CODE:
            return refuse(EDTYPE)
        max_slabs = min(cap, 64) if det else 0
        nvox = B * X * Y * Z
        vpb = cdiv(cdiv(nvox, max_slabs), 32) * 32 if max_slabs else 8192
        chunks = cdiv(nvox, vpb)
        return Plan(OK, "direct", 0, 0, chunks, chunks if max_slabs else 0, 0, 0, 0, 0, 0, max_slabs, 0)
    max_slabs = 8 if (fam != "h16" and not det) else cap
    n_ci = cdiv(Cin, 32)
    if fam == "split":
        ntiles = n_ci * (Cout // 32)
        if env["TDX_WGRAD_SPLIT_RING"]:
            v = view(grid, 2)
            nsplit = _persistent_split(ntiles, B * v[1], env)
            if B * v[1] >= 4 * nsplit:
                return done("split_ring", 1, 2, nsplit, max_slabs, v)
        v = view(grid, 4)
        return done("split", 1, 4, max(1, min(cdiv(256, ntiles), B * v[1])), max_slabs, v)
    NT = 2 if Cout % 64 == 0 else 1
    ntiles = n_ci * (Cout // (32 * NT))
    if fam == "f32":
        depth = 2 if NT == 2 else 4
        v = view(grid, depth)
        return done("brick_f32", NT, depth, max(1, min(cdiv(256, ntiles), B * v[1])), max_slabs, v)
    g = small_geom(C1, C2, Cout, B, grid, env)
    if g is not None:
        return done("small", NT, 0, max(1, min(g[3], cdiv(256, ntiles))), max_slabs, (0, 0), g[:4])
    ring = env["TDX_WGRAD_RING"]
    if ring and arena and not (NT == 1 and ring == 2):
        v = view(grid, 4)
        nsplit = _persistent_split(ntiles, B * v[1], env)
        if B * v[1] >= 4 * nsplit:
            return done("ring", NT, 4, nsplit, max_slabs, v)
    v = view(grid, 4, bool(env["TDX_CONV3_PERM"]))
    return done("brick16", NT, 4, max(1, min(cdiv(256 if NT == 2 else 512, ntiles), B * v[1])), max_slabs, v)


# --------------------------------------------------------------------------------------------------------------- the table

# kernel: the kernel the row is for; tile / depth / nsplit / nslab (0: atomics) / sum_unpack: the plan it expects (with the
# arena bound unless arena is False).  dtypes: storage formats the row runs in.  impl: TDX_CONV_*; env: switches set for the row (all others
# unset); bias False: dbias = NULL.  Every row runs the exact families of its storage format (`families`) and Gaussian inputs.
Case = namedtuple("Case", "name kernel dtypes impl C1 C2 Cout B grid env tile depth nsplit nslab sum_unpack arena bias",
                  defaults=(True, True))

NO_SIDE = {"TDX_WGRAD_RING": "0", "TDX_WGRAD_SMALL_ROWS": "0"}  # ring and small refused through their switches
DET = {"TDX_DETERMINISTIC": "1"}
CUS8 = {"TDX_PERSISTENT_CUS": "8"}


def families(dname):
    """The exact input families (conv3_wgrad_reference.FAMILIES) a row runs in this storage format: the wide families are
    float32 tensors, and every float32 run of every row takes them -- no row is too large (at most 8232 voxels)."""
    return ("ints", "wide-x", "wide-dy") if dname == "f32" else ("ints",)


CASES = [
    # ---- brick16: 4 x 8 x 8 bricks; ring / small refused by shape (Cin < 128, fewer than 4 nsplit bricks) unless NO_SIDE
    Case("b16_one_brick", "brick16", H16, AUTO, 32, 0, 32, 1, (4, 8, 8), {}, 1, 4, 1, 1, 0),
    Case("b16_partial_two_inputs_3co", "brick16", H16, AUTO, 32, 32, 96, 1, (5, 9, 9), {}, 1, 4, 6, 6, 0),
    Case("b16_perm_z_first", "brick16", H16, AUTO, 32, 0, 64, 1, (16, 8, 4), {}, 2, 4, 2, 2, 0),
    Case("b16_perm_y_first", "brick16", H16, AUTO, 64, 0, 32, 1, (8, 4, 16), {}, 1, 4, 2, 2, 0),
    Case("b16_perm_off", "brick16", ("bf16",), AUTO, 64, 0, 32, 1, (8, 4, 16), {"TDX_CONV3_PERM": "0"}, 1, 4, 4, 4, 0),
    Case("b16_half_ci_tile", "brick16", H16, AUTO, 16, 0, 64, 2, (5, 9, 9), {}, 2, 4, 12, 12, 1),
    Case("b16_prefetch_256", "brick16", H16, AUTO, 256, 0, 256, 1, (9, 9, 17), NO_SIDE, 2, 4, 8, 8, 0),
    Case("b16_thin_axes", "brick16", H16, AUTO, 32, 0, 32, 2, (5, 3, 1), {}, 1, 4, 2, 2, 0),
    Case("b16_extent_2", "brick16", ("bf16",), MFMA, 32, 0, 32, 1, (2, 9, 5), {}, 1, 4, 2, 2, 0, True, False),
    # ---- small: packed K, row groups of up to 256 voxels
    Case("small_ragged_group_shrunk", "small", H16, AUTO, 128, 0, 32, 23, (5, 3, 1), {}, 1, 0, 3, 3, 0),
    Case("small_one_per_group", "small", H16, AUTO, 256, 0, 96, 3, (7, 9, 4), {}, 1, 0, 3, 3, 0),
    Case("small_x_slabs", "small", H16, AUTO, 160, 0, 64, 1, (13, 7, 6), {}, 2, 0, 3, 3, 0),
    Case("small_two_inputs_x_slabs", "small", H16, AUTO, 128, 128, 64, 2, (5, 13, 11), {}, 2, 0, 10, 10, 1),
    Case("small_groups_of_4", "small", ("bf16",), AUTO, 128, 0, 64, 7, (4, 4, 3), {}, 2, 0, 2, 2, 0, True, False),
    # ---- ring: producer / consumer, needs the arena; both branches of its split rule
    Case("ring_cus256_half_ci_ragged", "ring", H16, AUTO, 16, 0, 256, 43, (5, 9, 9), {}, 2, 4, 64, 64, 1),
    Case("ring_cus256_two_inputs_nt1", "ring", H16, AUTO, 32, 32, 96, 29, (5, 9, 9), {}, 1, 4, 43, 43, 1),
    Case("ring_cus8_whole_bricks", "ring", H16, AUTO, 32, 0, 64, 1, (16, 16, 32), CUS8, 2, 4, 8, 8, 0),
    Case("ring_cus8_32_bricks", "ring", ("bf16",), AUTO, 32, 0, 32, 32, (4, 8, 8), CUS8, 1, 4, 8, 8, 0),
    Case("ring_one_brick_short", "brick16", ("bf16",), AUTO, 32, 0, 32, 31, (4, 8, 8), CUS8, 1, 4, 31, 31, 1),
    Case("ring_without_arena", "brick16", ("bf16",), AUTO, 32, 0, 64, 1, (16, 16, 32), CUS8, 2, 4, 32, 32, 1, False),
    # ---- brick_f32: fp32-IEEE products; NT = 1 on 4 x 8 x 8, NT = 2 on 2 x 8 x 8; 8 slabs, else atomics
    Case("f32_nt1_half_ci_tile", "brick_f32", ("f32",), AUTO, 24, 0, 32, 1, (5, 9, 9), {}, 1, 4, 6, 6, 0),
    Case("f32_nt2_half_ci_atomics", "brick_f32", ("f32",), AUTO, 8, 0, 64, 1, (9, 9, 17), {}, 2, 2, 30, 0, 0),
    Case("f32_two_inputs_3co", "brick_f32", ("f32",), AUTO, 32, 32, 96, 2, (5, 9, 9), {}, 1, 4, 12, 0, 0),
    Case("f32_deterministic", "brick_f32", ("f32",), AUTO, 8, 0, 64, 1, (9, 9, 17), DET, 2, 2, 30, 30, 1),
    # ---- split precision: single-role (4 x 8 x 8) and producer / consumer (2 x 8 x 8), both sides of its 4 nsplit rule
    Case("split_single_half_ci", "split", ("f32",), SPLIT, 8, 0, 32, 1, (5, 9, 9), {}, 1, 4, 6, 6, 0),
    Case("split_single_two_inputs", "split", ("f32",), SPLIT, 32, 32, 64, 3, (5, 9, 9), {}, 1, 4, 18, 0, 0),
    Case("split_ring_cus256", "split_ring", ("f32",), SPLIT, 128, 0, 128, 8, (3, 9, 9), {}, 1, 2, 16, 0, 0),
    Case("split_ring_cus8_32_bricks", "split_ring", ("f32",), SPLIT, 24, 0, 32, 32, (2, 8, 8), CUS8, 1, 2, 8, 8, 0),
    Case("split_ring_one_brick_short", "split", ("f32",), SPLIT, 24, 0, 32, 31, (2, 8, 8), CUS8, 1, 4, 31, 0, 0),
    Case("split_ring_switched_off", "split", ("f32",), SPLIT, 32, 32, 32, 2, (16, 16, 16), {"TDX_WGRAD_SPLIT_RING": "0"}, 1, 4, 32, 0, 0),
    Case("split_ring_deterministic", "split_ring", ("f32",), SPLIT, 32, 32, 32, 2, (16, 16, 16), {**DET, **CUS8}, 1, 2, 4, 4, 0),
    # ---- direct: the vector ALU, every dtype; a channel count no MFMA kernel takes, and TDX_CONV_DIRECT on one they do
    Case("direct_unsupported_channels", "direct", ("f32", "bf16", "f16"), AUTO, 8, 0, 40, 2, (5, 9, 9), {}, 0, 0, 1, 0, 0),
    Case("direct_two_inputs_asked", "direct", ("f32", "bf16", "f16"), DIRECT, 32, 32, 32, 1, (5, 9, 9), {}, 0, 0, 1, 0, 0),
    Case("direct_two_chunks", "direct", ("f32",), DIRECT, 8, 0, 8, 3, (14, 14, 14), {}, 0, 0, 2, 0, 0),
    Case("direct_deterministic", "direct", ("f32", "bf16"), AUTO, 8, 0, 40, 2, (5, 9, 9), DET, 0, 0, 26, 26, 0),
    # ---- merges of the 16-bit kernels: ceil rounding puts nsplit one above the slab capacity (atomics); held to it when
    # deterministic
    Case("b16_atomics_171_splits", "brick16", H16, AUTO, 96, 0, 32, 29, (5, 9, 9), {"TDX_WGRAD_RING": "0"}, 1, 4, 171, 0, 0),
    Case("b16_deterministic_170", "brick16", ("bf16",), AUTO, 96, 0, 32, 29, (5, 9, 9), {"TDX_WGRAD_RING": "0", **DET}, 1, 4, 170, 170, 1),
    Case("small_deterministic", "small", ("bf16",), AUTO, 256, 0, 96, 3, (7, 9, 4), DET, 1, 0, 3, 3, 0),
    Case("ring_deterministic", "ring", ("bf16",), AUTO, 32, 32, 96, 29, (5, 9, 9), DET, 1, 4, 43, 43, 1),
]

# one row per kernel that also goes through ops.conv3(...).backward
AUTOGRAD = ("b16_partial_two_inputs_3co", "small_one_per_group", "ring_cus8_whole_bricks", "f32_nt1_half_ci_tile", "split_single_half_ci",
            "split_ring_cus8_32_bricks", "direct_unsupported_channels")
# rows that run TDX_WS_CLEAN twice on one persistent zeroed workspace
WS_CLEAN_TWICE = ("b16_one_brick", "small_x_slabs", "ring_cus8_32_bricks", "f32_nt2_half_ci_atomics", "split_single_two_inputs",
                  "split_ring_cus8_32_bricks", "direct_unsupported_channels", "b16_atomics_171_splits")
# rows the planted defects of the reference are shown on
DEFECTS = ("b16_partial_two_inputs_3co", "small_two_inputs_x_slabs", "ring_cus256_two_inputs_nt1", "split_single_two_inputs", "b16_thin_axes")


def by_name(name):
    return next(c for c in CASES if c.name == name)


def case_env(c):
    """the row's switches as `plan` takes them"""
    return {k: int(v) for k, v in c.env.items()}


def case_plan(c, dtype, arena=None):
    return plan(dtype, c.impl, c.C1, c.C2, c.Cout, c.B, c.grid, case_env(c), c.arena if arena is None else arena)


# ---- the shipped model's layers (the shapes of _CONV3_ROUTES in test_abi_and_host.py: the test holds the two lists together)
# in the modes that test uses: the plan the library of the change that added the query gave, recorded from it.  This pin
# freezes current behaviour; it is not a comparison with a reference.
PIN_MODES = (("bf16", AUTO), ("f16", AUTO), ("f32", AUTO), ("f32", SPLIT), ("bf16", DIRECT), ("f32", DIRECT))
# per shape (C1, C2, Cout, B, X, Y, Z): the plans without an arena, then with one; one word per mode of PIN_MODES:
# kernel:tile:depth:nsplit:nslab:sum_unpack, or E<status> where the call is refused
PIN = {
    (64, 0, 64, 6, 192, 64, 48): (
        "brick16:2:4:128:128:1 brick16:2:4:128:128:1 brick_f32:2:2:128:0:0 split_ring:1:2:64:0:0 direct:0:0:432:0:0 direct:0:0:432:0:0",
        "ring:2:4:128:128:1 ring:2:4:128:128:1 brick_f32:2:2:128:0:0 split_ring:1:2:64:0:0 direct:0:0:432:0:0 direct:0:0:432:0:0"),
    (64, 64, 64, 6, 192, 64, 48): (
        "brick16:2:4:64:64:1 brick16:2:4:64:64:1 brick_f32:2:2:64:0:0 split_ring:1:2:32:0:0 direct:0:0:432:0:0 direct:0:0:432:0:0",
        "ring:2:4:64:64:1 ring:2:4:64:64:1 brick_f32:2:2:64:0:0 split_ring:1:2:32:0:0 direct:0:0:432:0:0 direct:0:0:432:0:0"),
    (128, 0, 128, 6, 96, 32, 24): (
        "brick16:2:4:32:32:1 brick16:2:4:32:32:1 brick_f32:2:2:32:0:0 split_ring:1:2:16:0:0 direct:0:0:54:0:0 direct:0:0:54:0:0",
        "ring:2:4:32:32:1 ring:2:4:32:32:1 brick_f32:2:2:32:0:0 split_ring:1:2:16:0:0 direct:0:0:54:0:0 direct:0:0:54:0:0"),
    (256, 0, 256, 6, 48, 16, 12): (
        "brick16:2:4:8:8:0 brick16:2:4:8:8:0 brick_f32:2:2:8:8:0 split_ring:1:2:4:4:0 direct:0:0:7:0:0 direct:0:0:7:0:0",
        "ring:2:4:8:8:0 ring:2:4:8:8:0 brick_f32:2:2:8:8:0 split_ring:1:2:4:4:0 direct:0:0:7:0:0 direct:0:0:7:0:0"),
    (512, 0, 512, 6, 24, 8, 6): (
        "small:2:0:2:2:0 small:2:0:2:2:0 brick_f32:2:2:2:2:0 split_ring:1:2:1:1:0 direct:0:0:1:0:0 direct:0:0:1:0:0",
        "small:2:0:2:2:0 small:2:0:2:2:0 brick_f32:2:2:2:2:0 split_ring:1:2:1:1:0 direct:0:0:1:0:0 direct:0:0:1:0:0"),
    (512, 0, 512, 6, 12, 4, 3): (
        "small:2:0:2:2:0 small:2:0:2:2:0 brick_f32:2:2:2:2:0 split_ring:1:2:1:1:0 direct:0:0:1:0:0 direct:0:0:1:0:0",
        "small:2:0:2:2:0 small:2:0:2:2:0 brick_f32:2:2:2:2:0 split_ring:1:2:1:1:0 direct:0:0:1:0:0 direct:0:0:1:0:0"),
    (512, 512, 256, 6, 24, 8, 6): (
        "small:2:0:2:2:0 small:2:0:2:2:0 brick_f32:2:2:2:2:0 split_ring:1:2:1:1:0 direct:0:0:1:0:0 direct:0:0:1:0:0",
        "small:2:0:2:2:0 small:2:0:2:2:0 brick_f32:2:2:2:2:0 split_ring:1:2:1:1:0 direct:0:0:1:0:0 direct:0:0:1:0:0"),
    (64, 0, 64, 6, 194, 50, 50): (
        "brick16:2:4:128:128:1 brick16:2:4:128:128:1 brick_f32:2:2:128:0:0 split_ring:1:2:64:0:0 direct:0:0:356:0:0 direct:0:0:356:0:0",
        "ring:2:4:128:128:1 ring:2:4:128:128:1 brick_f32:2:2:128:0:0 split_ring:1:2:64:0:0 direct:0:0:356:0:0 direct:0:0:356:0:0"),
    (128, 0, 128, 6, 97, 25, 25): (
        "brick16:2:4:32:32:1 brick16:2:4:32:32:1 brick_f32:2:2:32:0:0 split_ring:1:2:16:0:0 direct:0:0:45:0:0 direct:0:0:45:0:0",
        "ring:2:4:32:32:1 ring:2:4:32:32:1 brick_f32:2:2:32:0:0 split_ring:1:2:16:0:0 direct:0:0:45:0:0 direct:0:0:45:0:0"),
    (8, 0, 8, 2, 48, 32, 32): (
        "direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0",
        "direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0 direct:0:0:12:0:0"),
    (4, 0, 64, 6, 192, 64, 48): (
        "E-2 E-2 E-2 E-2 E-2 E-2",
        "E-2 E-2 E-2 E-2 E-2 E-2"),
}


def pin_word(p):
    """a plan (dict of the library's query) as its word of PIN"""
    return f"E{p['status']}" if p["status"] else ":".join(str(p[k]) for k in ("kernel", "tile", "depth", "nsplit", "nslab", "sum_unpack"))
