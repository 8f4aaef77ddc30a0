"""The bits of the forward / data-gradient 3x3x3 conv kernels that tile the grid in bricks -- csrc/tdx_conv3_mfma.hip (16-bit),
tdx_conv3_mfma_f32.hip (fp32 IEEE), tdx_conv3_mfma_split*.hip (split precision) -- and of the ring kernel's remainder slabs
(tdx_conv3_ring.hip + the thin-brick kernel): the cases shared by tests/test_conv3_bits.py and tests/golden/make_golden_bits.py.

`run(group)` calls the C ABI through `turbdiff_amd._lib` for every case of the group and returns one record per case
(tests/pinned_bits.py).  A case's outputs are y (tdx_conv3_fwd, with bias), y of tdx_conv3_fwd_gn, and dx1 | dx2 of
tdx_conv3_bwd_data and of tdx_conv3_bwd_data_add (with addends), the data gradient under TDX_SHELL_DETERMINISTIC=1 so that the
halo-shell term is added in a fixed order.  The fused statistics are NOT pinned: their f64 atomics arrive in any order.
Inputs are seeded CPU draws; only digests are stored, and beside them the raw bits of the first 4 voxels of sample 0 (ring group:
the 8 voxels of its far corner, where the three remainder slabs meet) at each group's smallest shape, at the narrowest channels
whose forward AND data gradient run on the brick kernels (NARROW_DX).

Every case asserts through tdx_conv3_fwd_kernel that the kernel family it was chosen for serves it, the forward as called and
the data gradient as the conv Cout -> Cin it is routed as.  `plan16` / `plan32` / `bricks` restate in Python the host planning
rules the shapes were chosen against; tests/test_conv3_bits.py holds the comments of this table to those restatements (a check
of the table's arithmetic, not of the host code: the library does not report its plans).
"""

import contextlib
import os

import torch

from pinned_bits import record
from step_inputs import rnd

FIXTURE = "conv3_bits.json"
H16 = {"bf16": torch.bfloat16, "f16": torch.float16}
FWD = [(C1, C2, Co) for C1, C2 in ((16, 0), (32, 16)) for Co in (32, 64, 96)]  # Co: NT = 1, NT = 2, three N tiles
# The data gradient's N is Cin = C1 + C2, and the brick kernels serve it only where Cin % 32 == 0: at the inputs above (Cin = 16,
# 48) dx comes from the vector-ALU kernel + fold (_conv_case asserts which).  So, for dx on the brick kernels: Cin = 32 as one
# tensor (NT = 1, no d2) and as d1 | d2 inside one N tile, Cin = 64 (NT = 2, the tile straddles d1 | d2), Cin = 96 (three N tiles)
DGRAD = [(32, 0, 32), (16, 16, 32), (32, 32, 32), (64, 32, 32)]
CHANNELS = FWD + DGRAD
NARROW = (16, 0, 32)
NARROW_DX = (32, 0, 32)
# (B, grid) of the brick groups -> what the 16-bit planning rule makes of it: (main permutation, thin slabs per axis)
SMALL = {
    (2, (4, 8, 8)): ((0, 1, 2), (False, False, False)),   # exactly one brick; raw bits stored
    (2, (5, 9, 9)): ((1, 0, 2), (False, False, False)),   # partial bricks on every axis (6 bricks against 8 unpermuted)
    (2, (16, 8, 4)): ((2, 0, 1), (False, False, False)),  # the brick's short edge along z
    (2, (8, 4, 16)): ((1, 0, 2), (False, False, False)),  # ... along y
}
THIN16 = (1, (62, 33, 34))   # 69564 voxels >= 60000: thin slabs on all three axes, forward and data gradient
THIN32 = (3, (66, 33, 34))   # fp32 kernels: 3 * 17 * 5 * 5 = 1275 >= 1024 bricks: thin slabs in the data gradient
BIG = (2, (64, 64, 64))      # split kernel: 2 * 8^3 = 1024 big (8 x 8 x 8) bricks at 32 output channels
PARTIAL = (2, (5, 9, 9))
# ring kernel + remainder slabs on the thin-brick kernel: (B, C1, C2, Cout, grid, brick depth), the ragged rows of
# test_conv3_ring_kernel_vs_brick_kernel
RING = [(2, 32, 0, 32, (34, 17, 9), 8), (2, 32, 32, 64, (24, 17, 16), 8), (1, 64, 0, 64, (50, 26, 18), 8),
        (1, 64, 0, 64, (34, 17, 14), 4)]
GROUPS = ["brick16/bf16", "brick16/f16", "partial/bf16", "partial/f16", "ring_slabs/bf16", "ring_slabs/f16",
          "f32/auto", "f32/split", "f32_thin/auto", "f32_thin/split", "split_big"]


def bricks(ext, perm, dims=(4, 8, 8)):
    n = 1
    for k in range(3):
        n *= -(-ext[perm[k]] // dims[k])
    return n


def plan16(grid, force_thin=False):
    """(main permutation, thin slab per axis) of the 16-bit brick kernel's planning rule for a plain call."""
    big = force_thin or grid[0] * grid[1] * grid[2] >= 60000
    thin = tuple(big and 1 <= grid[a] % (4, 8, 8)[a] <= 2 and grid[a] > (4, 8, 8)[a] for a in range(3))
    main = [grid[a] - grid[a] % (4, 8, 8)[a] if thin[a] else grid[a] for a in range(3)]
    return min(((0, 1, 2), (1, 0, 2), (2, 0, 1)), key=lambda p: bricks(main, p)), thin


def plan32(B, grid, data_gradient, dims=(4, 8, 8)):
    """thin slab per axis of brick_plan (fp32 and split kernels)."""
    full = B * bricks(grid, (0, 1, 2))
    return tuple(data_gradient and full >= 1024 and 1 <= grid[a] % dims[a] <= 2 and grid[a] > dims[a] for a in range(3))


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Lib:
    """Calls with the launching stream's arena bound (L.call), or with no arena at all."""

    def __init__(self, L, arena):
        self.L, self.arena = L, arena

    def _unbind(self):
        self.L._ACTIVE = None  # the next L.call binds its arena again
        rc = self.L.load().tdx_set_scratch(None, 0)
        assert rc == 0, rc

    def call(self, name, *args):
        if self.arena:
            return self.L.call(name, *args)
        with self.L._LAUNCH_LOCK:
            self._unbind()
            rc = getattr(self.L.load(), name)(*args)
        assert rc == 0, (name, rc)

    def family(self, C1, C2, Co, B, grid, code, impl):
        with self.L._LAUNCH_LOCK:
            if self.arena:
                self.L.ensure_scratch()
            else:
                self._unbind()
            return self.L.query("tdx_conv3_fwd_kernel", C1, C2, Co, B, *grid, code, impl)


def _name(B, grid, C1, C2, Co, **flags):
    return f"{B}x" + "x".join(map(str, grid)) + f"/{C1}+{C2}->{Co}" + "".join(f"/{k}{v}" for k, v in flags.items())


def _bits(rec, outs, crop):
    small = record([crop(o) for o in outs], True)
    rec.update({k: small[k] for k in ("bits", "itemsize") if k in small})
    return rec


def _conv_case(lib, B, grid, C1, C2, Co, dt, code, pack, impl, family, crop=None):
    """y, y of the fused-statistics forward, dx1 | dx2 without and with addends."""
    L, d = lib.L, torch.device("cuda:0")
    X, Y, Z = grid
    Ci = C1 + C2
    x1 = rnd(B, X, Y, Z, C1, seed=1).to(d).to(dt)
    x2 = rnd(B, X, Y, Z, C2, seed=2).to(d).to(dt) if C2 else None
    w = (rnd(Co, Ci, 3, 3, 3, seed=3) * (2.0 / (27 * Ci)) ** 0.5).to(d)
    bias, gy = rnd(Co, seed=4).to(d), rnd(B, X, Y, Z, Co, seed=5).to(d).to(dt)
    a1 = rnd(B, X, Y, Z, C1, seed=6).to(d).to(dt)
    a2 = rnd(B, X, Y, Z, C2, seed=7).to(d).to(dt) if C2 else None
    wf, wb = torch.empty(27 * Ci * Co, dtype=dt, device=d), torch.empty(27 * Ci * Co, dtype=dt, device=d)
    st = L.stream()
    L.call("tdx_conv3_pack_weight", L.ptr(w), L.ptr(wf), L.ptr(wb), Ci, Co, pack, st)
    assert lib.family(C1, C2, Co, B, grid, code, impl) == family, (B, grid, C1, C2, Co)
    # the data gradient is the zero-padded conv Co -> Ci of the same route (conv3_bwd_data_impl)
    assert lib.family(Co, 0, Ci, B, grid, code, impl) == (family if Ci % 32 == 0 else L.KERNEL_DIRECT), (B, grid, Co, Ci)
    y, ygn = (torch.empty(B, X, Y, Z, Co, device=d, dtype=dt) for _ in range(2))
    lib.call("tdx_conv3_fwd", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), L.ptr(bias), L.ptr(y), B, X, Y, Z, Co, code, impl, st)
    stats = torch.empty(B, 8, 2, device=d)
    gws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, Co), dtype=torch.uint8, device=d)
    lib.call("tdx_conv3_fwd_gn", L.ptr(x1), C1, L.ptr(x2), C2, L.ptr(wf), L.ptr(bias), L.ptr(ygn), L.ptr(stats), 8, 1e-5,
             L.ptr(gws), B, X, Y, Z, Co, code, impl, st)
    dws = torch.empty(L.query("tdx_conv3_bwd_data_workspace_bytes", B, X, Y, Z, Ci, code, impl), dtype=torch.uint8, device=d)
    dx1, dxa1 = torch.empty_like(x1), torch.empty_like(x1)
    dx2, dxa2 = (torch.empty_like(x2), torch.empty_like(x2)) if C2 else (None, None)
    with _env(TDX_SHELL_DETERMINISTIC="1"):
        lib.call("tdx_conv3_bwd_data", L.ptr(gy), L.ptr(wb), L.ptr(dx1), C1, L.ptr(dx2), C2, 0, B, X, Y, Z, Co, code, impl,
                 L.ptr(dws), st)
        lib.call("tdx_conv3_bwd_data_add", L.ptr(gy), L.ptr(wb), L.ptr(dxa1), C1, L.ptr(dxa2), C2, L.ptr(a1), L.ptr(a2), B, X, Y, Z,
                 Co, code, impl, L.ptr(dws), st)
    torch.cuda.synchronize()
    outs = [o for o in (y, ygn, dx1, dx2, dxa1, dxa2) if o is not None]
    rec = record(outs)
    return _bits(rec, outs, crop) if crop else rec


def _sample0(o):
    return o[:1, :1, :1, :4]  # the first 4 voxels


def _far_corner(o):
    return o[:1, -2:, -2:, -2:]


def _brick16(L, dn):
    lib, dt, code = _Lib(L, arena=False), H16[dn], L.dtype_code(H16[dn])
    res = {}
    with _env(TDX_CONV3_RING="0"):
        for B, grid in list(SMALL) + [THIN16]:
            for C1, C2, Co in CHANNELS:
                crop = _sample0 if grid == (4, 8, 8) and (C1, C2, Co) == NARROW_DX else None
                res[_name(B, grid, C1, C2, Co)] = _conv_case(lib, B, grid, C1, C2, Co, dt, code, code, L.CONV_AUTO, L.KERNEL_BRICK, crop)
    return res


def _partial(L, dn):
    """tdx_conv3_fwd_partial: the first C1 channels of rows of ld1 = C1 + 8, accumulators started from `init`."""
    lib, dt, code, d = _Lib(L, arena=False), H16[dn], L.dtype_code(H16[dn]), torch.device("cuda:0")
    B, (X, Y, Z) = PARTIAL
    res = {}
    st = L.stream()
    for C1, _, Co in FWD:
        ld1 = C1 + 8
        x = rnd(B, X, Y, Z, ld1, seed=1).to(d).to(dt)
        w = (rnd(Co, C1, 3, 3, 3, seed=3) * (2.0 / (27 * C1)) ** 0.5).to(d)
        bias = rnd(Co, seed=4).to(d)
        wf = torch.empty(27 * C1 * Co, dtype=dt, device=d)
        L.call("tdx_conv3_pack_weight", L.ptr(w), L.ptr(wf), None, C1, Co, code, st)
        for shared in (True, False):
            init = rnd(1 if shared else B, X, Y, Z, Co, seed=8).to(d).to(dt)
            y, ygn = (torch.empty(B, X, Y, Z, Co, device=d, dtype=dt) for _ in range(2))
            lib.call("tdx_conv3_fwd_partial", L.ptr(x), C1, ld1, L.ptr(wf), L.ptr(bias), L.ptr(init), int(shared), L.ptr(y), None, 0,
                     0.0, None, B, X, Y, Z, Co, code, L.CONV_AUTO, st)
            stats = torch.empty(B, 8, 2, device=d)
            gws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, Co), dtype=torch.uint8, device=d)
            lib.call("tdx_conv3_fwd_partial", L.ptr(x), C1, ld1, L.ptr(wf), L.ptr(bias), L.ptr(init), int(shared), L.ptr(ygn),
                     L.ptr(stats), 8, 1e-5, L.ptr(gws), B, X, Y, Z, Co, code, L.CONV_AUTO, st)
            torch.cuda.synchronize()
            rec = record([y, ygn])
            if (C1, Co) == NARROW[::2] and shared:
                rec = _bits(rec, [y, ygn], _sample0)
            res[_name(B, (X, Y, Z), C1, 0, Co, ld=ld1, shared=int(shared))] = rec
    return res


def _ring_slabs(L, dn):
    lib, dt, code = _Lib(L, arena=True), H16[dn], L.dtype_code(H16[dn])
    res = {}
    for i, (B, C1, C2, Co, grid, depth) in enumerate(RING):
        with _env(TDX_CONV3_RING="2", TDX_RING_Z4="2" if depth == 4 else "0"):
            assert L.query("tdx_conv3_ring_brick_depth", C1, C2, Co, B, *grid) == depth
            res[_name(B, grid, C1, C2, Co, depth=depth)] = _conv_case(lib, B, grid, C1, C2, Co, dt, code, code, L.CONV_AUTO,
                                                                     L.KERNEL_RING, _far_corner if i == 0 else None)
    return res


def _f32(L, mode, shapes, channels):
    lib = _Lib(L, arena=False)
    pack, impl = (L.F32_SPLIT, L.CONV_SPLIT) if mode == "split" else (L.F32, L.CONV_AUTO)
    res = {}
    for B, grid in shapes:
        for C1, C2, Co in channels:
            crop = _sample0 if grid == (4, 8, 8) and (C1, C2, Co) == NARROW_DX else None
            res[_name(B, grid, C1, C2, Co)] = _conv_case(lib, B, grid, C1, C2, Co, torch.float32, L.F32, pack, impl, L.KERNEL_BRICK, crop)
    return res


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd._lib` is bound to."""
    from turbdiff_amd import _lib as L

    kind, _, mode = group.partition("/")
    if kind == "brick16":
        return _brick16(L, mode)
    if kind == "partial":
        return _partial(L, mode)
    if kind == "ring_slabs":
        return _ring_slabs(L, mode)
    if kind == "f32":
        return _f32(L, mode, list(SMALL), CHANNELS)
    if kind == "f32_thin":
        return _f32(L, mode, [THIN32], [NARROW, NARROW_DX, (32, 32, 32)])
    return _f32(L, "split", [BIG], [NARROW, NARROW_DX])
