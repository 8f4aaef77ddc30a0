"""The bits of the streaming GroupNorm kernels of csrc/tdx_groupnorm.hip and of the codec kernels whose arithmetic the two fused
tails repeat (csrc/tdx_codec.hip): the cases shared by tests/test_gn_bits.py and tests/golden/make_golden_bits.py.

`run(group)` calls one entry of the C ABI through `turbdiff_amd._lib` for every case of the group and returns one record per
case (tests/pinned_bits.py).  `stats` is an INPUT, drawn on the CPU: the f64-atomic statistics pass is not part of what is
pinned.  Inputs are seeded CPU draws; only digests are stored, and the raw bits at V = 5.

The shapes (B, C, G, V) are the smallest that reach each branch of the streaming loops; `lane_paths` restates the grid rule
(gn_blocks_per_sample) and tests/test_gn_bits.py::test_shapes_reach_their_branches holds every claim below against it.
"""

import torch

from pinned_bits import record
from step_inputs import rnd

THREADS, UNROLL, MAX_BLOCKS = 256, 4, 512  # GN_THREADS, GN_UNROLL, GN_MAX_BLOCKS
TRIP, TAIL, BOTH = (True, False), (False, True), (True, True)  # what a lane with work runs: (a full trip, the tail loop)

# (B, C, G, V): blocks per sample, voxel stride, spare threads per block, the paths its working lanes take
SHAPES = {
    (1, 8, 1, 5): (1, 256, 0, {TAIL}),             # one block, tail loop only; raw bits stored
    (2, 64, 8, 1000): (8, 256, 0, {TRIP, TAIL}),   # first voxel < 232: one full trip, the others the tail only
    (1, 24, 3, 1500): (5, 425, 1, {TRIP, TAIL}),   # L = 3, rows = 85: thread 255 is a spare and writes nothing
    (3, 512, 8, 150): (10, 40, 0, {TRIP, TAIL}),   # L = 64, a whole wave per voxel: decode's widest butterfly
    (1, 8, 2, 5000): (5, 1280, 0, {TRIP, TAIL}),   # L = 1
    (32, 256, 8, 2600): (64, 512, 0, {BOTH}),      # the 2048 / B cap binds: every lane runs a full trip AND THEN the tail
}
BIG = (32, 256, 8, 2600)  # bf16 only (21 M elements)
SMALL = [s for s in SHAPES if s != BIG]
ENCODED = [(2, 32, True, 8, 1000), (1, 16, False, 2, 5)]  # (B, D, with c_raw, G, V): C = 64 and C = 16
DECODE = [(2, 32, 8, 1000), (2, 64, 8, 1000), (3, 512, 8, 150)]  # (B, C, G, V); L must be a power of two
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GROUPS = ["gn_apply", "gn_bwd", "gn_apply_encoded", "gn_apply_decode", "encode_fwd", "decode_fwd", "gn_apply/big", "gn_bwd/big"]
FIXTURE = "gn_bits.json"


def blocks_per_sample(B, C, V):
    rows = THREADS // (C // 8)
    return max(1, min(-(-2048 // B), -(-V // (rows * UNROLL)), MAX_BLOCKS))


def stream_paths(stride, V):
    """{(ran a full trip, ran the tail loop)} over the lanes that have one of V voxels, walked with `stride`, UNROLL per trip."""
    paths = set()
    for v in range(min(stride, V)):  # a lane's first voxel
        trips = 0
        while v + (UNROLL - 1) * stride < V:
            v, trips = v + UNROLL * stride, trips + 1
        paths.add((trips > 0, v < V))
    return paths


def lane_paths(B, C, V):
    """(blocks, stride, spare threads, {(ran a full trip, ran the tail loop)} over the lanes that have a voxel)."""
    L = C // 8
    rows = THREADS // L
    blocks = blocks_per_sample(B, C, V)
    stride = blocks * rows
    return blocks, stride, THREADS - rows * L, stream_paths(stride, V)


def _name(*shape, dtype, **flags):
    return "x".join(map(str, shape)) + f"/{dtype}" + "".join(f"/{k}{int(v)}" for k, v in flags.items())


def _stats(B, G, d):
    return torch.stack((rnd(B, G, seed=8) * 0.1, rnd(B, G, seed=9).abs() + 0.5), dim=-1).contiguous().to(d)


def _gn_inputs(shape, dt, d):
    B, C, G, V = shape
    x, other = (rnd(B, V, C, seed=s).to(d).to(dt) for s in (1, 2))  # other: the residual (apply) / dy (backward)
    par = dict(stats=_stats(B, G, d), gamma=rnd(C, seed=10).to(d), beta=rnd(C, seed=11).to(d),
               scale=(0.5 * rnd(B, C, seed=4)).to(d), shift=(0.5 * rnd(B, C, seed=5)).to(d))
    return x, other, par


def _gn_apply(L, shapes, dtypes, d):
    res = {}
    for shape in shapes:
        B, C, G, V = shape
        for dn in dtypes:
            x, r, p = _gn_inputs(shape, DTYPES[dn], d)
            for act in (False, True):
                for has_res in (False, True):
                    for film in (False, True):
                        y = torch.empty_like(x)
                        L.call("tdx_gn_apply", L.ptr(x), L.ptr(p["stats"]), L.ptr(p["gamma"]), L.ptr(p["beta"]),
                               L.ptr(p["scale"] if film else None), L.ptr(p["shift"] if film else None),
                               L.ptr(r if has_res else None), L.ptr(y), B, V, C, G, int(act), L.dtype_code(x.dtype), L.stream())
                        res[_name(*shape, dtype=dn, act=act, res=has_res, film=film)] = record([y], V == 5)
    return res


def _gn_bwd(L, shapes, dtypes, d):
    res = {}
    for shape in shapes:
        B, C, G, V = shape
        ws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, C), dtype=torch.uint8, device=d)
        for dn in dtypes:
            x, dy, p = _gn_inputs(shape, DTYPES[dn], d)
            for act in (False, True):
                for film in (False, True):
                    dx = torch.empty_like(x)
                    dgamma, dbeta = torch.empty(C, device=d), torch.empty(C, device=d)
                    dscale, dshift = (torch.empty(B, C, device=d), torch.empty(B, C, device=d)) if film else (None, None)
                    L.call("tdx_gn_bwd", L.ptr(x), L.ptr(dy), L.ptr(p["stats"]), L.ptr(p["gamma"]), L.ptr(p["beta"]),
                           L.ptr(p["scale"] if film else None), L.ptr(p["shift"] if film else None), L.ptr(dx), L.ptr(dgamma),
                           L.ptr(dbeta), L.ptr(dscale), L.ptr(dshift), B, V, C, G, int(act), L.dtype_code(x.dtype), L.ptr(ws),
                           L.stream())
                    outs = [dx, dgamma, dbeta] + ([dscale, dshift] if film else [])
                    res[_name(*shape, dtype=dn, act=act, film=film)] = record(outs, V == 5)
    return res


def _encoder(B, D, with_c, V, d):
    x, wx, bx = rnd(B, 4, V, seed=1).to(d), rnd(D, 4, seed=3).to(d), rnd(D, seed=4).to(d)
    c, wc, bc = (rnd(4, V, seed=2).to(d), rnd(D, 4, seed=5).to(d), rnd(D, seed=6).to(d)) if with_c else (None, None, None)
    return x, wx, bx, c, wc, bc


def _encoded(L, fused, d):
    res = {}
    for B, D, with_c, G, V in ENCODED:
        C = 2 * D if with_c else D
        x, wx, bx, c, wc, bc = _encoder(B, D, with_c, V, d)
        Fc = 4 if with_c else 0
        for dn, dt in DTYPES.items():
            y = torch.empty(B, V, C, device=d, dtype=dt)
            if fused:
                h, stats, gamma, beta = rnd(B, V, C, seed=7).to(d).to(dt), _stats(B, G, d), rnd(C, seed=10).to(d), rnd(C, seed=11).to(d)
                L.call("tdx_gn_apply_encoded", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(x), 4, L.ptr(wx), L.ptr(bx), L.ptr(c), Fc, L.ptr(wc), L.ptr(bc), L.ptr(y),
                       B, V, D, G, L.dtype_code(dt), L.stream())
            else:
                L.call("tdx_encode_fwd", L.ptr(x), 4, L.ptr(wx), L.ptr(bx), L.ptr(c), Fc, L.ptr(wc), L.ptr(bc), L.ptr(y), B, V, D,
                       L.dtype_code(dt), L.stream())
            res[_name(B, D, G, V, dtype=dn, c=with_c)] = record([y], V == 5)
    return res


def _decode(L, fused, d):
    res = {}
    for B, C, G, V in DECODE:
        w, bias = rnd(4, C, seed=12).to(d), rnd(4, seed=13).to(d)
        stats, gamma, beta = _stats(B, G, d), rnd(C, seed=10).to(d), rnd(C, seed=11).to(d)
        for dn, dt in DTYPES.items():
            h, r = (rnd(B, V, C, seed=s).to(d).to(dt) for s in (1, 2))
            out = torch.empty(B, 4, V, device=d)
            if fused:
                L.call("tdx_gn_apply_decode", L.ptr(h), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(r), L.ptr(w), L.ptr(bias), L.ptr(out), B, V, C, G, 4, L.dtype_code(dt),
                       L.stream())
            else:
                L.call("tdx_decode_fwd", L.ptr(h), L.ptr(w), L.ptr(bias), L.ptr(out), B, V, C, 4, L.dtype_code(dt), L.stream())
            res[_name(B, C, G, V, dtype=dn)] = record([out])
    return res


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd._lib` is bound to."""
    from turbdiff_amd import _lib as L

    d = torch.device("cuda:0")
    entry, _, big = group.partition("/")
    if entry in ("gn_apply", "gn_bwd"):
        fn = _gn_apply if entry == "gn_apply" else _gn_bwd
        return fn(L, [BIG], ["bf16"], d) if big else fn(L, SMALL, list(DTYPES), d)
    if entry in ("gn_apply_encoded", "encode_fwd"):
        return _encoded(L, entry == "gn_apply_encoded", d)
    return _decode(L, entry == "gn_apply_decode", d)
