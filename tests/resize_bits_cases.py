"""The bits of the trilinear resize (csrc/tdx_resize.hip): the cases shared by tests/test_resize_bits.py and
tests/golden/make_golden_bits.py.

`run(group)` returns one record per case and dtype (tests/pinned_bits.py).  Every case is a row of resize_cases.CASES -- the
smallest shape that reaches its route -- with seeded Gaussian inputs, and pins three outputs: y of tdx_resize_fwd, dx of
tdx_resize_bwd without `add`, and dx with `add`.  tests/test_resize_reference.py holds the inexact rows to a derived bound
only; here a reorder of the kernels' floating-point operations changes a digest.  Only digests are stored, and for one case
per group the raw bits of the first HEAD elements of every output, so that a mismatch there reads in ulps.

    pairs    resize_up_pairs_kernel: the 4 x 8 x 8 and 2 x 8 x 8 tiles with partial tiles, odd output extents, in == 1
    gather   resize_fwd_kernel: C / 8 = 3 (lane 255 idle), 512 channels (two trips over the 8-voxel tile), the two-trip rows
             at C = 64 and C = 24, out == 1
    adjoint  resize_bwd_kernel with K = 2, 4, 6 and 12 (ratio 11/64: candidate 11 in use), resize_bwd_generic_kernel
"""

import torch

import resize_cases as cases
import resize_reference as R
from pinned_bits import record as _digest, tensor_bytes

GROUPS = ["pairs", "gather", "adjoint"]
FIXTURE = "resize_bits.json"
HEAD = 512  # elements of each output whose raw bits one case of a group stores


def _row(B, C, src, dst):
    return next(c for c in cases.CASES if (c.B, c.C, c.src, c.dst) == (B, C, src, dst))


ROWS = {
    "pairs": [_row(1, 8, (9, 9, 9), (17, 17, 17)), _row(1, 16, (5, 5, 3), (9, 9, 9)), _row(2, 16, (6, 3, 4), (13, 7, 9)),
              _row(1, 8, (1, 1, 1), (3, 4, 5))],
    "gather": [_row(1, 24, (9, 5, 5), (17, 9, 9)), _row(2, 512, (6, 4, 3), (3, 3, 3)), _row(1, 512, (2, 3, 9), (3, 2, 5)),
               _row(2, 64, (32, 32, 32), (32, 32, 33)), _row(2, 24, (32, 32, 64), (32, 32, 65)), _row(1, 8, (4, 5, 6), (1, 1, 1))],
    "adjoint": [_row(1, 8, (9, 9, 9), (5, 5, 5)), _row(1, 8, (12, 3, 3), (24, 6, 6)), _row(1, 8, (4, 4, 4), (9, 9, 9)),
                _row(1, 8, (12, 2, 12), (65, 3, 65)), _row(1, 8, (3, 3, 3), (17, 17, 17))],
}
# the case of each group that stores raw bits; the first holds every element of its outputs (480, 8 and 8)
BITS = {"pairs": "1x8-1x1x1-3x4x5/f32", "gather": "1x8-4x5x6-1x1x1/bf16", "adjoint": "1x8-9x9x9-5x5x5/f16"}


def names(group):
    return [f"{cases.case_id(c)}/{d}" for c in ROWS[group] for d in c.dtypes]


def record(outs, smallest=False):
    rec = _digest(outs)
    if smallest:
        rec["bits"] = [tensor_bytes(o.flatten()[:HEAD]).hex() for o in outs]
        rec["itemsize"] = [o.element_size() for o in outs]
    return rec


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd._lib` is bound to."""
    from turbdiff_amd import ops

    dev = torch.device("cuda:0")
    res = {}
    for seed, c in enumerate(ROWS[group]):
        assert cases.routed(c)[1] == cases.expected(c), cases.case_id(c)
        g = torch.Generator().manual_seed(100 + seed)
        x = torch.randn(c.B, *c.src, c.C, generator=g)
        dy = torch.randn(c.B, *c.dst, c.C, generator=g)
        add = torch.randn(c.B, *c.src, c.C, generator=g)
        for dname in c.dtypes:
            dt = R.DTYPES[dname]
            xd, dyd, addd = (t.to(dev).to(dt) for t in (x, dy, add))
            y, geom = ops._resize_fwd(xd, c.dst)
            dx = ops._resize_bwd(dyd, None, geom)
            dxa = ops._resize_bwd(dyd, addd, geom)
            key = f"{cases.case_id(c)}/{dname}"
            res[key] = record([y, dx, dxa], key == BITS[group])
    return res
