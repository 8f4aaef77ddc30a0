"""A plain float64 reference of the weight gradient of the replicate-padded 3x3x3 convolution (tdx_conv3_bwd_weight: csrc/
tdx_conv3_direct.hip and the six tdx_conv3_wgrad_*.hip), the inputs for which every one of its kernels is EXACT, and the error
bounds where they are not.  It uses neither the kernels nor the oracle and runs on whatever device its inputs are on
(tests/test_conv3_wgrad_reference.py holds it against float64 F.conv3d over F.pad(mode="replicate") and autograd).

    dW[co, ci, a, b, c] = sum_{n, v} x[n, clamp(v + (a - 1, b - 1, c - 1))][ci] dy[n, v][co],     dbias[co] = sum_{n, v} dy[n, v][co]

with x = [x1 | x2] (n, X, Y, Z, Cin) and dy (n, X, Y, Z, Cout) channels-last, clamp per axis into [0, extent - 1]: `wgrad`,
27 clamped gathers and matmuls.

Notation: u = 2^-24 (unit roundoff of float32), gamma_n = n u / (1 - n u), rows = n X Y Z (the terms of every sum above).

WHAT THE KERNELS COMPUTE.  All seven accumulate in float32 and store float32: no storage rounding.  The 16-bit kernels (brick16,
small, ring) multiply the stored bf16 / fp16 values in the matrix cores: products of two 8- or 11-bit significands are exact
in float32.  brick_f32 and direct multiply in float32 (one rounding per product).  The split-precision kernels (split,
split_ring) read float32 tensors and form, per value v (`split8`, csrc/tdx_mfma.h: __builtin_convertvector to __bf16, round to
nearest even),   vh = bf16(v),   vl = bf16(v - vh)   (v - vh is exact in float32: vh is within half a bf16 ulp of v), and
accumulate the three bf16 products xh dyh + xl dyh + xh dyl; xl dyl is dropped.  The split bias gradient is the float32 sum of
dy (split: from the staging registers) or of ones x (dyh + dyl) (split_ring).
Partial sums of K splits are merged by per-split slabs added in slab order (tiled unpack up to 8, summing unpack beyond) or by
float32 atomics in arrival order; all of it is ONE summation tree over the `rows` terms (zero-initialised accumulators: adding
to zero is exact; rows of a ragged brick beyond the grid contribute exact zeros).

EXACT INPUTS (`exact_inputs`).
  * "ints": x and dy are integers in [-4, 4] -- the same numbers in f32, bf16 and fp16, and their own bf16 hi part (lo = 0).
    Every product is an integer with |x dy| <= 16 and every partial sum in any order is an integer of magnitude at most
    sum |x| |dy| < 2^24: exact in float32's 24 bits.  Every route and every merge, atomics in arrival order included, must
    produce THE integer: torch.equal on dW and on dbias against the reference cast to float32.
  * "wide-x" / "wide-dy" (float32 tensors only): one operand is m 2^-6 with odd |m| in (256, 1023] -- 10 significant bits, so
    its bf16 hi part drops bits and its lo part is NOT zero, while hi + lo is the value exactly (the residual is at most 2
    units of 2^-6 in magnitude, whether hi was rounded or truncated); the other operand is an integer in [-2, 2] (lo = 0).
    The dropped lo x lo product is then zero, the three kept products are multiples of 2^-6, and every partial sum is bounded
    by sum (|hi| + |lo|) |other| < 2^24 units of 2^-6: the split-precision kernels, like brick_f32 and direct, must again
    give the reference bit for bit.  A lost or mis-paired lo term changes it (`drop_lo`).
  `assert_exact` proves these preconditions for the tensors it is given, from the reference side alone.

INEXACT INPUTS (`gaussian_inputs`; first order, times SLACK = 1 + 2^-10 for the second-order terms, like conv1_reference).
  * 16-bit and fp32 routes (`wgrad_bound`): a float32 sum of `rows` terms in any order errs by at most
    gamma_rows sum |x dy| (a leaf passes through its product's rounding -- none on the 16-bit routes -- and at most rows - 1
    additions); dbias likewise with gamma_rows sum |dy|.  This is conv1_reference.wgrad_bound, and like it loose: it grows
    with rows where the error grows with its root.  The exact rows are the sharp check, these show that unrestricted
    operands change nothing.
  * split precision on Gaussian float32 inputs (`split_bound`): write x = xh + xl + ex, dy = dyh + dyl + ey.  Rounding to
    nearest gives |xl + ex| = |x - xh| <= 2^-9 |x|, |ex| <= 2^-9 |x - xh| <= 2^-18 |x|, |xh| <= (1 + 2^-9) |x|, and the same
    for dy.  Then   x dy - (xh dyh + xl dyh + xh dyl) = xh ey + ex dyh + (xl + ex)(dyl + ey),   at most
        (2 (1 + 2^-9) 2^-18 + 2^-18) |x dy|  <  (3 + 2^-7) 2^-18 |x dy|                     (the residuals of the 8-bit lo
    parts and the dropped lo x lo term) per product.  The 3 rows products are exact in float32 and each passes at most
    3 rows - 1 additions; their magnitudes sum to at most (1 + 2^-9)^2 + 2 (1 + 2^-9) 2^-9 < 1 + 2^-7 times |x dy|:
        dW:     ((3 + 2^-7) 2^-18  +  gamma_(3 rows) (1 + 2^-7)) sum |x dy|
        dbias:  (2^-18 + gamma_(2 rows) (1 + 2^-9)) sum |dy|          (split_ring: |ey| <= 2^-18 |dy| per term, 2 rows terms;
                                                                       split's float32 sum of dy is within gamma_rows sum |dy|)
No element is left out of any comparison and no figure here comes from a run of the kernels.
"""

import itertools

import torch

import gn_reference as G

U, SLACK = G.U, G.SLACK
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FAMILIES = ("ints", "wide-x", "wide-dy")
WIDE_UNIT = 2.0**-6
TAPS = tuple(itertools.product(range(3), repeat=3))


# ----------------------------------------------------------------------------------------------------------- the operation


def _cat(x1, x2):
    return x1.double() if x2 is None else torch.cat((x1.double(), x2.double()), dim=-1)


def _clamped(n, e, device):
    return (torch.arange(n, device=device) + e).clamp_(0, n - 1)


def gather(x, tap, zero_pad=False):
    """x (B, X, Y, Z, C) -> (rows, C): row (n, v) holds x[n, clamp(v + tap - 1)]; zero_pad: zero outside the grid instead"""
    B, X, Y, Z, C = x.shape
    a, b, c = (t - 1 for t in tap)
    g = x[:, _clamped(X, a, x.device)][:, :, _clamped(Y, b, x.device)][:, :, :, _clamped(Z, c, x.device)]
    if zero_pad:
        for dim, n, e in ((1, X, a), (2, Y, b), (3, Z, c)):
            i = torch.arange(n, device=x.device) + e
            shape = [1] * 5
            shape[dim] = n
            g = g * ((i >= 0) & (i < n)).to(g.dtype).reshape(shape)
    return g.reshape(-1, C)


def wgrad(x1, x2, dy, zero_pad=False, keep=None):
    """dW (Cout, Cin, 3, 3, 3), dbias (Cout), float64.  keep: optional (rows,) mask of the voxels that are summed (the
    planted defects drop some); zero_pad: the planted defect of that name."""
    x, g = _cat(x1, x2), dy.double().reshape(-1, dy.shape[-1])
    if keep is not None:
        g = g * keep.to(g.dtype).reshape(-1, 1)
    dW = torch.empty(g.shape[1], x.shape[-1], 3, 3, 3, dtype=torch.float64, device=x.device)
    for tap in TAPS:
        dW[(slice(None), slice(None)) + tap] = g.t() @ gather(x, tap, zero_pad)
    return dW, g.sum(0)


def magnitude(x1, x2, dy):
    """(sum |x| |dy| per element of dW, sum |dy| per element of dbias): what bounds every partial sum in every order"""
    return wgrad(x1.abs(), None if x2 is None else x2.abs(), dy.abs())


# ------------------------------------------------------------------------------------------------------------------ inputs


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _wide(shape, g):
    m = 2 * torch.randint(128, 512, shape, generator=g) + 1  # odd, 257 .. 1023
    sign = 2 * torch.randint(0, 2, shape, generator=g) - 1
    return (sign * m).float() * WIDE_UNIT


def exact_inputs(B, grid, C1, C2, Cout, family="ints", seed=0):
    """CPU float32 tensors x1 (B, X, Y, Z, C1), x2 (.., C2) or None, dy (.., Cout) of the given family (module docstring)"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(7000 + 100 * FAMILIES.index(family) + seed)
    small = (lambda s: _ints(s, -4, 4, g)) if family == "ints" else (lambda s: _ints(s, -2, 2, g))
    fx = (lambda s: _wide(s, g)) if family == "wide-x" else small
    fy = (lambda s: _wide(s, g)) if family == "wide-dy" else small
    lead = (B, *grid)
    return dict(x1=fx((*lead, C1)), x2=fx((*lead, C2)) if C2 else None, dy=fy((*lead, Cout)))


def gaussian_inputs(B, grid, C1, C2, Cout, dt, seed=0):
    """The same keys, standard normal, rounded to the storage format dt (float32 values)"""
    g = torch.Generator().manual_seed(8000 + seed)
    q = lambda *s: torch.randn(*s, generator=g).to(dt).float()
    lead = (B, *grid)
    return dict(x1=q(*lead, C1), x2=q(*lead, C2) if C2 else None, dy=q(*lead, Cout))


def bf16_hi(t, truncate=False):
    """The bf16 hi part of float32 values as float32: rounded to nearest even (what the kernels do) or truncated"""
    if truncate:
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return t.to(torch.bfloat16).float()


def drop_lo(t):
    """Planted defect: the operand without its lo part"""
    return None if t is None else bf16_hi(t)


def _units(name, t, unit, limit=2.0**24):
    q = t.double() / unit
    assert torch.equal(q, q.round()), f"{name} is not a multiple of {unit}"
    assert q.abs().max().item() < limit, f"{name} reaches {q.abs().max().item()} units of {unit}: not below 2^24"


def assert_exact(p, family, dtypes):
    """The preconditions of an exact row, from the reference alone: units (1, or 2^-6 for the wide families), the values
    survive every storage format the row lists, and the sum of absolute terms -- of the hi and lo parts where they differ
    from the value -- stays below 2^24 units for every element of dW and dbias."""
    unit = 1.0 if family == "ints" else WIDE_UNIT
    if family != "ints":
        assert set(dtypes) == {"f32"}, "the wide families are float32 tensors"
    for k in ("x1", "x2", "dy"):
        if p[k] is None:
            continue
        _units(k, p[k], unit)
        for name in dtypes:
            assert torch.equal(p[k].to(DTYPES[name]).float(), p[k]), f"{k} does not survive {name}"
    mags = []
    for truncate in (False, True):  # hi + lo is the value with a rounded and with a truncated hi; lo fits bf16
        parts = {}
        for k in ("x1", "x2", "dy"):
            if p[k] is None:
                parts[k] = None
                continue
            hi = bf16_hi(p[k], truncate)
            lo = p[k] - hi
            assert torch.equal(hi.double() + lo.double(), p[k].double()) and torch.equal(bf16_hi(lo), lo), f"{k}: hi + lo is not exact"
            parts[k] = hi.abs() + lo.abs()
        mags.append(parts)
    wide = {"ints": None, "wide-x": "dy", "wide-dy": "x1"}[family]
    if wide is not None:  # the other operand has no lo part: the dropped lo x lo product is zero
        others = ("dy",) if wide == "dy" else ("x1", "x2")
        assert all(p[k] is None or torch.equal(bf16_hi(p[k]), p[k]) for k in others), "lo x lo must be zero"
        narrow = ("x1", "x2") if wide == "dy" else ("dy",)
        assert any(p[k] is not None and not torch.equal(bf16_hi(p[k]), p[k]) for k in narrow), "the wide operand needs a lo part"
    same = all(mags[0][k] is None or torch.equal(mags[0][k], mags[1][k]) for k in mags[0])  # "ints": the value is its own hi
    for parts in mags[:1] if same else mags:
        mw, mb = magnitude(parts["x1"], parts["x2"], parts["dy"])
        _units("sum (|xh| + |xl|)(|dyh| + |dyl|)", mw, unit)
        _units("sum |dyh| + |dyl|", mb, unit)


# ------------------------------------------------------------------------------------------------------------------ bounds


def gamma_n(n):
    return n * U / (1.0 - n * U)


def wgrad_bound(x1, x2, dy):
    """(bound of dW, bound of dbias) for the 16-bit, fp32-IEEE and vector-ALU routes"""
    rows = dy[..., 0].numel()
    mw, mb = magnitude(x1, x2, dy)
    g = SLACK * gamma_n(rows)
    return g * mw, g * mb


def split_bound(x1, x2, dy):
    """(bound of dW, bound of dbias) for the split-precision routes on unrestricted float32 inputs"""
    rows = dy[..., 0].numel()
    mw, mb = magnitude(x1, x2, dy)
    w = (3.0 + 2.0**-7) * 2.0**-18 + gamma_n(3 * rows) * (1.0 + 2.0**-7)
    b = 2.0**-18 + gamma_n(2 * rows) * (1.0 + 2.0**-9)
    return SLACK * w * mw, SLACK * b * mb
