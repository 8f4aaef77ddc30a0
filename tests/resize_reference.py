"""A plain float64 reference of the trilinear resize (align_corners=True) on (B, X, Y, Z, C) tensors and of its adjoint, the
inputs for which the kernels of csrc/tdx_resize.hip are EXACT, and the error bounds where they are not.  It uses neither the
kernels, nor the oracle, nor F.interpolate; it runs on whatever device its inputs are on (tests/test_resize_reference.py holds
it against float64 F.interpolate and its autograd).

THE OPERATION.  Per axis a dense out x in matrix W_a: output o sits at src = o (in - 1) / (out - 1) (0 when out == 1), computed
as a fractions.Fraction and cast once; i0 = floor(src) clamped to in - 1, i1 = min(i0 + 1, in - 1), f = src - i0;
W_a[o, i0] += 1 - f, W_a[o, i1] += f.  Forward: y = (Wx (x) Wy (x) Wz) x, one einsum per axis.  Adjoint: the transposes applied
to dy, plus `add`.

Notation: u = 2^-24, the unit roundoff of float32 (one rounding: relative error <= u).

DYADIC CASES (`dyadic_inputs`, `assert_exact`).  When (in - 1) / (out - 1) is k / 2^m on every axis, with small k, the float32
scale, every source index scale * o and every weight are exact: `assert_exact` checks that the float32 tables of
resize_cases.axis_weights ARE W_a.  Every weight is then a multiple of unit_a = 2^-m_a and every product of three a multiple of
unit = unit_x unit_y unit_z, at most 1: it fits float32 when 1 / unit <= 2^24.  x, dy and add are integers, so every term
w v and every partial sum, in any order and any grouping (the paired kernel sums z, then y, then x), is a multiple of unit, and
it is exact when its magnitude in that unit stays below 2^24.  A partial sum never exceeds sum |w| |v|:
  * forward: the rows of W_a sum to 1, so sum |w| |x| <= max |x|; `assert_exact` wants max |x| / unit < 2^24;
  * adjoint: `assert_exact` evaluates (|Wx|^T (x) |Wy|^T (x) |Wz|^T) |dy| + |add| -- which also bounds acc + add -- and wants
    its largest element / unit < 2^24.  `dyadic_inputs` picks the range of dy from the same quantities: the product of the
    largest column sums of the three W_a bounds sum |w| for any input voxel.
Integers up to 8, and the multiples of 1024 up to 4096 of the large-add variant, are exact in bf16 and fp16.  Hence the
forward, the adjoint and the adjoint with add equal the reference rounded ONCE, float32 -> T (Vec8<T>::store: round to nearest
even, which is what Tensor.to(T) does), bit for bit; for T = float32 they equal the reference.

INEXACT CASES (`first_order`, `bound`).  Line numbers are those of csrc/tdx_resize.hip.
  * Source index.  scale = fl((in - 1) / (out - 1)) (line 18) carries one rounding, src~ = fl(scale * o) (line 23) another:
    |src~ - src| <= delta_a(o) = 2 u src_a(o) (1 + u).  src~ - (float) i0 (line 25) is exact (both within a factor of two, or
    i0 = 0) and lies in [0, 1): the clamp does nothing.
  * Weights.  The float32 tap weights f~ = src~ - i0 and 1 - f~ taken in exact arithmetic are therefore within delta_a(o) of
    f and 1 - f.  Where src lies within delta_a(o) of an integer n the two arithmetics may pick different tap pairs,
    (n - 1, n) against (n, n + 1); the interpolant is continuous there (the tap that only one of them has carries a weight
    below delta_a(o), the shared one differs by |src~ - src|), so an error of delta_a(o) on the union of both pairs covers it.
    `axis_error` builds E_a, shaped like W_a, with delta_a(o) on those taps: |w~_a[o, i] - W_a[o, i]| <= E_a[o, i].
    The rounding of fl(1 - f~) (lines 78, 130, 242: inexact only where src~ < 1) is relative to the weight and is counted in R.
  * First order.  With every term w~ v passing through at most R roundings of relative size u,
        |got - ref| <= u R (|Wx| (x) |Wy| (x) |Wz|) |v| + sum_a (the same product with E_a in place of |W_a|) |v|
    and the transposes for the adjoint, plus u |add| for the one rounding of acc + add (line 327 / 381; that rounding's share
    of the sum is one of the R).
  * R, the roundings of a term on the longest path.  A product and an add are counted separately; where the compiler contracts
    them into one fma the count is an over-estimate.
      gather, resize_fwd_kernel:  3 (1 - w per axis, line 78) + 2 (wx * wy * wz, line 89) + 1 (w * v, line 92)
                                  + 8 (the adds into acc, 8 taps, line 92)                                         = 14
      paired, resize_up_pairs_kernel:  3 x 2 (per axis 1 - w1, line 130, and its sum with w1 when both taps fall on one
                                  window entry, line 131) + 3 (z: a product and two adds, line 198) + 3 (y, line 207)
                                  + 1 (tx.w * r, line 208) + 3 (the adds into acc over the window's x planes, line 208)  = 16
      tiled adjoint, resize_bwd_kernel<T, K>:  3 x 2 (axis_weight, lines 242-243) + 2 (wx * wy, line 307; wxy * wz, line 315)
                                  + 1 (w * v, line 318) + cx cy K (the sequential adds into acc over every candidate, the
                                  zero-weight padding included, lines 304-318; cx, cy <= the largest spans along x and y)
                                  + 1 (acc + add, line 327)                                                = 10 + cx cy K
      generic adjoint, resize_bwd_generic_kernel:  3 x 2 + 2 (lines 363, 367) + 1 (line 372) + sx sy sz (adds into acc, one
                                  per candidate with a non-zero weight, at most the product of the spans) + 1 (line 381)
                                                                                                           = 10 + sx sy sz
  * Storage.  For bf16 and fp16 the store rounds acc to T: + ulp_T(ref) (a float32 value in the binade of ref or the next one
    rounds to T within ulp_T(ref); acc is, whenever the bound is below |ref|).
  * Second order.  The whole bound is multiplied by 1 + 2^-10.  What first order leaves out is (1 + u)^R - 1 - R u (R <= 2^14:
    below 2^-10 R u) and the products of two or three weight errors, or of a weight error with the roundings.  `first_order`
    does not argue about those: it evaluates the complete expression
        (1 + u)^R ((|Wx| + Ex) (x) (|Wy| + Ey) (x) (|Wz| + Ez)) |v|  -  (|Wx| (x) |Wy| (x) |Wz|) |v|
    from the reference, for every element of every case, and takes the larger of the two.  The complete expression wins only
    where the first-order terms vanish: an input voxel that no output reads along TWO axes, next to a source position that is
    an integer on both (24 -> 12: src(11) = 23, and float32 may read 22 with a weight below delta; 6 -> 3 likewise).  There a
    correct kernel may return delta_x delta_y |dy| ~ 10^-12 instead of 0, which no first-order bound allows; `first_order`
    asserts that this is the only place (first order below u^2 of the complete sum of |w| |v| wherever it is exceeded).
No figure here comes from a run of the kernels.
"""

from fractions import Fraction

import numpy as np
import torch

import resize_cases as cases
from gn_reference import store_rounding

U = 2.0**-24
SLACK = 1.0 + 2.0**-10
R_GATHER, R_PAIRS = 14, 16
R_MAX = 2**14
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# ------------------------------------------------------------------------------------------------------------ the operation


def _positions(n_in, n_out):
    return [Fraction(o * (n_in - 1), n_out - 1) if n_out > 1 else Fraction(0) for o in range(n_out)]


def axis_matrix(n_in, n_out):
    """W_a, out x in float64 (CPU)"""
    W = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o, src in enumerate(_positions(n_in, n_out)):
        i0 = min(src.numerator // src.denominator, n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        f = float(src - i0)
        W[o, i0] += 1.0 - f
        W[o, i1] += f
    return W


def axis_error(n_in, n_out):
    """E_a, out x in float64 (CPU): delta_a(o) on the taps of o in float64 and on the neighbour the float32 arithmetic may
    pick instead (module docstring)"""
    E = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o, src in enumerate(_positions(n_in, n_out)):
        delta = 2.0 * U * float(src) * (1.0 + U)
        if delta == 0.0:
            continue
        i0 = min(src.numerator // src.denominator, n_in - 1)
        f = float(src - i0)
        taps = {i0, min(i0 + 1, n_in - 1)}
        if f < delta:
            taps.add(max(i0 - 1, 0))
        if f + delta >= 1.0:
            taps.add(min(i0 + 2, n_in - 1))
        for i in taps:
            E[o, i] = delta
    return E


def matrices(src, dst, device="cpu"):
    return [axis_matrix(i, o).to(device) for i, o in zip(src, dst)]


def errors(src, dst, device="cpu"):
    return [axis_error(i, o).to(device) for i, o in zip(src, dst)]


def _apply(mats, v):
    """(Mx (x) My (x) Mz) v for v (B, X, Y, Z, C) float64: z first (the cheapest order when the grid grows)"""
    v = torch.einsum("rk,bijkc->bijrc", mats[2], v)
    v = torch.einsum("qj,bijrc->biqrc", mats[1], v)
    return torch.einsum("pi,biqrc->bpqrc", mats[0], v)


def _t(mats):
    return [m.t() for m in mats]


def forward(x, dst):
    return _apply(matrices(x.shape[1:4], dst, x.device), x.double())


def adjoint(dy, src, add=None):
    dx = _apply(_t(matrices(src, dy.shape[1:4], dy.device)), dy.double())
    return dx if add is None else dx + add.double()


def unread(src, dst):
    """(X, Y, Z) bool: input voxels that no output reads (a zero column of some W_a); their gradient is `add`, or 0"""
    cols = [axis_matrix(i, o).sum(0) == 0 for i, o in zip(src, dst)]
    return cols[0][:, None, None] | cols[1][None, :, None] | cols[2][None, None, :]


# ------------------------------------------------------------------------------------------------------------- exact cases


def _unit(W):
    """the largest power of two that divides every entry of W"""
    for m in range(25):
        if torch.equal(W * 2.0**m, torch.round(W * 2.0**m)):
            return 2.0**-m
    raise AssertionError("the weights are not dyadic")


def dyadic_inputs(src, dst, B, C, seed=0, add_scale=1):
    """CPU float32 x (B, *src, C), dy (B, *dst, C), add like x, all integers: x in [-8, 8], add in add_scale * [-4, 4], dy in
    [-m, m] with m <= 8 the largest for which sum |w| |dy| + |add| stays below 2^24 units for ANY input voxel (the product of
    the largest column sums of the W_a bounds sum |w|)."""
    mats = matrices(src, dst)
    unit = float(np.prod([_unit(W) for W in mats]))
    col = float(np.prod([W.sum(0).max().item() for W in mats]))
    add_max = 4 * add_scale
    m = min(8, int((2.0**24 * unit - unit - add_max) / col))
    assert m >= 1, "no integer range of dy keeps the adjoint exact"
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randint(-8, 9, (B, *src, C), generator=g).float(),
                dy=torch.randint(-m, m + 1, (B, *dst, C), generator=g).float(),
                add=(add_scale * torch.randint(-4, 5, (B, *src, C), generator=g)).float())


def assert_exact(src, dst, p):
    """The preconditions of the exact cases (module docstring), from the reference alone."""
    mats = matrices(src, dst)
    for a, W in enumerate(mats):
        Wf = torch.from_numpy(cases.axis_weights(cases.make_axis(src[a], dst[a]))).double()
        assert torch.equal(Wf, W), f"axis {a}: the float32 scale, source indices or weights are not exact"
        assert bool((W.sum(1) == 1.0).all()) and bool((W >= 0).all())
    unit = float(np.prod([_unit(W) for W in mats]))
    assert 1.0 / unit <= 2.0**24  # every product of three weights, a multiple of unit and at most 1, fits 24 bits
    for k in ("x", "dy", "add"):
        assert torch.equal(p[k], p[k].round()), f"{k} is not integer"
        for dt in DTYPES.values():
            assert torch.equal(p[k].to(dt).float(), p[k]), f"{k} is not exact in {dt}"
    assert p["x"].abs().max().item() / unit < 2.0**24
    worst = _apply(_t(mats), p["dy"].double().abs()) + p["add"].double().abs()
    assert worst.max().item() / unit < 2.0**24
    return unit


# ------------------------------------------------------------------------------------------------------------------ bounds


def adjoint_roundings(route):
    """R of the adjoint kernel a route takes (module docstring)"""
    sx, sy, sz = route.spans
    return 10 + (sx * sy * sz if route.bwd == cases.GENERIC else sx * sy * route.bwd)


def forward_roundings(route):
    return R_PAIRS if route.fwd == cases.PAIRS else R_GATHER


def first_order(mats, errs, v, R, add=None):
    """u R (|Wx| (x) |Wy| (x) |Wz|) |v| + sum_a (E_a in place of |W_a|) |v| [+ u |add|] per output element; the complete
    expression / (1 + 2^-10) where that is larger (module docstring, second order)."""
    assert R <= R_MAX
    av = v.double().abs()
    aw = [m.abs() for m in mats]
    p_abs = _apply(aw, av)
    first = U * R * p_abs
    for a in range(3):
        first = first + _apply([errs[b] if b == a else aw[b] for b in range(3)], av)
    p_full = _apply([w + e for w, e in zip(aw, errs)], av)
    full = (1.0 + U)**R * p_full - p_abs
    over = full > SLACK * first
    assert bool((first[over] <= U * U * p_full[over]).all()), "second-order terms above 2^-10 of a first-order bound that is not 0"
    first = torch.maximum(first, full / SLACK)
    return first if add is None else first + U * add.double().abs()


def forward_bound(x, dst, route, ref, dtype):
    d = x.device
    first = first_order(matrices(x.shape[1:4], dst, d), errors(x.shape[1:4], dst, d), x, forward_roundings(route))
    return SLACK * first + store_rounding(ref, dtype)


def adjoint_bound(dy, src, route, ref, dtype, add=None):
    d = dy.device
    first = first_order(_t(matrices(src, dy.shape[1:4], d)), _t(errors(src, dy.shape[1:4], d)), dy, adjoint_roundings(route), add)
    return SLACK * first + store_rounding(ref, dtype)
