"""A plain float64 reference of GroupNorm (+ FiLM + SiLU + residual) on (B, V, C) tensors, the inputs for which the kernels of
csrc/tdx_groupnorm.hip are EXACT, and the error bounds where they are not.  It uses neither the kernels nor the oracle; it runs
on whatever device its inputs are on (tests/test_gn_reference.py holds it against float64 autograd of F.group_norm).

Notation: u = 2^-24, the unit roundoff of float32 (one rounding: relative error <= u; "1 ulp": <= 2 u).  With
film = 1 + scale, k = gamma film, xhat = (x - mean) rstd:

    n  = (xhat gamma + beta) film + shift            y  = [silu](n) + res
    dn = dy [silu'](n)     P = sum_v dn     Q = sum_v dn xhat     A = mean_g(k P)     Bq = mean_g(k Q)
    dx = rstd (k dn - A - xhat Bq)     dgamma = sum_b film Q     dbeta = sum_b film P     dshift = P     dscale = gamma Q + beta P

DYADIC INPUTS (`dyadic_inputs`).  x is an integer in [-8, 8], mean an integer in [-2, 3], rstd a power of two in [1/4, 2],
gamma a multiple of 1/2, beta / shift / scale / res multiples of 1/4, dy an integer in [-4, 4].  Every product the kernels form
with act = 0 then has at most 12 significant bits of float32's 24: a = rstd gamma film, c0, n = fma(x, a, c0), n + res, xhat,
dn xhat and the float32 partial sums of P and Q are exact, whatever their order (`assert_exact` checks exactly that, from the
reference: a value that survives the round trip through float32, sums below 2^24 in their unit).  Hence
  * tdx_gn_apply(act = 0) equals the reference rounded once to T, bit for bit;
  * P and Q are exact, the f64 products behind dgamma / dbeta / dscale / dshift are exact, and the four equal the reference cast
    to float32, bit for bit;
  * A and Bq are one f64 division and one cast: `bwd(round_group_means=True)` performs the same two operations;
  * dx = fma(k1, dn, -fma(xhat, k3, k2)) with k1 = rstd k, k2 = rstd A, k3 = rstd Bq exact: two float32 roundings, each at most
    u times a magnitude below |k1 dn| + |k2| + |xhat k3|, and the store to T:
        |dx - ref| <= 2 u (|k1 dn| + |k2| + |xhat k3|) + ulp_T(ref) [T != float32]                              (`dx_rounding`)
    (a float32 value within the same or the next binade of ref rounds to T within ulp_T(ref).)

act = 1 (`silu_bounds`, `bwd_bounds`).  n is still exact, and `dyadic_inputs(narrow=True)` keeps |n| <= 32.  sigmoid_f(n) is
v_rcp_f32(1 + v_exp_f32(c n)), c = float32(-log2 e).  The AMD ISA documents give both instructions as accurate to 1 ulp (the
guides on kernel writing give no other figure).  Then, to first order,
  * the argument: c differs from -log2 e by 0.224 u relative (the constant's own rounding), the product rounds once: the
    argument is off by at most 1.224 u relative, which moves exp(-n) by at most 1.224 |n| u relative; bounded as 1.25 |n| u;
  * v_exp_f32: 2 u.  These two reach the sum 1 + exp(-n) weighted by exp(-n) / (1 + exp(-n)) = 1 - s <= 1;
  * the add: u;  v_rcp_f32: 2 u.
        E_s = (1.25 |n| + 5) u      relative error of sigmoid_f(n)
  * silu: n s~ [+ res] is one multiply or one fma:  |y - ref| <= |n| s E_s + u (|n s| + |res|) + ulp_T(ref)
  * dsilu_f = s~ fma(n, fl(1 - s~), 1), with t = 1 + n (1 - s):  fl(1 - s~) is off by s E_s + u (1 - s), the fma by |n| times
    that plus u |t|, the last product adds |t| s E_s and rounds once:
        E_d = s (|n| (s E_s + u (1 - s)) + |t| (E_s + 2 u))      ABSOLUTE error of dsilu_f(n) (t cancels near n = -1.28)
  * dn = fl(dy dsilu_f):  D = |dy| E_d + u |dy silu'(n)| per element.
  * P and Q are float32 sums: a thread adds its n_t voxels in turn, then one thread adds the block's `rows` partials in turn, so
    a term passes through at most n_t + rows roundings; the sums over blocks and everything after are f64:
        |P~ - P| <= sum_v D + (n_t + rows) u sum_v (|dn| + D)        |Q~ - Q| likewise with every term times |xhat|
    (xhat is exact, the fma into Q rounds once per term like the add into P).  The sums come from the reference.
  * the parameter gradients are f64 combinations of P~, Q~ cast once: their bounds are the same combinations of the bounds of P
    and Q with absolute coefficients, plus u |ref| for the cast; A and Bq likewise, plus 2 u |A| (this cast and the reference's).
  * dx: |k1| D + rstd (E_A + |xhat| E_Bq) on top of `dx_rounding`.
Every bound is multiplied by 1 + 2^-10 for the second-order terms (products of two errors of at most 45 u; (1 + u)^m - 1 - m u
for chains of m <= 600 roundings): they are below 2^-10 of the first-order terms.  No figure here comes from a run of the kernels.

STATISTICS.  For integer x every float32 per-thread sum of x and x^2 is exact below 2^24, the f64 block sums and atomics are sums
of integers: the kernel's (sum, sum of squares) are exact, and mean = s / N, var = ss / N - mean^2, rstd = 1 / sqrt(var + eps)
are the same few f64 operations `stats` performs, so the two differ by the final double-to-float rounding only: 1 ulp of float32.
"""

import math
from collections import namedtuple

import torch

from gn_cases import THREADS, stream_paths

U = 2.0**-24
SLACK = 1.0 + 2.0**-10
N_MAX = 32.0  # |n| of the act = 1 cases
VOX_PER_BLOCK, DET_MAX_BLOCKS, ARENA_HEAD = 1024, 64, 256  # GN_VOX_PER_BLOCK; the caps of gn_stats_launch


def f32(v):
    """A Python float rounded to float32, as a C `float` argument arrives."""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------ the operation


def _per_channel(stats, C):
    """mean, rstd of each channel's group as (B, 1, C) float64"""
    B, G, _ = stats.shape
    s = stats.double().repeat_interleave(C // G, dim=1)
    return s[:, None, :, 0], s[:, None, :, 1]


def stats(x, G, eps32):
    """(B, G, 2) float64 mean and 1 / sqrt(var + eps32) of x (B, V, C) over each group's C / G channels and the V voxels."""
    B, V, C = x.shape
    xd = x.double().reshape(B, V, G, C // G)
    n = float(C // G * V)
    mean = xd.sum((1, 3)) / n
    var = ((xd * xd).sum((1, 3)) / n - mean * mean).clamp_min(0.0)
    return torch.stack((mean, 1.0 / torch.sqrt(var + eps32)), dim=-1)


def pre_activation(x, stats, gamma, beta, scale, shift):
    """n, xhat as float64 (B, V, C)"""
    mean, rstd = _per_channel(stats, x.shape[-1])
    xhat = (x.double() - mean) * rstd
    n = xhat * gamma.double() + beta.double()
    if scale is not None:
        n = n * (1.0 + scale.double()[:, None, :]) + shift.double()[:, None, :]
    return n, xhat


def apply(x, stats, gamma, beta, scale, shift, res, act):
    n, _ = pre_activation(x, stats, gamma, beta, scale, shift)
    y = n * torch.sigmoid(n) if act else n
    return y if res is None else y + res.double()


Bwd = namedtuple("Bwd", "dx dgamma dbeta dscale dshift terms")


def bwd(x, dy, stats, gamma, beta, scale, shift, act, round_group_means=True):
    """The five gradients in float64 and `terms`, what the bounds are made of.  round_group_means: A and Bq are cast to float32
    after their f64 division, as the kernel hands them from its group pass to its apply pass."""
    B, V, C = x.shape
    G = stats.shape[1]
    n, xhat = pre_activation(x, stats, gamma, beta, scale, shift)
    _, rstd = _per_channel(stats, C)
    film = torch.ones(B, C, dtype=torch.float64, device=x.device) if scale is None else 1.0 + scale.double()
    k = gamma.double() * film  # (B, C)
    s = torch.sigmoid(n)
    dsilu = s * (1.0 + n * (1.0 - s)) if act else torch.ones_like(n)
    dn = dy.double() * dsilu
    P, Q = dn.sum(1), (dn * xhat).sum(1)  # (B, C)
    N = float(C // G * V)
    group = lambda t: (t.reshape(B, G, C // G).sum(-1) / N)
    A, Bq = group(k * P), group(k * Q)  # (B, G)
    if round_group_means:
        A, Bq = A.float().double(), Bq.float().double()
    per_c = lambda t: t.repeat_interleave(C // G, dim=1)[:, None, :]
    k1dn, k2, xk3 = rstd * k[:, None, :] * dn, rstd * per_c(A), xhat * rstd * per_c(Bq)
    dx = k1dn - k2 - xk3
    dgamma, dbeta = (film * Q).sum(0), (film * P).sum(0)
    dscale, dshift = (gamma.double() * Q + beta.double() * P, P) if scale is not None else (None, None)
    terms = dict(n=n, xhat=xhat, rstd=rstd, k=k, film=film, dn=dn, dsilu=dsilu, P=P, Q=Q, A=A, Bq=Bq,
                 dx_terms=k1dn.abs() + k2.abs() + xk3.abs(), sum_abs_P=dn.abs().sum(1), sum_abs_Q=(dn * xhat).abs().sum(1))
    return Bwd(dx, dgamma, dbeta, dscale, dshift, terms)


# ------------------------------------------------------------------------------------------------------------------ inputs


def _pick(values, shape, g):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(len(values), shape, generator=g)]


def dyadic_inputs(shape, seed=0, narrow=False):
    """CPU float32 tensors x, res, dy (B, V, C), stats (B, G, 2), gamma, beta (C), scale, shift (B, C), every value exact in bf16
    and fp16.  narrow (the act = 1 cases): rstd in {1/4, 1/2} only, which keeps |n| <= (5.5 * 2 + 2) * 2 + 2 = 28 <= N_MAX."""
    B, C, G, V = shape
    g = torch.Generator().manual_seed(seed)
    quarters = lambda lo, hi: [q / 4 for q in range(int(4 * lo), int(4 * hi) + 1)]
    return dict(
        x=torch.randint(-8, 9, (B, V, C), generator=g).float(),
        res=_pick(quarters(-4, 4), (B, V, C), g),
        dy=torch.randint(-4, 5, (B, V, C), generator=g).float(),
        stats=torch.stack((torch.randint(-2, 4, (B, G), generator=g).float(),
                           _pick([0.25, 0.5] if narrow else [0.25, 0.5, 1.0, 2.0], (B, G), g)), dim=-1).contiguous(),
        gamma=_pick([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0], (C,), g),
        beta=_pick(quarters(-2, 2), (C,), g),
        scale=_pick([-0.5, -0.25, 0.0, 0.25, 0.5, 1.0], (B, C), g),
        shift=_pick(quarters(-2, 2), (B, C), g))


def integer_input(shape, seed=0, constant=None):
    """x (B, V, C) float32 for the statistics pass: integers in [-8, 8], or one integer everywhere."""
    B, C, G, V = shape
    if constant is not None:
        return torch.full((B, V, C), float(constant))
    return torch.randint(-8, 9, (B, V, C), generator=torch.Generator().manual_seed(seed)).float()


def _survives_f32(name, t):
    assert torch.equal(t.float().double(), t), f"{name} is not exact in float32: the inputs are not the exact ones"


def assert_exact(p, film, act):
    """The preconditions of the exact cases (module docstring), from the reference alone: the float32 intermediates survive a
    round trip through float32 and each channel's sum of |terms| of P and of Q -- an upper bound of every per-thread and per-block
    partial sum -- is below 2^24 in the terms' unit (dn: 1, dn xhat: 1/4).  act = 1: n is exact and |n| <= N_MAX."""
    sc, sh = (p["scale"], p["shift"]) if film else (None, None)
    n, xhat = pre_activation(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh)
    mean, rstd = _per_channel(p["stats"], p["x"].shape[-1])
    filmf = 1.0 + sc.double()[:, None, :] if film else 1.0
    a = rstd * p["gamma"].double() * filmf
    for name, t in (("a", a), ("c0", n - p["x"].double() * a), ("n", n), ("n + res", n + p["res"].double()), ("xhat", xhat)):
        _survives_f32(name, t)
    if act:
        assert n.abs().max().item() <= N_MAX
        return
    dn = p["dy"].double()
    for name, t, unit in (("P", dn, 1.0), ("Q", dn * xhat, 0.25)):
        _survives_f32(name + " terms", t)
        assert torch.equal(t / unit, torch.round(t / unit)) and (t.abs().sum(1) / unit).max().item() < 2.0**24, name


# ------------------------------------------------------------------------------------------------------ distances and bounds

_FORMAT = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}  # significand bits, least normal exponent


def ulp_distance(a, b):
    """Units of the last place between two float32 tensors, through their int32 views (+0 and -0 are 0 apart)."""
    def ordered(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    assert a.dtype == b.dtype == torch.float32
    return (ordered(a) - ordered(b)).abs()


def ulp_of(ref, dtype):
    """The spacing of `dtype` at |ref| (float64; its subnormal spacing below the least normal number)."""
    bits, emin = _FORMAT[dtype]
    e = torch.frexp(ref.abs())[1] - 1  # floor(log2 |ref|); frexp(0) gives exponent 0, clamped next
    e = torch.where(ref == 0, torch.full_like(e, emin), e.clamp_min(emin))
    return torch.ldexp(torch.ones_like(ref), e - (bits - 1))


def store_rounding(ref, dtype):
    return 0.0 if dtype == torch.float32 else ulp_of(ref, dtype)


def dx_rounding(terms, ref, dtype):
    """act = 0, and the part of act = 1 that is not inherited: the two fmas and the store of dx."""
    return 2.0 * U * terms["dx_terms"] + store_rounding(ref, dtype)


def silu_bounds(n):
    """E_s (relative, of sigmoid_f), E_d (absolute, of dsilu_f) per element of n (float64), first order (module docstring)."""
    s = torch.sigmoid(n)
    t = 1.0 + n * (1.0 - s)
    e_s = (1.25 * n.abs() + 5.0) * U
    e_d = s * (n.abs() * (s * e_s + U * (1.0 - s)) + t.abs() * (e_s + 2.0 * U))
    return e_s, e_d


def apply_bound(n, res, ref, dtype):
    """act = 1: |tdx_gn_apply - ref| per element."""
    s = torch.sigmoid(n)
    e_s, _ = silu_bounds(n)
    r = 0.0 if res is None else res.double().abs()
    return SLACK * (n.abs() * s * e_s + U * ((n * s).abs() + r)) + store_rounding(ref, dtype)


def bwd_bounds(ref, dy, gamma, beta, chain, G, V, dtype):
    """act = 1: bounds of |kernel - ref| for dx (B, V, C), dgamma, dbeta (C), dscale, dshift (B, C).  chain = n_t + rows."""
    t = ref.terms
    B, C = t["P"].shape
    _, e_d = silu_bounds(t["n"])
    D = dy.double().abs() * e_d + U * t["dn"].abs()
    ax = t["xhat"].abs()
    eP = D.sum(1) + chain * U * (t["sum_abs_P"] + D.sum(1))
    eQ = (D * ax).sum(1) + chain * U * (t["sum_abs_Q"] + (D * ax).sum(1))
    N = float(C // G * V)
    group = lambda e: (t["k"].abs() * e).reshape(B, G, C // G).sum(-1) / N
    per_c = lambda e: e.repeat_interleave(C // G, dim=1)[:, None, :]
    eA, eB = group(eP) + 2.0 * U * t["A"].abs(), group(eQ) + 2.0 * U * t["Bq"].abs()
    k1 = (t["rstd"] * t["k"][:, None, :]).abs()
    dx = SLACK * (k1 * D + t["rstd"] * (per_c(eA) + ax * per_c(eB))) + dx_rounding(t, ref.dx, dtype)
    cast = lambda e, r: SLACK * e + U * r.abs()
    f, ga, be = t["film"].abs(), gamma.double().abs(), beta.double().abs()
    return dict(dx=dx, dgamma=cast((f * eQ).sum(0), ref.dgamma), dbeta=cast((f * eP).sum(0), ref.dbeta),
                dscale=None if ref.dscale is None else cast(ga * eQ + be * eP, ref.dscale),
                dshift=None if ref.dshift is None else cast(eP, ref.dshift))


# ---------------------------------------------------------------------------------------- the grid of the statistics pass

StatsGeometry = namedtuple("StatsGeometry", "vpb blocks rows spare per_thread paths tables")


def stats_geometry(B, V, C, deterministic, arena_bytes):
    """The launch of gn_stats_launch, restated: voxels per block, blocks per sample, voxel rows and spare threads of a block,
    the most values one thread adds per channel, the loop paths its lanes take ({(a four-in-flight trip, the tail loop)}, by
    gn_cases.stream_paths: a block walks its voxels with stride `rows`), and whether the blocks store per-block tables that
    gn_stats_merge_kernel adds (deterministic, with room in the arena past its ARENA_HEAD bytes)."""
    round32 = lambda v: (v + 31) // 32 * 32
    vpb = -(-B * V // 128)
    vpb = 32 if vpb < 32 else min(VOX_PER_BLOCK, round32(vpb))
    tables = False
    if deterministic:
        if -(-V // vpb) > DET_MAX_BLOCKS:
            vpb = round32(-(-V // DET_MAX_BLOCKS))
        need = B * -(-V // vpb) * C * 2 * 8
        tables = arena_bytes > 0 and arena_bytes >= ARENA_HEAD + need
        if not tables:
            vpb = round32(V)  # one block per sample
    L = C // 8
    rows = THREADS // L
    blocks = -(-V // vpb)
    sizes = {min(vpb, V - i * vpb) for i in (0, blocks - 1)}  # a whole block and the last one
    paths = set().union(*(stream_paths(rows, n) for n in sizes))
    return StatsGeometry(vpb, blocks, rows, THREADS - rows * L, -(-min(vpb, V) // rows), paths, tables)


def var_bound(per_thread, mean, var):
    """Relative error of the variance the statistics pass gets from NON-integer float32 x: a thread adds per_thread values of x
    and of x^2 in float32 (x^2 rounds once, each add once: relative errors (n_t - 1) u of sum x and n_t u of sum x^2 when x does
    not change sign), the rest is f64.  var = E[x^2] - mean^2 then errs by at most n_t u E[x^2] + 2 (n_t - 1) u mean^2
    <= 3 n_t u (var + mean^2); the (n_t + 1) leaves 3 u (var + mean^2) for the float32 rounding of rstd (2 u (var + eps))."""
    return 3.0 * (per_thread + 1) * U * (1.0 + mean * mean / var)
