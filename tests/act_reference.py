"""tests/gn_reference.py's `apply` and `bwd` restated in float64 with an ACTIVATION argument (the TDX_ACT_* codes of
include/tdx.h), and the error bounds of the device functions of csrc/tdx_act.h.  Inputs, distances and the bound structure are
gn_reference's: `dyadic_inputs(narrow=True)` makes n = fma(x, a, c0) exact with |n| <= N_MAX = 32, so the only errors are those
of f(n), f'(n) and the roundings after them.  No figure here comes from a run of the kernels.

    y = f(n) + res        dn = dy f'(n)        everything after dn as in gn_reference

With u = 2^-24 ("1 ulp" of a hardware instruction: relative error <= 2 u, the AMD ISA documents' figure for v_exp_f32, v_log_f32
and v_rcp_f32; a constant rounds with u, every multiply / add / fma rounds once with u), E_f is the ABSOLUTE error of the device
f(n) including its own last rounding and E_d that of the device f'(n).  `apply_bound` is gn_reference.apply_bound with E_f in
the place of |n| s E_s; `bwd_bounds` is gn_reference.bwd_bounds with E_d in the place of silu_bounds' e_d.  To first order:

SiLU (code 1).  gn_reference's: E_f = |n| s E_s, E_d = silu_bounds(n)[1].

GELU (code 2).  tau = n / sqrt 2, Phi = (1 + erf tau) / 2, phi = exp(-n^2 / 2) / sqrt(2 pi).
  * t = fl(n c1), c1 = fl(1 / sqrt 2): the constant and the product round once each, t = tau (1 + 2 u); erf moves by
    erf'(tau) |tau| 2 u = (4 / sqrt pi) |tau| exp(-tau^2) u.
  * erff is the device library's: it enters at the OpenCL full-profile limit of erf, 16 ulp <= 32 u |erf tau| (only the
    library's bitcode is on a build machine: no tighter figure can be cited).
        E_erf = 32 u |erf tau| + (4 / sqrt pi) |tau| exp(-tau^2) u
  * f = fma(h, e~, h) with h = n / 2 exact:                          E_f = |n| / 2 E_erf + u |f|
  * Phi~ = fma(1/2, e~, 1/2): E_erf / 2 + u Phi.
  * q = v_exp_f32(fl(fl(n n) c2)), c2 = fl(-log2(e) / 2): the square, the constant and the product round once each, the
    argument a = -n^2 log2(e) / 2 is off by 3 u |a|, which moves 2^a by ln 2 |a| 3 u = 1.5 n^2 u; the instruction adds 2 u.
  * m = fl(n c3), c3 = fl(1 / sqrt(2 pi)): 2 u.  f' = fma(m, q, Phi~) rounds once:
        E_d = E_erf / 2 + u Phi + |n phi| (1.5 n^2 + 4) u + u |f'| + TINY
    TINY = 2^-122 covers a q below 2^-126 flushed to zero (|m| < 16).

ReLU (code 3).  A compare and a select: E_f = E_d = 0.  With dyadic inputs relu(n) + res is exact in float32 and dn = dy or 0,
so everything gn_reference proves for act = 0 holds: y is the reference rounded once to T, the parameter gradients are the
reference cast to float32, dx is within `dx_rounding`.

Softplus (code 4; beta = 1, threshold = 20).  n > 20: f = n and f' = 1, a select: E_f = E_d = 0.  Otherwise
f = fma(v_log_f32(1 + w~), fl(ln 2), max(n, 0)), w~ = v_exp_f32(fl(c |n|)), c = fl(-log2 e), w = exp(-|n|), l = log(1 + w):
  * the argument of the exponential as in gn_reference's sigmoid_f: 1.25 |n| u on w; the instruction 2 u: E_w = (1.25 |n| + 2) u
    relative.
  * S = fl(1 + w~): relative error sigma' E_w + u, sigma' = w / (1 + w) = sigmoid(-|n|).  It moves log S by the same amount,
    ABSOLUTE.
  * v_log_f32: 2 u l (in natural units);  fl(ln 2): u l;  the fma rounds once, max(n, 0) is exact:
        E_f = sigma' E_w + u + 3 u l + u |f|
  * f' = sigmoid_f(n), relative error gn_reference's E_s = (1.25 |n| + 5) u:        E_d = s E_s

Tanh (code 5).  f = tanhf(n), the device library's: it enters at the OpenCL full-profile limit of tanh, 5 ulp <= 10 u T with
T = |tanh n| (a multiple of the value: exact at n = 0):                 E_f = 10 u T
  * f' = fma(-t~, t~, 1) of the recomputed t~, one rounding:             E_d = 2 T E_f + u (1 - T^2)

THE STORE TO T.  gn_reference adds ulp_T(ref) for it, which presumes the float32 result in the binade of ref or the next one.
Here f(n) can be far below its own error bound (GELU and Softplus of a very negative n, a dx that cancels), so the store is
bounded at the largest magnitude the float32 result can have: with e the float32 bound, rounding to T errs by at most half the
spacing of T at |ref| + e; `stored` adds that whole spacing, ulp_T(|ref| + e) -- gn_reference's term wherever e < |ref|.

The second-order terms are covered by gn_reference's SLACK = 1 + 2^-10 as there (every first-order relative error above is
below 1600 u, so their products are below 2^-12 of a first-order term).
"""

import math

import torch

from gn_reference import SLACK, U, Bwd, _per_channel, dx_rounding, dyadic_inputs, pre_activation, silu_bounds, store_rounding, ulp_of  # noqa: F401

NONE, SILU, GELU, RELU, SOFTPLUS, TANH = range(6)  # TDX_ACT_*
NAMES = {SILU: "silu", GELU: "gelu", RELU: "relu", SOFTPLUS: "softplus", TANH: "tanh"}
MODULES = {SILU: torch.nn.SiLU, GELU: torch.nn.GELU, RELU: torch.nn.ReLU, SOFTPLUS: torch.nn.Softplus, TANH: torch.nn.Tanh}
THRESHOLD = 20.0
TINY = 2.0**-122
_SQRT2, _SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------------------ the operation


def f(n, act):
    """f(n) in float64"""
    if act == NONE:
        return n
    if act == SILU:
        return n * torch.sigmoid(n)
    if act == GELU:
        return 0.5 * n * (1.0 + torch.erf(n / _SQRT2))
    if act == RELU:
        return torch.where(n > 0, n, torch.zeros_like(n))
    if act == SOFTPLUS:
        return torch.where(n > THRESHOLD, n, torch.log1p(torch.exp(n.clamp_max(THRESHOLD))))
    if act == TANH:
        return torch.tanh(n)
    raise ValueError(act)


def df(n, act):
    """f'(n) in float64"""
    if act == NONE:
        return torch.ones_like(n)
    if act == SILU:
        s = torch.sigmoid(n)
        return s * (1.0 + n * (1.0 - s))
    if act == GELU:
        return 0.5 * (1.0 + torch.erf(n / _SQRT2)) + n * torch.exp(-0.5 * n * n) / _SQRT2PI
    if act == RELU:
        return (n > 0).double()
    if act == SOFTPLUS:
        return torch.where(n > THRESHOLD, torch.ones_like(n), torch.sigmoid(n))
    if act == TANH:
        return 1.0 - torch.tanh(n) ** 2
    raise ValueError(act)


def apply(x, stats, gamma, beta, scale, shift, res, act):
    n, _ = pre_activation(x, stats, gamma, beta, scale, shift)
    y = f(n, act)
    return y if res is None else y + res.double()


def bwd(x, dy, stats, gamma, beta, scale, shift, act, round_group_means=True):
    """gn_reference.bwd with dn = dy f'(n): the five gradients in float64 and `terms`."""
    B, V, C = x.shape
    G = stats.shape[1]
    n, xhat = pre_activation(x, stats, gamma, beta, scale, shift)
    _, rstd = _per_channel(stats, C)
    film = torch.ones(B, C, dtype=torch.float64, device=x.device) if scale is None else 1.0 + scale.double()
    k = gamma.double() * film  # (B, C)
    dact = df(n, act)
    dn = dy.double() * dact
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
    terms = dict(n=n, xhat=xhat, rstd=rstd, k=k, film=film, dn=dn, dact=dact, P=P, Q=Q, A=A, Bq=Bq,
                 dx_terms=k1dn.abs() + k2.abs() + xk3.abs(), sum_abs_P=dn.abs().sum(1), sum_abs_Q=(dn * xhat).abs().sum(1))
    return Bwd(dx, dgamma, dbeta, dscale, dshift, terms)


# ------------------------------------------------------------------------------------------------------------------ bounds


def act_bounds(n, act):
    """(E_f, E_d): absolute errors of the device f(n) and f'(n) per element of n (float64), first order (module docstring)."""
    a = n.abs()
    if act == RELU:
        return torch.zeros_like(n), torch.zeros_like(n)
    if act == SILU:
        s = torch.sigmoid(n)
        e_s, e_d = silu_bounds(n)
        return a * s * e_s, e_d
    if act == GELU:
        tau = n / _SQRT2
        erf = torch.erf(tau)
        e_erf = 32.0 * U * erf.abs() + 4.0 / math.sqrt(math.pi) * tau.abs() * torch.exp(-tau * tau) * U
        Phi, phi = 0.5 * (1.0 + erf), torch.exp(-0.5 * n * n) / _SQRT2PI
        e_f = 0.5 * a * e_erf + U * f(n, act).abs()
        e_d = 0.5 * e_erf + U * Phi + (n * phi).abs() * (1.5 * n * n + 4.0) * U + U * df(n, act).abs() + TINY
        return e_f, e_d
    if act == SOFTPLUS:
        w = torch.exp(-a)
        e_w = (1.25 * a + 2.0) * U
        e_f = w / (1.0 + w) * e_w + U + 3.0 * U * torch.log1p(w) + U * f(n, act).abs()
        e_s, _ = silu_bounds(n)
        e_d = torch.sigmoid(n) * e_s
        linear = n > THRESHOLD
        return torch.where(linear, torch.zeros_like(n), e_f), torch.where(linear, torch.zeros_like(n), e_d)
    if act == TANH:
        T = torch.tanh(a)
        e_f = 10.0 * U * T
        return e_f, 2.0 * T * e_f + U * (1.0 - T * T)
    raise ValueError(act)


def stored(e, ref, dtype):
    """e, a bound of |float32 result - ref|, plus the store of that result to `dtype` (module docstring)"""
    return e if dtype == torch.float32 else e + ulp_of(ref.abs() + e, dtype)


def apply_bound(n, res, ref, dtype, act):
    """|tdx_gn_apply(act) - ref| per element: gn_reference.apply_bound with E_f for |n| s E_s."""
    e_f, _ = act_bounds(n, act)
    r = 0.0 if res is None else res.double().abs()
    return stored(SLACK * (e_f + U * (f(n, act).abs() + r)), ref, dtype)


def bwd_bounds(ref, dy, gamma, beta, chain, G, V, dtype, act):
    """gn_reference.bwd_bounds with E_d for silu_bounds' e_d: bounds of |kernel - ref| for dx (B, V, C), dgamma, dbeta (C),
    dscale, dshift (B, C).  chain = n_t + rows."""
    t = ref.terms
    B, C = t["P"].shape
    _, e_d = act_bounds(t["n"], act)
    D = dy.double().abs() * e_d + U * t["dn"].abs()
    ax = t["xhat"].abs()
    eP = D.sum(1) + chain * U * (t["sum_abs_P"] + D.sum(1))
    eQ = (D * ax).sum(1) + chain * U * (t["sum_abs_Q"] + (D * ax).sum(1))
    N = float(C // G * V)
    group = lambda e: (t["k"].abs() * e).reshape(B, G, C // G).sum(-1) / N
    per_c = lambda e: e.repeat_interleave(C // G, dim=1)[:, None, :]
    eA, eB = group(eP) + 2.0 * U * t["A"].abs(), group(eQ) + 2.0 * U * t["Bq"].abs()
    k1 = (t["rstd"] * t["k"][:, None, :]).abs()
    dx = stored(SLACK * (k1 * D + t["rstd"] * (per_c(eA) + ax * per_c(eB))) + dx_rounding(t, ref.dx, torch.float32), ref.dx, dtype)
    cast = lambda e, r: SLACK * e + U * r.abs()
    fl, ga, be = t["film"].abs(), gamma.double().abs(), beta.double().abs()
    return dict(dx=dx, dgamma=cast((fl * eQ).sum(0), ref.dgamma), dbeta=cast((fl * eP).sum(0), ref.dbeta),
                dscale=None if ref.dscale is None else cast(ga * eQ + be * eP, ref.dscale),
                dshift=None if ref.dshift is None else cast(eP, ref.dshift))
