"""A plain float64 reference of the 1x1 convolution family (csrc/tdx_conv1.hip, tdx_conv1_mfma.hip, tdx_conv1_mfma_f32.hip), the
inputs for which those kernels are EXACT, and the error bounds where they are not.  It uses neither the kernels nor the oracle
and runs on whatever device its inputs are on (tests/test_conv1_reference.py holds it against float64 F.conv3d and autograd).

    forward   y[r, n]    = bias[n] + sum_k [x1 | x2][r, k] w[k, n] + add[r, n]                       `forward`
    tail      add[r, n]  = silu(fma(h[r, n], ka, c0)),  ka = rstd gamma,  c0 = beta - mean rstd gamma     `tail`
    gradient  dW[k, n]   = sum_r x[r, k] dy[r, n],   dbias[n] = sum_r dy[r, n]                            `wgrad`
    data gradient        = forward(dy, None, W[:, col : col + C], None, add) on a block of the (Cout, Cin) weight

Notation: u = 2^-24 (unit roundoff of float32), T the storage format, round_T round-to-nearest-even to T, ulp_T(v) the spacing
of T at |v|, gamma_n = n u / (1 - n u).

WHERE EACH ROUTE ROUNDS (routes: conv1_cases).  All three accumulate in float32.
  * V (conv1_fwd_kernel<T>) and F (conv1_f32_mfma_fwd_kernel): v = acc; v += bias; v += add in float32, ONE rounding to T by
    the store (`stf`: __float2bfloat16 / the (f16) cast, both to nearest even; none for float32):   y = round_T((acc + bias) + add)
  * H (conv1_mfma_fwd_kernel): acc + bias goes through LDS as T (`H16::pack2`), is widened again, the addend is added in
    float32 and the sum is stored (`Vec8::store`, the same conversion):       y0 = round_T(acc + bias),  y = round_T(y0 + addend)
    Without an addend the second rounding is the identity and the two forms coincide.
  `rounded_once` and `rounded_twice` are the two forms; every case is compared with the form of its route.
  H stages the float32 weights as T: `H16::pack2` is __builtin_convertvector of a float pair to __bf16 / _Float16, which the
  compiler lowers to v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 under the default rounding mode: round to nearest, ties to even --
  the rounding of torch's `.to(T)`.  For H the reference is therefore given `w.to(T)`; V and F read w as float32.
  The weight gradients are float32 sums of products of T values, stored as float32: no storage rounding on any route.

EXACT INPUTS (`exact_inputs`).  x and dy are integers in [-4, 4]; w = m 2^-e with an integer |m| <= 127 and e in 7 .. 11 (7
significant bits: it survives bf16 and fp16; |w| < 1); bias is a multiple of 1/4 in [-2, 2], add a multiple of 1/4 in [-4, 4];
the prefill of an accumulated gradient is an integer in [-50, 50].  Every product x w is a multiple of 2^-11 with |x w| < 4, so
every partial sum of at most Cin <= 1024 products, bias and add, IN ANY ORDER, is a multiple of 2^-11 below
(4 * 1024 + 6) * 2^11 < 2^24 units: exact in float32's 24 bits, whatever the order the MFMA pipeline, the K slices or the two
inputs are walked in.  x dy is an integer with |x dy| <= 16: sums over at most 4097 rows plus the prefill stay below 2^17,
again exact in any order -- atomics in arrival order, per-split slabs added in slab order, and accumulation onto the prefill
all give THE integer.  `assert_exact` proves both from the reference alone (units and the sum of absolute terms), for the rows
it is given.  Hence, bit for bit (torch.equal):
  forward, data gradient = the reference rounded at the route's rounding points;   dW, dbias = the reference cast to float32.
  `narrow=True` is the family for rows WITH an addend: at most 8 non-zero weights per column, each +-1/2 or +-1, so that
  |acc + bias| <= 34 and is a multiple of 1/4 -- at most 136 units of 1/4, 8 significant bits: y0 is representable in bf16 and fp16 and the two rounding
  forms coincide.  The dense family (the default) is the one whose acc + bias is NOT representable in 16 bits (units of 2^-11
  at magnitudes of 1 .. 100: 12 bits and more): with an addend and a 16-bit T the two forms differ, and each route must give
  its own.

INEXACT INPUTS (Gaussian).  First order, times SLACK = 1 + 2^-10 for the second-order terms like gn_reference.
  * forward (`forward_bound`): a float32 dot product of K terms in any order errs by at most gamma_K sum_k |x_k w_k| (the
    products round on V and F and are exact on H; each term then passes through at most K - 1 additions); the bias and the
    addend are two more additions:        gamma_(Cin + 2) (sum_k |x_k w_k| + |bias| + |add|)  +  ulp_T(ref) per storage rounding
    -- one on V and F (none for float32, where the last addition's rounding is among the Cin + 2), two on H with an addend
    (ulp_T(y0) + ulp_T(y)).  A float32 value within the same or the next binade of ref rounds to T within ulp_T(ref).
  * weight gradient (`wgrad_bound`): the per-split loop, the merge of the four wave tiles, the atomics or the ordered sum of the
    slabs and the accumulation are ONE summation tree whose leaves are the `rows` products (accumulators and slabs start at
    zero, and adding to zero is exact).  A leaf passes through its product's rounding (none on H, whose products of T values
    are exact) and at most rows - 1 additions:                                        gamma_rows sum_r |x dy|
    and with accumulate = 1 the prefill is one more leaf and every leaf may pass one more addition:
                                                                          gamma_(rows + 1) (sum_r |x dy| + |prefill|)
    with |prefill| the element accumulated onto (of the dW buffer for dW, of the dbias buffer for dbias; dbias has no
    products: gamma_(rows - 1) would do, gamma_rows is used).  This is loose (it grows with rows where the error grows with
    its root): the exact rows are the sharp check of the weight gradient, these show that rounded operands change nothing.
  * fused tail (`tail_bound`).  The kernel forms ka = fl(rstd gamma) (one rounding: u |ka|) and c0 = beta - mean rstd gamma,
    which the compiler may contract: fl(fl(mean rstd) gamma) then a subtraction, or one fma -- either way at most
    2 u |mean rstd gamma| + u |c0|.  n~ = fma(h, ka~, c0~) is then off by
        d_n = u |h ka| + 2 u |mean rstd gamma| + u |c0| + u |n|
    silu' is bounded by 1.1, so silu(n~) moves by at most 1.1 d_n; silu_f itself is gn_reference's
    |n| s E_s + u |n s| (`silu_bounds`: v_exp_f32 and v_rcp_f32 at 1 ulp each, from the AMD ISA documents; |n| <= N_MAX);
    the float32 addition y0 + silu rounds once (u |y|), the store once (ulp_T).  y0 itself carries `forward_bound` without
    its addend (for exact conv inputs: nothing but the exact round_T(acc + bias), which the reference then uses as it is).
  * fused tail against the two launches it replaces (`tail_two_launch_bound`; exact rows only: y0 = round_T(acc + bias) and n
    are then the same numbers in both, and both evaluate the same silu_f(n) = fl(n s~)).  tdx_gn_apply adds the residual as
    fma(n, s~, y0), one rounding of the true n s~ + y0; the fused kernel forms fl(fl(n s~) + y0), or the same fma where the
    compiler contracts it.  Before the store the two float32 values are within u |n s~| + 2 u |y| of each other, bounded as
    2 u (|silu(n)| + |y|); rounding two values that close to T gives the same number or, where a rounding boundary of T
    lies between them, neighbours:                                             2 u (|silu(n)| + |y|) + ulp_T(y)
No element is left out of any comparison and no figure here comes from a run of the kernels.
"""

import torch

import gn_reference as G

U, SLACK, N_MAX = G.U, G.SLACK, G.N_MAX
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = 2.0**-11  # of the exact forward's products and sums


# ----------------------------------------------------------------------------------------------------------- the operation


def _cat(x1, x2):
    return x1.double() if x2 is None else torch.cat((x1.double(), x2.double()), dim=-1)


def forward(x1, x2, w, bias, add):
    """(y0, y) float64: y0 = bias + [x1 | x2] @ w, y = y0 + add.  w (Cin, Cout): the caller passes it as the route reads it
    (rounded to T for H) and already cut to its column block."""
    y0 = _cat(x1, x2) @ w.double()
    if bias is not None:
        y0 = y0 + bias.double()
    return y0, (y0 if add is None else y0 + add.double())


def weight_block(w2, col, C):
    """The (Cout, C) block w2[:, col : col + C] of a (Cout, Cin) weight, as the data gradient reads it: its [k][n] matrix."""
    return w2[:, col:col + C]


def tail(h, stats, gamma, beta, groups):
    """(n, silu(n)) float64 (B, V, C): the addend of the fused tail; stats (B, G, 2) = mean, rstd"""
    assert stats.shape[1] == groups and h.shape[-1] % groups == 0
    n, _ = G.pre_activation(h, stats, gamma, beta, None, None)
    return n, n * torch.sigmoid(n)


def wgrad(x, dy):
    """dW (Cin, Cout), dbias (Cout) float64"""
    return x.double().t() @ dy.double(), dy.double().sum(0)


def _round(t, dt):
    """float64 -> T with ONE rounding: through float32 only where that step is exact"""
    assert torch.equal(t.float().double(), t), "not exact in float32: rounding to T through float32 would round twice"
    return t.float().to(dt)


def rounded_once(y0, add, dt):
    """V and F: round_T((acc + bias) + add), for values exact in float32"""
    return _round(y0 if add is None else y0 + add.double(), dt)


def rounded_twice(y0, add, dt):
    """H: round_T(round_T(acc + bias) + add)"""
    t = _round(y0, dt)
    return t if add is None else _round(t.double() + add.double(), dt)


def rounded(route, y0, add, dt):
    return rounded_twice(y0, add, dt) if route == "H" else rounded_once(y0, add, dt)


# ------------------------------------------------------------------------------------------------------------------ inputs


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_inputs(rows, C1, C2, Cout, seed=0, narrow=False):
    """CPU float32 tensors x1 (rows, C1), x2 (rows, C2) or None, w (Cin, Cout), bias (Cout), add, dy (rows, Cout): see the
    module docstring.  Every value is the same number in f32, bf16, fp16."""
    g = torch.Generator().manual_seed(1000 + seed)
    Cin = C1 + C2
    if narrow:
        w = torch.zeros(Cin, Cout)
        k = torch.stack([torch.randperm(Cin, generator=g)[:min(8, Cin)] for _ in range(Cout)], dim=1)  # (<= 8, Cout) distinct rows
        vals = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(4, k.shape, generator=g)]
        w.scatter_(0, k, vals)
    else:
        w = _ints((Cin, Cout), -127, 127, g) * torch.ldexp(torch.ones(()), -_ints((Cin, Cout), 7, 11, g).int())
    return dict(x1=_ints((rows, C1), -4, 4, g), x2=_ints((rows, C2), -4, 4, g) if C2 else None, w=w,
                bias=_ints((Cout,), -8, 8, g) / 4, add=_ints((rows, Cout), -16, 16, g) / 4, dy=_ints((rows, Cout), -4, 4, g))


PREFILL = 50


def prefill(shape, seed=0, exact=True):
    """What a gradient buffer holds before the call: integers in [-PREFILL, PREFILL] (exact rows) or Gaussian; CPU float32"""
    g = torch.Generator().manual_seed(4000 + seed)
    return _ints(shape, -PREFILL, PREFILL, g) if exact else torch.randn(*shape, generator=g)


def gaussian_inputs(rows, C1, C2, Cout, dt, seed=0):
    """The same keys, Gaussian, activations rounded to T; w ~ N(0, 1 / Cin) stays float32 (H rounds it while staging)."""
    g = torch.Generator().manual_seed(2000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    Cin = C1 + C2
    q = lambda t: t.to(dt).float()
    return dict(x1=q(rn(rows, C1)), x2=q(rn(rows, C2)) if C2 else None, w=rn(Cin, Cout) * Cin**-0.5, bias=rn(Cout),
                add=q(rn(rows, Cout)), dy=q(rn(rows, Cout)))


def tail_inputs(B, V, Cout, groups, seed=0, exact=True, dt=torch.float32):
    """h (B, V, Cout), stats (B, G, 2), gamma, beta: gn_reference.dyadic_inputs(narrow=True) -- n exact, |n| <= 28 -- or Gaussian"""
    if exact:
        p = G.dyadic_inputs((B, Cout, groups, V), seed=seed, narrow=True)
        return dict(h=p["x"], stats=p["stats"], gamma=p["gamma"], beta=p["beta"])
    g = torch.Generator().manual_seed(3000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    h = (rn(B, V, Cout) * 1.7 + 0.3).to(dt).float()
    return dict(h=h, stats=G.stats(h, groups, 1e-5).float(), gamma=1.0 + 0.5 * rn(Cout), beta=0.2 * rn(Cout))


def _units(name, t, unit, limit=2.0**24):
    q = t.double() / unit
    assert torch.equal(q, q.round()), f"{name} is not a multiple of {unit}"
    assert q.abs().max().item() < limit, f"{name} reaches {q.abs().max().item()} units of {unit}: not below 2^24"


def assert_exact(p, bias=True, add=True, narrow=False):
    """The preconditions of the exact rows, from the reference alone (module docstring)."""
    x = _cat(p["x1"], p["x2"])
    for dt in DTYPES.values():  # the same numbers in every storage format
        for k in ("x1", "x2", "w", "add", "dy"):
            assert p[k] is None or torch.equal(p[k].to(dt).float(), p[k]), f"{k} does not survive {dt}"
    # forward: the sum of |terms| bounds every partial sum in every order
    mag = x.abs() @ p["w"].double().abs() + p["bias"].double().abs() + p["add"].double().abs()
    _units("sum |x w| + |bias| + |add|", mag, UNIT)
    _units("x", x, 1.0), _units("w", p["w"], UNIT), _units("bias", p["bias"], 0.25), _units("add", p["add"], 0.25)
    # the data gradient: dy against any block of w^T has the same terms as sum_n |dy w|
    _units("sum |dy w|", p["dy"].double().abs() @ p["w"].double().abs().t(), UNIT)
    # weight gradient: integers; sum_r |x dy| + |prefill| below 2^24
    _units("dy", p["dy"], 1.0)
    pre = float(PREFILL)
    _units("sum |x dy| + |prefill|", x.abs().t() @ p["dy"].double().abs() + pre, 1.0)
    _units("sum |dy| + |prefill|", p["dy"].double().abs().sum(0) + pre, 1.0)
    y0, _ = forward(p["x1"], p["x2"], p["w"], p["bias"] if bias else None, None)
    for dt in DTYPES.values():
        t = _round(y0, dt)
        if add:
            _round(t.double() + p["add"].double(), dt)  # asserts that H's float32 addition y0 + add is exact
        if narrow:
            assert torch.equal(t.double(), y0), "narrow family: acc + bias must be representable in every T"


# ------------------------------------------------------------------------------------------------------------------ bounds


def gamma_n(n):
    return n * U / (1.0 - n * U)


def magnitude(x1, x2, w, bias, add):
    m = _cat(x1, x2).abs() @ w.double().abs()
    if bias is not None:
        m = m + bias.double().abs()
    return m if add is None else m + add.double().abs()


def forward_bound(route, x1, x2, w, bias, add, y0, y, dt):
    """|kernel - y| per element; w as the route reads it"""
    Cin = x1.shape[-1] + (0 if x2 is None else x2.shape[-1])
    b = SLACK * gamma_n(Cin + 2) * magnitude(x1, x2, w, bias, add) + G.store_rounding(y, dt)
    if route == "H" and add is not None:
        b = b + G.ulp_of(y0, dt)
    return b


def wgrad_bound(x, dy, pre_w=None, pre_b=None):
    """(bound of dW (Cin, Cout), bound of dbias (Cout)).  pre_w (Cin, Cout), pre_b (Cout): what the call accumulates onto,
    element for element; None (both) without accumulate."""
    sw, sb = x.double().abs().t() @ dy.double().abs(), dy.double().abs().sum(0)
    rows = x.shape[0]
    if pre_w is None:
        g = SLACK * gamma_n(rows)
        return g * sw, g * sb
    g = SLACK * gamma_n(rows + 1)
    return g * (sw + pre_w.double().abs()), g * (sb + pre_b.double().abs())


def tail_bound(h, stats, gamma, beta, n, y0_bound, y0, y, dt):
    """|tdx_conv1_fwd_gn - (y0 + silu(n))| per element.  y0_bound: what y0 = round_T(acc + bias) may be off by (0 where the
    conv inputs are exact and the reference holds the rounded y0 itself)."""
    mean, rstd = G._per_channel(stats, h.shape[-1])
    ka = rstd * gamma.double()
    mrg = (mean * ka).abs()
    c0 = beta.double() - mean * ka
    d_n = U * ((h.double() * ka).abs() + 2.0 * mrg + c0.abs() + n.abs())
    s = torch.sigmoid(n)
    e_s, _ = G.silu_bounds(n)
    silu_err = 1.1 * d_n + n.abs() * s * e_s + U * (n * s).abs()
    return SLACK * (silu_err + U * y.abs()) + y0_bound + G.store_rounding(y, dt)


def tail_two_launch_bound(silu, y, dt):
    """|tdx_conv1_fwd_gn - (tdx_conv1_fwd, then tdx_gn_apply with that residual)| per element, on exact inputs"""
    return SLACK * 2.0 * U * (silu.abs() + y.abs()) + G.ulp_of(y, dt)
