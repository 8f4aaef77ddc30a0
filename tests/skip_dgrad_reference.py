"""Float64 reference, exact inputs and element-wise bounds of the input gradient of a ResnetBlock with a projected (1x1) skip,

    dx = d/dx [ <conv3d(replicate_pad(x), W1), dh1> + <conv1x1(x, wr), gy> ]
       = adjoint3x3x3(dh1) + gy . wr                                   (linear in x: the point x is taken at does not matter)

shared by tests/test_skip_dgrad_gpu.py (the kernels) and tests/test_skip_dgrad_host.py (the reference against autograd of the
expression above, on the CPU).  It uses neither the kernels nor the oracle.

Notation as in conv1_reference: u = 2^-24, T the storage format, ulp_T(v) the spacing of T at |v|, gamma_n = n u / (1 - n u),
SLACK = 1 + 2^-10 for second-order terms.

THE PIECES.  G = the gradient w.r.t. the PADDED input (X + 2)(Y + 2)(Z + 2), by autograd of the unpadded float64 conv3d.  Its
interior is the zero-padded correlation the data-gradient kernels compute as their main term (`adj_main`); each of its halo
positions is one term of the halo shell, folded onto the voxel it clamps to: a voxel that lies on f of the six faces receives
2^f - 1 of them (1 on a face, 3 on an edge, 7 at a corner).  `ref` = fold(G) + gy . wr; the fold is the adjoint of replicate
padding, again by autograd.  `folds` = 2^f - 1 per voxel, `fold_abs` = the fold of |G| over the halo alone.

EXACT INPUTS (`exact_inputs`).  dh1 and gy are integers in [-4, 4]; every weight is m 2^-e with an integer |m| <= 127 and e in
7 .. 11: the same numbers in f32, bf16 and fp16, |w| < 1.  Every product is a multiple of 2^-11; a voxel sums at most
8 x 27 x Cout + Cout of them (a corner).  `assert_exact` shows from the reference alone that the sum of |products| of every
element stays below 2^24 units of 2^-11 (it reaches about 2^21 at the corners of the cases used): every partial sum in any
order is then exact in float32, so the fp32 accumulation of the matrix cores is EXACT and what remains are the roundings to T.

WHERE EACH ROUTE ROUNDS TO T, and the bound per element (`bounds`).  n = 27 Cout (folds + 1) + Cout products per voxel (the
issue's 27 Cout + Cout at an interior voxel); mag = the same sum over |products|.
  * fused (tdx_conv3_bwd_data_skip): the accumulator holds main + gy . wr =: M and is stored ONCE.  Interior voxel: M = ref,
        gamma_n mag + ulp_T(ref).
    Voxel on a face: the shell terms are added onto the stored value one at a time, each addition rounded to T.  The value a
    fold stores is a partial sum M + (some of the shell terms), of magnitude at most P = |M| + fold_abs, so each of the
    `folds` roundings is within ulp_T(P):        gamma_n mag + ulp_T(M) + folds ulp_T(P)            (at most 7 folds, at a corner)
    (ulp_T(ref) would not be sound there: where the shell cancels the main term, ref is small and the stored partial sums are not.
    A rounding to nearest is within HALF a spacing; counting a whole ulp_T per storage rounding, as the route tests of the 1x1
    and GroupNorm kernels do, also covers the shell term's own conversion to T, which the packed 16-bit atomics need: that
    term is at most fold_abs <= P in magnitude.)
  * two launches (tdx_conv3_bwd_data, then tdx_conv1_fwd with the adjoint as its addend): the adjoint's main term is stored
    (ulp_T(adj_main)), the folds land on it (folds ulp_T(|adj_main| + fold_abs)), and the 1x1 kernel's matrix-core route rounds
    gy . wr to T in LDS (ulp_T(skip), conv1_reference route H) before it adds the addend and stores (ulp_T(ref)):
        gamma_n mag + ulp_T(adj_main) + folds ulp_T(|adj_main| + fold_abs) + ulp_T(skip) + ulp_T(ref)
    At an interior voxel that is three roundings against the fused route's one, and the fused bound is the smaller of the two
    by at least ulp_T(adj_main) + ulp_T(skip): the test asserts that, and holds the fused result to the fused bound everywhere.
For float32 tensors (old route only) no term of ulp_T appears; the folds' fp32 additions are among the n of gamma_n.
No figure here comes from a run of the kernels.
"""

import torch
import torch.nn.functional as F

import gn_reference as G

U, SLACK = G.U, G.SLACK
UNIT = 2.0**-11


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _dyadic(shape, g):
    return _ints(shape, -127, 127, g) * torch.ldexp(torch.ones(()), -_ints(shape, 7, 11, g).int())


def exact_inputs(B, grid, C1, C2, Cout, seed=0):
    """CPU float32: dh1, gy (B, X, Y, Z, Cout), w1 (Cout, Cin, 3, 3, 3), wr (Cout, Cin); every value survives bf16 and fp16."""
    g = torch.Generator().manual_seed(7000 + seed)
    Cin = C1 + C2
    return dict(dh1=_ints((B, *grid, Cout), -4, 4, g), gy=_ints((B, *grid, Cout), -4, 4, g), w1=_dyadic((Cout, Cin, 3, 3, 3), g),
                wr=_dyadic((Cout, Cin), g), C1=C1, C2=C2)


def _ncv(t):
    return t.double().permute(0, 4, 1, 2, 3).contiguous()


def _nvc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _padded_grad(dh1, w1):
    """G (B, Cin, X + 2, Y + 2, Z + 2): gradient of <conv3d(xp, w1), dh1> w.r.t. the padded input xp"""
    B, X, Y, Z, _ = dh1.shape
    xp = torch.zeros(B, w1.shape[1], X + 2, Y + 2, Z + 2, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv3d(xp, w1.double()), xp, _ncv(dh1))
    return g


def _fold(gp):
    """adjoint of replicate padding: (B, C, X + 2, Y + 2, Z + 2) -> (B, C, X, Y, Z)"""
    B, C, Xp, Yp, Zp = gp.shape
    x = torch.zeros(B, C, Xp - 2, Yp - 2, Zp - 2, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.pad(x, (1, 1, 1, 1, 1, 1), mode="replicate"), x, gp)
    return g


def _halo(gp):
    h = gp.clone()
    h[:, :, 1:-1, 1:-1, 1:-1] = 0
    return h


def fold_counts(grid):
    """2^f - 1 per voxel (X, Y, Z), f = the number of faces the voxel lies on"""
    f = torch.zeros(grid, dtype=torch.int64)
    for a, n in enumerate(grid):
        on = torch.zeros(n, dtype=torch.int64)
        on[0] += 1
        on[-1] += 1  # (an extent of 1 would count both faces: not used)
        f += on.reshape([n if k == a else 1 for k in range(3)])
    return 2**f - 1


def reference(p):
    """float64 (B, X, Y, Z, Cin) tensors: ref, adj_main, skip, fold_abs, mag; folds (X, Y, Z) int64; n (X, Y, Z) float64"""
    dh1, gy, w1, wr = p["dh1"], p["gy"], p["w1"], p["wr"]
    Cout = w1.shape[0]
    gp = _padded_grad(dh1, w1)
    skip = gy.double() @ wr.double()
    adj = _nvc(_fold(gp))
    mag = _nvc(_fold(_padded_grad(dh1.abs(), w1.abs()))) + gy.double().abs() @ wr.double().abs()
    folds = fold_counts(tuple(dh1.shape[1:4]))
    return dict(ref=adj + skip, adj_main=_nvc(gp[:, :, 1:-1, 1:-1, 1:-1]), skip=skip, fold_abs=_nvc(_fold(_halo(gp).abs())), mag=mag,
                folds=folds, n=(27.0 * Cout * (folds + 1) + Cout).double())


def direct(p):
    """The issue's definition, by autograd of the whole expression in float64 (the host test holds `reference` against it)."""
    dh1, gy, w1, wr = p["dh1"], p["gy"], p["w1"], p["wr"]
    B, X, Y, Z, _ = dh1.shape
    x = torch.zeros(B, w1.shape[1], X, Y, Z, dtype=torch.float64, requires_grad=True)
    h = F.conv3d(F.pad(x, (1, 1, 1, 1, 1, 1), mode="replicate"), w1.double())
    s = F.conv3d(x, wr.double()[:, :, None, None, None])
    (g,) = torch.autograd.grad((h * _ncv(dh1)).sum() + (s * _ncv(gy)).sum(), x)
    return _nvc(g)


def assert_exact(p, r):
    for dt in (torch.bfloat16, torch.float16):
        for k in ("dh1", "gy", "w1", "wr"):
            assert torch.equal(p[k].to(dt).float(), p[k]), f"{k} does not survive {dt}"
    q = r["mag"] / UNIT
    assert torch.equal(q, q.round()) and q.max().item() < 2.0**24, "a sum of |products| is not below 2^24 units of 2^-11"


def gamma_n(n):
    return n * U / (1.0 - n * U)


def bounds(r, dt):
    """(fused, two_launch): |kernel - ref| per element, float64 (B, X, Y, Z, Cin)"""
    folds = r["folds"].double()[None, :, :, :, None]
    common = SLACK * gamma_n(r["n"])[None, :, :, :, None] * r["mag"]
    if dt == torch.float32:
        return common, common
    ulp = lambda v: G.ulp_of(v, dt)
    M = r["adj_main"] + r["skip"]
    fused = common + ulp(M) + folds * ulp(M.abs() + r["fold_abs"])
    two = common + ulp(r["adj_main"]) + folds * ulp(r["adj_main"].abs() + r["fold_abs"]) + ulp(r["skip"]) + ulp(r["ref"])
    return fused, two


def interior(grid):
    """bool (X, Y, Z): voxels on no face"""
    return fold_counts(grid) == 0
