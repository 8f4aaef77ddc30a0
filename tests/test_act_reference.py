"""tests/act_reference.py against float64 autograd of module(F.group_norm(x) * (1 + scale) + shift) + res, per activation of the
reference's `actfn` choices (torch's module at its default arguments), by the method and tolerance of
tests/test_gn_reference.py::test_reference_is_the_autograd_of_group_norm; and the bounds' own sanity.  No GPU."""

import math

import pytest
import torch
import torch.nn.functional as F

import act_reference as A
import gn_cases as cases
import gn_reference as R

FLAGS = [(film, res) for film in (False, True) for res in (False, True)]
CODES = list(A.NAMES)


@pytest.mark.parametrize("act", CODES, ids=[A.NAMES[c] for c in CODES])
@pytest.mark.parametrize("film,res", FLAGS)
def test_reference_is_the_autograd_of_the_module(film, res, act):
    B, C, G, V = 2, 24, 3, 37
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, r, dy = 1.5 * rn(B, V, C) + 0.3, rn(B, V, C), rn(B, V, C)
    # gamma of 8: n reaches past Softplus's threshold of 20 on both sides of it, and far into every function's tails
    gamma, beta, scale, shift = 8 * (1 + 0.3 * rn(C)), 0.2 * rn(C), 0.5 * rn(B, C), 0.5 * rn(B, C)
    eps = 1e-5
    leaves = [t.clone().requires_grad_() for t in (x, gamma, beta, scale, shift, r)]
    xa, ga, ba, sa, ha, ra = leaves
    n = F.group_norm(xa.transpose(1, 2), G, ga, ba, eps).transpose(1, 2)
    if film:
        n = n * (1 + sa[:, None, :]) + ha[:, None, :]
    assert (n > A.THRESHOLD).any() and (n < -A.THRESHOLD).any()
    y = A.MODULES[act]()(n)
    y = y + ra if res else y
    y.backward(dy)

    st = R.stats(x, G, eps)
    sc, sh = (scale, shift) if film else (None, None)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert close(A.apply(x, st, gamma, beta, sc, sh, r if res else None, act), y.detach())
    ref = A.bwd(x, dy, st, gamma, beta, sc, sh, act, round_group_means=False)
    assert close(ref.dx, xa.grad) and close(ref.dgamma, ga.grad) and close(ref.dbeta, ba.grad)
    if film:
        assert close(ref.dscale, sa.grad) and close(ref.dshift, ha.grad)


@pytest.mark.parametrize("act", [A.NONE, A.SILU])
def test_codes_0_and_1_are_gn_reference(act):
    p = R.dyadic_inputs((2, 64, 8, 1000), narrow=True)
    args = (p["stats"], p["gamma"], p["beta"], p["scale"], p["shift"])
    assert torch.equal(A.apply(p["x"], *args, p["res"], act), R.apply(p["x"], *args, p["res"], bool(act)))
    a, b = A.bwd(p["x"], p["dy"], *args, act), R.bwd(p["x"], p["dy"], *args, bool(act))
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("dx", "dgamma", "dbeta", "dscale", "dshift"))
    if act == A.SILU:  # and the bounds: E_f = |n| s E_s gives gn_reference.apply_bound up to the store term's argument
        n = a.terms["n"]
        ref = A.apply(p["x"], *args, p["res"], act)
        assert torch.equal(A.apply_bound(n, p["res"], ref, torch.float32, act), R.apply_bound(n, p["res"], ref, torch.float32))
        mine = A.bwd_bounds(a, p["dy"], p["gamma"], p["beta"], 12, 8, 1000, torch.float32, act)
        theirs = R.bwd_bounds(b, p["dy"], p["gamma"], p["beta"], 12, 8, 1000, torch.float32)
        assert all(torch.equal(mine[k], theirs[k]) for k in mine)


def test_bounds_are_what_the_docstring_derives():
    """Spot values, worked by hand from the module docstring (u = 2^-24)."""
    u = R.U
    n = torch.tensor([0.0, 1.0, -3.0, 21.0], dtype=torch.float64)
    e_f, e_d = A.act_bounds(n, A.RELU)
    assert not e_f.any() and not e_d.any()
    e_f, e_d = A.act_bounds(n, A.TANH)
    assert e_f[0].item() == 0.0 and e_d[0].item() == u  # tanh 0 = 0 exactly; the fma rounds once
    T = math.tanh(3.0)
    assert abs(e_f[2].item() - 10 * u * T) < 1e-22 and abs(e_d[2].item() - (20 * u * T * T + u * (1 - T * T))) < 1e-22
    e_f, e_d = A.act_bounds(n, A.SOFTPLUS)
    assert e_f[3].item() == 0.0 and e_d[3].item() == 0.0  # past the threshold: a select
    ln2 = torch.log(torch.tensor(2.0, dtype=torch.float64)).item()
    assert abs(e_f[0].item() - (0.5 * 2 * u + u + 3 * u * ln2 + u * ln2)) < 1e-22
    assert abs(e_d[0].item() - 0.5 * 5 * u) < 1e-22
    e_f, e_d = A.act_bounds(n, A.GELU)
    assert e_f[0].item() == 0.0  # h = 0
    assert abs(e_d[0].item() - (u * 0.5 + u * 0.5 + A.TINY)) < 1e-22  # erf 0 = 0: u Phi + u f'
    # everywhere on the inputs' range the first-order relative errors stay below the 1600 u the SLACK argument uses
    n = torch.linspace(-32, 32, 4097, dtype=torch.float64)
    assert (1.5 * n * n + 4).max().item() < 1600 and (1.25 * n.abs() + 5).max().item() < 1600


def test_stored_covers_a_result_far_below_its_error_bound():
    ref = torch.tensor([1.0, 1e-12], dtype=torch.float64)
    e = torch.tensor([1e-7, 1e-5], dtype=torch.float64)
    got = A.stored(e, ref, torch.bfloat16)
    assert got[0].item() == 1e-7 + 2.0**-7  # e < |ref|: gn_reference's ulp_T(ref)
    assert got[1].item() == 1e-5 + 2.0**-24  # the spacing of bf16 at 1e-5 (2^-17 <= 1e-5 < 2^-16)
    assert A.stored(e, ref, torch.float32) is e


@pytest.mark.parametrize("shape", cases.SMALL, ids=["x".join(map(str, s)) for s in cases.SMALL])
def test_inputs_reach_every_branch(shape):
    """What tests/test_act_gpu.py asserts again before it launches: n is exact, within N_MAX, 0 somewhere at every multi-voxel
    shape (ReLU's derivative at 0), and at (3, 512, 8, 150) with FiLM on both sides of Softplus's threshold."""
    for seed in (0, 1):
        p = R.dyadic_inputs(shape, seed=seed, narrow=True)
        for film in (False, True):
            R.assert_exact(p, film, True)
            sc, sh = (p["scale"], p["shift"]) if film else (None, None)
            n, _ = R.pre_activation(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh)
            if shape[3] > 5 and seed == 0:
                assert (n == 0).any()
            if shape == (3, 512, 8, 150) and film:
                assert int((n > A.THRESHOLD).sum()) == {0: 54, 1: 19}[seed] and n.numel() == 230400
            # ReLU: dn = dy or 0 keeps the act = 0 exactness of P and Q (gn_reference.assert_exact's sums, by |dn| <= |dy|)
            xhat_unit = 0.25
            q = p["dy"].double() * R.pre_activation(p["x"], p["stats"], p["gamma"], p["beta"], sc, sh)[1]
            assert torch.equal(q / xhat_unit, torch.round(q / xhat_unit)) and (q.abs().sum(1) / xhat_unit).max().item() < 2.0**24
            assert torch.equal((A.f(n, A.RELU) + p["res"].double()).float().double(), A.f(n, A.RELU) + p["res"].double())
