"""Host side of the two samplers a learned-variance model takes over S of T steps, no GPU needed: the packed [8, S] table of
the respaced chain (`schedules.respaced_tables`), the one function that decides which update a call gets
(`sampling.check_sampling_arguments`), the sampler signatures, and the keyword on the public entry points and the tools."""

import inspect
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from respaced_reference import CASES, U, training_chain_f64
from turbdiff_amd import schedules as S

ROW = {name: i for i, name in enumerate(S.RESPACED_PACKED_ORDER)}
ROOT = Path(__file__).resolve().parent.parent


def test_packed_order():
    assert S.RESPACED_PACKED_ORDER == ("sqrt_recip_a", "sqrt_recipm1_a", "coef1", "coef2", "log_beta", "posterior_log_var",
                                       "sqrt_p", "sqrt_one_minus_p")


@pytest.mark.parametrize("name,T", CASES)
def test_full_chain_is_the_training_chain(name, T):
    """taus = range(T): the respaced chain IS the training chain, so its float64 table has to reproduce the training chain's
    float64 quantities up to the rounding of beta' = 1 - abar_t / abar_{t-1}.

    Propagation, u = 2^-53.  abar_t = fl(abar_{t-1} alpha_t), so a / p = alpha_t (1 + e) with |e| <= 2u after the division,
    and beta' = fl(1 - a / p) is within 2u alpha_t + u beta' <= 3u of beta_t: bound 4u absolute (measured: at most 1.5u over
    all five schedules at T = 10 / 500 / 1000).  The same delta carried to first order through each row, divided by what the
    row's formula divides by:
        log_beta   d log(beta) = delta / beta                      bound 4u / beta
        coef1      beta sqrt(p) / (1 - a), sqrt(p) <= 1            bound 4u / (1 - a)
        coef2      (1 - p) sqrt(a / p) / (1 - a) against (1 - p) sqrt(1 - beta) / (1 - a): d sqrt(alpha) = delta / (2 sqrt(alpha)),
                   times (1 - p) <= 1                               bound 4u / (1 - a)
    (the own roundings of the rows, a few u relative on numbers <= 1, sit inside the slack between 1.5u and 4u wherever
    beta, 1 - a < 1, which is everywhere).  The rows that do not involve beta' are the training chain's bit for bit."""
    tab = S.respaced_tables(name, T, range(T), dtype=torch.float64)
    assert tab.shape == (8, T) and tab.dtype == torch.float64 and torch.isfinite(tab).all()
    betas, abar, prev, coef1, coef2 = training_chain_f64(name, T)
    d_beta = (torch.exp(tab[ROW["log_beta"]]) - betas).abs()  # informative only: goes through exp
    beta_r = 1.0 - abar / prev
    errs = {
        "beta": ((beta_r - betas).abs() / (4 * U)).max().item(),
        "log_beta": ((tab[ROW["log_beta"]] - torch.log(betas)).abs() * betas / (4 * U)).max().item(),
        "coef1": ((tab[ROW["coef1"]] - coef1).abs() * (1.0 - abar) / (4 * U)).max().item(),
        "coef2": ((tab[ROW["coef2"]] - coef2).abs() * (1.0 - abar) / (4 * U)).max().item(),
    }
    print(f"{name} T={T}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in errs.items()) + f" (exp(lb) - beta {d_beta.max().item():.1e})")
    assert all(v <= 1.0 for v in errs.values()), errs
    assert torch.equal(tab[ROW["sqrt_recip_a"]], torch.rsqrt(abar))
    assert torch.equal(tab[ROW["sqrt_recipm1_a"]], torch.sqrt(1.0 / abar - 1))
    assert torch.equal(tab[ROW["sqrt_p"]], torch.sqrt(prev))
    assert torch.equal(tab[ROW["sqrt_one_minus_p"]], torch.sqrt(1.0 - prev))
    # the posterior variance of the training chain for t >= 1 (its column 0 is an extrapolation no step reads)
    plv = torch.log(betas * (1.0 - prev) / (1.0 - abar))
    assert ((tab[ROW["posterior_log_var"]][1:] - plv[1:]).abs() * betas[1:] <= 4 * U).all()


@pytest.mark.parametrize("name,T", CASES)
@pytest.mark.parametrize("steps,start_from", [(1, None), (4, None), (7, None), (1, 6), (4, 6), (7, 9)])
def test_subsequence_tables(name, T, steps, start_from):
    """What the kernel test's bound presumes of the table (entries and sigma <= 1), and two float64 identities per column:
    c1 + c2 sqrt(a) = sqrt(p) -- the posterior mean of a noise-free point x_t = sqrt(a) x0 is sqrt(p) x0 -- to
    4u / (1 - a) (four roundings of O(1) numbers over 1 - a), and prod_k (1 - beta'_k) = a with beta'_k = exp(log_beta[k])
    read back from the table.  For the product: beta' = fl(1 - fl(a / p)) is rounded once (u / 2 relative), its logarithm
    once (u |lb| / 2 relative to beta' after the exp), the exp once more (u at most): beta'_tab = beta' (1 + e), |e| <=
    u (|lb| / 2 + 2).  Seen from 1 - beta' = a / p that is e beta' / (1 - beta') <= e p / a relative; the division, the
    subtraction and the running product add 2u per factor.  Relative bound: u sum_k ((|lb_k| / 2 + 2) p_k / a_k + 2)."""
    tau = S.ddim_timesteps(T, steps, start_from)
    t64 = S.respaced_tables(name, T, tau, dtype=torch.float64)
    t32 = S.respaced_tables(name, T, tau)
    assert t64.shape == (8, steps) and torch.isfinite(t64).all()
    assert t32.dtype == torch.float32 and t32.is_contiguous() and torch.equal(t32, t64.to(torch.float32))
    assert torch.isfinite(t32).all()
    lb, plv = t64[ROW["log_beta"]], t64[ROW["posterior_log_var"]]
    assert plv[0] == lb[0] and (plv <= lb).all()
    for tab in (t64, t32):
        for row in ("coef1", "coef2", "sqrt_p", "sqrt_one_minus_p"):
            assert (tab[ROW[row]] >= 0).all() and (tab[ROW[row]] <= 1).all(), row
        sig = torch.exp(tab[ROW["log_beta"]] / 2)
        assert (sig >= 0).all() and (sig <= 1).all()
        assert tab[ROW["coef1"]][0] == 1.0 and tab[ROW["coef2"]][0] == 0.0
        assert (tab[ROW["posterior_log_var"]] <= tab[ROW["log_beta"]]).all()
    abar = training_chain_f64(name, T)[1]
    a = abar[torch.tensor(tau)]
    p = torch.nn.functional.pad(a[:-1], (1, 0), value=1.0)
    ident = (t64[ROW["coef1"]] + t64[ROW["coef2"]] * torch.sqrt(a) - torch.sqrt(p)).abs() * (1.0 - a) / (4 * U)
    prod = torch.cumprod(1.0 - torch.exp(lb), dim=0)
    rel = ((prod - a).abs() / a) / (U * torch.cumsum((lb.abs() / 2 + 2) * p / a + 2, dim=0))
    print(f"{name} T={T} S={steps} start_from={start_from}: identity {ident.max().item():.3f} of its bound, product {rel.max().item():.3f}")
    assert ident.max().item() <= 1.0
    assert rel.max().item() <= 1.0


def test_respaced_tables_refuse_bad_arguments():
    for taus in ([0, 5, 5], [3, 2], [0, 10], [-1, 3], []):
        with pytest.raises(ValueError):
            S.respaced_tables("sigmoid", 10, taus)


# ---------------------------------------------------------------------------------------------------------------------
def _d(learned, T=10):
    return SimpleNamespace(learned_variances=learned, num_timesteps=T)


def test_resolution_table_row_by_row():
    from turbdiff_amd.sampling import check_ddim_arguments, check_sampling_arguments as check

    for learned in (False, True):
        assert check(_d(learned), None, 0.0) is None                                      # today's ancestral loop
        assert check(_d(learned), None, 0.0, None, None) is None
        for m in ("ddim", "respaced"):
            with pytest.raises(ValueError, match="sampling_timesteps"):                  # a method needs a step count
                check(_d(learned), None, 0.0, None, m)
        for m in ("euler", "", "DDIM"):
            with pytest.raises(ValueError, match="sampling_method"):
                check(_d(learned), 4, 0.0, None, m)
    assert check(SimpleNamespace(num_timesteps=10), 4, 0.0) == "ddim"                     # no attribute: fixed variances
    assert check(_d(False), 4, 0.5) == check(_d(False), 4, 0.5, None, "ddim") == "ddim"   # today's DDIM
    with pytest.raises(ValueError, match="respaced"):
        check(_d(False), 4, 0.0, None, "respaced")
    with pytest.raises(ValueError, match="learned_variances") as e:                      # learned, S, no method: as before
        check(_d(True), 4, 0.0)
    assert "sampling_method" in str(e.value) and '"respaced"' in str(e.value) and '"ddim"' in str(e.value)
    assert check(_d(True), 4, 0.0, None, "respaced") == "lv-respaced"
    for eta in (0.5, 1.0, -0.1):
        with pytest.raises(ValueError, match="eta"):
            check(_d(True), 4, eta, None, "respaced")
    for eta in (0.0, 0.5, 1.0):
        assert check(_d(True), 4, eta, None, "ddim") == "lv-ddim"
    for eta in (-0.1, 1.01):
        with pytest.raises(ValueError, match="eta"):
            check(_d(True), 4, eta, None, "ddim")
        with pytest.raises(ValueError, match="eta"):
            check(_d(False), 4, eta, None, "ddim")
    # S and start_from go through schedules.ddim_timesteps, for every method
    for learned, m in ((False, None), (False, "ddim"), (True, "respaced"), (True, "ddim")):
        for steps, start in ((0, None), (11, None), (7, 6), (2, 11)):
            with pytest.raises(ValueError):
                check(_d(learned), steps, 0.0, start, m)
        assert check(_d(learned), 6, 0.0, 6, m) is not None
    # the old check keeps its behaviour
    check_ddim_arguments(_d(False), 4, 0.5)
    with pytest.raises(ValueError, match="learned_variances"):
        check_ddim_arguments(_d(True), 4, 0.0)


def _stand_in(**kw):
    return SimpleNamespace(model=SimpleNamespace(compute_dtype=torch.float32, conv_impl=None), noise_bcs=True, clip_denoised=False,
                           num_timesteps=10, **kw)


def test_signatures_of_existing_calls_are_unchanged_and_the_new_ones_are_distinct():
    from turbdiff_amd import _lib as L
    from turbdiff_amd.sampling import GraphSampler

    x = torch.zeros(2, 4, 6, 5, 4)
    lead = ((2, 4, 6, 5, 4), "cpu", None, torch.float32, None, L.conv_impl(), True, False, 10)
    sig = GraphSampler.signature_of
    fixed, learned = _stand_in(), _stand_in(learned_variances=True)
    existing = {
        "ancestral": (sig(fixed, x, None), lead + (None, 0.0)),
        "ancestral, attribute off": (sig(_stand_in(learned_variances=False), x, None), lead + (None, 0.0)),
        "learned variances": (sig(learned, x, None), lead + ("learned-variances", 0.0)),
        "ddim 4, 0.5": (sig(fixed, x, None, sampling_timesteps=4, eta=0.5), lead + (4, 0.5)),
        "ddim 4, 0": (sig(fixed, x, None, 4, 0.0), lead + (4, 0.0)),
        "ddim 7, 1": (sig(fixed, x, None, 7, 1.0), lead + (7, 1.0)),
    }
    for what, (got, want) in existing.items():
        assert got == want and len(got) == 11, what
    # a fixed-variance model under the explicit "ddim" is the sampler it always had
    assert sig(fixed, x, None, 4, 0.5, "ddim") == lead + (4, 0.5)
    resp4, resp7 = sig(learned, x, None, 4, 0.0, "respaced"), sig(learned, x, None, 7, 0.0, "respaced")
    ddim4, ddim7 = sig(learned, x, None, 4, 0.0, "ddim"), sig(learned, x, None, 7, 0.0, "ddim")
    assert resp4 == lead + (("learned-variances", "respaced", 4), 0.0)
    assert ddim4 == lead + (("learned-variances", "ddim", 4), 0.0)
    new = [resp4, resp7, ddim4, ddim7, sig(learned, x, None, 4, 1.0, "ddim")]
    every = new + [got for got, _ in existing.values()]
    assert all(a != b for i, a in enumerate(new) for b in every[i + 1:])
    assert all(s[:-2] == lead for s in new)
    assert inspect.signature(sig).parameters["sampling_method"].default is None
    assert list(inspect.signature(sig).parameters)[-2:] == ["eta", "sampling_method"]


def test_public_entry_points_carry_the_keyword():
    from turbdiff_amd.models.ddpm import GaussianDiffusion
    from turbdiff_amd.sampling import GraphSampler
    from turbdiff_amd.training import DiffusionTrainer

    for fn in (GaussianDiffusion.p_sample_loop, GraphSampler.__init__, DiffusionTrainer.sample, DiffusionTrainer.sample_cells,
               DiffusionTrainer._sample_normalized):
        names = list(inspect.signature(fn).parameters)
        assert names[names.index("eta") + 1] == "sampling_method", fn
        assert inspect.signature(fn).parameters["sampling_method"].default is None, fn
    task = DiffusionTrainer(**{**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}, u_net_levels=2, max_train_steps=20)
    assert task.sampling_method is None and task.sampling_timesteps is None and task.sampling_eta == 0.0


@pytest.mark.parametrize("tool", ["eval_ckpt.py", "sample_bench.py"])
def test_tools_accept_the_flag(tool):
    out = subprocess.run([sys.executable, str(ROOT / "tools" / tool), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "--sampling-method {ddim,respaced}" in out.stdout


def test_header_names_the_four_entries():
    from turbdiff_amd import _lib as L

    header = (ROOT / "include" / "tdx.h").read_text()
    for name in ("tdx_p_sample_step_lv_respaced", "tdx_p_sample_step_lv_respaced_rng", "tdx_ddim_step_lv", "tdx_ddim_step_lv_rng"):
        assert f"int {name}(" in header and name in L.SIGNATURES
