"""Host side of the DDIM sampler, no GPU needed: the timestep subsequence (`schedules.ddim_timesteps`) and the packed
[6, S] coefficient table (`schedules.ddim_tables`).

The table is checked against what it must reduce to: at S = T, eta = 1 the generalized DDIM step IS the ancestral step
with the posterior variance, so its coefficients have to reproduce the DDPM posterior-mean coefficients and the
posterior variance (all evaluated here in float64 from the same betas; the bound 1e-11 absolute sits far above the
float64 rounding of these expressions -- at most 3.2e-13 measured, at T = 1000 where the cumulative product is longest --
and far below any coefficient mix-up)."""

import pytest
import torch

from turbdiff_amd import schedules as S

# linear at T = 10 has beta > 1 (the reference scales the range by 1000 / T): degenerate, not a schedule anybody samples
CASES = [(name, T) for name in ("log-linear", "log-snr-linear", "cosine", "sigmoid") for T in (10, 1000)] + [("linear", 1000)]
ROW = {name: i for i, name in enumerate(S.DDIM_PACKED_ORDER)}


@pytest.mark.parametrize("T", [10, 1000])
@pytest.mark.parametrize("steps", [1, 2, 3, 7, "T"])
def test_ddim_timesteps_span_the_chain(T, steps):
    n = T if steps == "T" else steps
    tau = S.ddim_timesteps(T, n)
    assert len(tau) == n and all(isinstance(t, int) for t in tau)
    assert tau[-1] == T - 1
    assert all(b > a for a, b in zip(tau, tau[1:]))
    if n > 1:
        assert tau[0] == 0
    if n == T:
        assert tau == list(range(T))


def test_ddim_timesteps_with_start_from_and_bad_arguments():
    assert S.ddim_timesteps(10, 3, start_from=6) == [0, 3, 5]
    assert S.ddim_timesteps(10, 1, start_from=6) == [5]
    assert S.ddim_timesteps(10, 6, start_from=6) == list(range(6))
    for T, steps, start in [(10, 0, None), (10, 11, None), (10, 7, 6), (10, -1, None), (10, 2, 11), (10, 1, 0)]:
        with pytest.raises(ValueError):
            S.ddim_timesteps(T, steps, start)


def _posterior_f64(name, T):
    betas = S.betas_for(name, T).to(torch.float64)
    abar = torch.cumprod(1.0 - betas, dim=0)
    prev = torch.nn.functional.pad(abar[:-1], (1, 0), value=1.0)
    coef1 = betas * torch.sqrt(prev) / (1.0 - abar)
    coef2 = (1.0 - prev) * torch.sqrt(1.0 - betas) / (1.0 - abar)
    var = betas * (1.0 - prev) / (1.0 - abar)
    return abar, coef1, coef2, var


@pytest.mark.parametrize("name,T", CASES)
def test_full_chain_at_eta_one_is_the_ddpm_posterior(name, T):
    tab = S.ddim_tables(name, T, range(T), 1.0, dtype=torch.float64)
    assert tab.shape == (6, T) and tab.dtype == torch.float64 and torch.isfinite(tab).all()
    abar, coef1, coef2, var = _posterior_f64(name, T)
    sa, sb = torch.sqrt(abar), torch.sqrt(1.0 - abar)
    # x_prev = sp x0 + dir (x_t - sqrt(a) x0) / sqrt(1 - a) + sigma z: the weights of x_t and of x0
    errs = ((tab[ROW["dir"]] / sb - coef2).abs().max().item(),
            (tab[ROW["sqrt_p"]] - tab[ROW["dir"]] * sa / sb - coef1).abs().max().item(),
            (tab[ROW["sigma"]][1:] ** 2 - var[1:]).abs().max().item())
    print(f"{name} T={T}: coef2 {errs[0]:.2e}, coef1 {errs[1]:.2e}, sigma^2 {errs[2]:.2e}")
    assert all(e <= 1e-11 for e in errs), errs
    # the two rows predict_start_from_noise shares with the ancestral step
    assert torch.equal(tab[ROW["sqrt_recip_a"]], torch.rsqrt(abar))
    assert torch.equal(tab[ROW["sqrt_recipm1_a"]], torch.sqrt(1.0 / abar - 1))


@pytest.mark.parametrize("name,T", CASES)
@pytest.mark.parametrize("steps", [1, 4, 7])
def test_eta_zero_is_deterministic_and_tables_are_finite(name, T, steps):
    tau = S.ddim_timesteps(T, steps)
    t0 = S.ddim_tables(name, T, tau, 0.0, dtype=torch.float64)
    assert torch.equal(t0[ROW["sigma"]], torch.zeros(steps, dtype=torch.float64))
    assert torch.equal(t0[ROW["dir"]], t0[ROW["sqrt_one_minus_p"]])
    assert t0[ROW["sqrt_p"]][0] == 1.0 and t0[ROW["dir"]][0] == 0.0  # step 0 lands on x0 itself
    for eta in (0.0, 0.5, 1.0):
        t64 = S.ddim_tables(name, T, tau, eta, dtype=torch.float64)
        assert t64.shape == (6, steps) and torch.isfinite(t64).all()
        t32 = S.ddim_tables(name, T, tau, eta)
        assert t32.dtype == torch.float32 and t32.is_contiguous()
        assert torch.equal(t32, t64.to(torch.float32))
        # sigma^2 + dir^2 = 1 - p: the noise added and the direction term share the variance of the level produced
        assert torch.allclose(t64[ROW["sigma"]] ** 2 + t64[ROW["dir"]] ** 2, t64[ROW["sqrt_one_minus_p"]] ** 2, rtol=0, atol=1e-15)


def test_ddim_tables_refuse_bad_arguments():
    for taus, eta in [([0, 5, 9], -0.1), ([0, 5, 9], 1.5), ([0, 5, 5], 0.0), ([3, 2], 0.0), ([0, 10], 0.0), ([-1, 3], 0.0), ([], 0.0)]:
        with pytest.raises(ValueError):
            S.ddim_tables("sigmoid", 10, taus, eta)


def test_sampler_signature_keeps_its_leading_entries():
    """The DDIM switches are APPENDED to the signature a captured sampler is cached under: a default call hashes to the
    ancestral sampler whatever else is cached."""
    from types import SimpleNamespace

    from turbdiff_amd.sampling import GraphSampler

    d = SimpleNamespace(model=SimpleNamespace(compute_dtype=torch.float32, conv_impl=None), noise_bcs=True, clip_denoised=False,
                        num_timesteps=10)
    x = torch.zeros(2, 4, 6, 5, 4)
    base = GraphSampler.signature_of(d, x, None)
    assert base[-2:] == (None, 0.0)
    assert base[:-2] == (tuple(x.shape), "cpu", None, torch.float32, None, base[5], True, False, 10)
    ddim = GraphSampler.signature_of(d, x, None, sampling_timesteps=4, eta=0.5)
    assert ddim[:-2] == base[:-2] and ddim[-2:] == (4, 0.5)
    assert ddim != GraphSampler.signature_of(d, x, None, sampling_timesteps=4, eta=0.0) != base


def test_trainer_and_tools_expose_the_switches():
    import inspect

    from turbdiff_amd.models.ddpm import GaussianDiffusion
    from turbdiff_amd.training import DiffusionTrainer

    for fn in (GaussianDiffusion.p_sample_loop,):
        p = inspect.signature(fn).parameters
        assert p["sampling_timesteps"].default is None and p["eta"].default == 0.0
    for fn in (DiffusionTrainer.sample, DiffusionTrainer.sample_cells):
        p = inspect.signature(fn).parameters
        assert p["sampling_timesteps"].default is None and p["eta"].default is None
