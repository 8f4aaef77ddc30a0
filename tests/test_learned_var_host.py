"""Host side of the learned-variance path (no GPU): the signatures a captured sampler / training step is cached under
tell the learned-variance model from the fixed-variance one, the step tables are left as they were, and the formulas the
fused loss kernel implements (include/tdx.h, tdx_elbo_loss) -- value and analytic gradient, restated here in float64
numpy -- agree with torch autograd through `normal_kl` / `normal_log_lk` and through the kept torch formulation."""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _stand_in(**kw):
    base = dict(model=SimpleNamespace(compute_dtype=torch.float32, conv_impl=None), noise_bcs=True, clip_denoised=False,
                num_timesteps=10)
    base.update(kw)
    return SimpleNamespace(**base)


def test_sampler_signature_tells_learned_from_fixed_variances():
    """A learned-variance diffusion is cached under its own sampler (its captured step holds another update kernel); a
    stand-in without the attribute reads as fixed variances; the nine leading entries and the (None, 0.0) tail of the
    fixed-variance signature stay what tests/test_ddim_host.py pins, so the switch lives in the entry that names the update
    rule (None: ancestral, fixed variances; an int: DDIM over that many steps, which excludes learned variances)."""
    from turbdiff_amd.sampling import GraphSampler

    x = torch.zeros(2, 4, 6, 5, 4)
    bare = GraphSampler.signature_of(_stand_in(), x, None)
    fixed = GraphSampler.signature_of(_stand_in(learned_variances=False), x, None)
    learned = GraphSampler.signature_of(_stand_in(learned_variances=True), x, None)
    assert bare == fixed and bare[-2:] == (None, 0.0)
    assert learned != fixed and learned[:-2] == fixed[:-2] and learned[-2:] == ("learned-variances", 0.0)
    assert learned != GraphSampler.signature_of(_stand_in(), x, None, sampling_timesteps=4)


def test_training_step_signature_covers_the_elbo_switches():
    """What the captured training step bakes in of the learned-variance loss: which loss kernel (learned_variances and an
    ELBO weight) and its launch arguments elbo_weight, detach_mean, clip."""
    from turbdiff_amd.training import GraphedTrainingStep

    p = torch.nn.Parameter(torch.zeros(3))

    def sig(**kw):
        model = SimpleNamespace(model=SimpleNamespace(compute_dtype=torch.float32, conv_impl=None), loss_type="l2", noise_bcs=True,
                                **kw)
        task = SimpleNamespace(model=model, _opt=None, parameters=lambda: [p])
        return GraphedTrainingStep(task)._signature(torch.zeros(2, 4, 6, 5, 4), None)

    old = sig()  # a diffusion stand-in from before the switches existed
    base = sig(learned_variances=False, elbo_weight=None, detach_elbo_mean=True, clip_denoised=False)
    assert old == base and base[-4:] == (False, None, True, False)
    variants = [sig(learned_variances=True, elbo_weight=None, detach_elbo_mean=True, clip_denoised=False),
                sig(learned_variances=True, elbo_weight=0.1, detach_elbo_mean=True, clip_denoised=False),
                sig(learned_variances=True, elbo_weight=0.001, detach_elbo_mean=True, clip_denoised=False),
                sig(learned_variances=True, elbo_weight=0.1, detach_elbo_mean=False, clip_denoised=False),
                sig(learned_variances=True, elbo_weight=0.1, detach_elbo_mean=True, clip_denoised=True)]
    assert len({base, *variants}) == 6
    assert all(v[:-4] == base[:-4] for v in variants)


def test_step_tables_are_untouched_and_the_variance_table_is_a_buffer_of_its_own():
    """The learned-variance kernels take `posterior_log_var` as one more [T] pointer next to the packed [7, T] tables:
    PACKED_ORDER, and with it every fixed-variance launch, is what it was."""
    from turbdiff_amd import schedules
    from turbdiff_amd.models.ddpm import GaussianDiffusion

    assert schedules.PACKED_ORDER == ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                      "posterior_mean_coef2", "log_betas", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")
    d = GaussianDiffusion(torch.nn.Identity(), timesteps=10, beta_schedule="log-snr-linear", learned_variances=True)
    tabs = schedules.diffusion_tables("log-snr-linear", 10)
    assert tuple(d.step_tables.shape) == (7, 10) and torch.equal(d.step_tables, schedules.pack_step_tables(tabs))
    assert d.posterior_log_var.dtype == torch.float32 and d.posterior_log_var.is_contiguous()
    assert torch.equal(d.posterior_log_var, tabs["posterior_log_var"])
    # log_var is a lerp between the two tables: the posterior variance is the smaller one at every step
    assert bool((d.posterior_log_var <= d.log_betas).all())


# ---------------------------------------------------------------------------------------------------------------------
# the formulas of tdx_elbo_loss in float64 numpy


def elbo_np(out, noise, x_start, x_t, inside, t, tab, l1, clip, detach_mean, elbo_weight):
    """(loss[3], grad) of include/tdx.h, tdx_elbo_loss.  out (B, 2F, V); noise, x_start, x_t (B, F, V); inside bool [V];
    t int [B]; tab: name -> float64 [T]."""
    B, F, V = x_t.shape
    eps, w = out[:, :F], out[:, F:]
    col = lambda name: tab[name][t][:, None, None]
    recip, recipm1 = col("sqrt_recip_alphas_cumprod"), col("sqrt_recipm1_alphas_cumprod")
    c1, c2, lb, plv = col("posterior_mean_coef1"), col("posterior_mean_coef2"), col("log_betas"), col("posterior_log_var")
    first = (t == 0)[:, None, None]
    n = B * F * int(inside.sum())
    m = inside[None, None, :].astype(np.float64)
    d = eps - noise
    simple = ((np.abs(d) if l1 else d * d) * m).sum() / n
    g_eps = (np.sign(d) if l1 else 2.0 * d) * m / n
    s = 1.0 / (1.0 + np.exp(-w))
    log_var = lb + s * (plv - lb)
    raw = recip * x_t - recipm1 * eps
    x0 = np.clip(raw, -1.0, 1.0) if clip else raw
    passes = (raw >= -1.0) & (raw <= 1.0) if clip else np.ones_like(raw, dtype=bool)
    mean = c1 * x0 + c2 * x_t
    true_mean = c1 * x_start + c2 * x_t
    diff = np.where(first, x_t - mean, true_mean - mean)
    inv = np.exp(-log_var)
    a = np.where(first, 0.0, np.exp(plv - log_var))
    cst = np.where(first, math.log(2.0 * math.pi), -plv - 1.0)
    term = 0.5 * (log_var + cst + a + diff * diff * inv)
    elbo = (term * m).sum() / n
    d_log_var = 0.5 * (1.0 - a - diff * diff * inv)
    g_w = elbo_weight * d_log_var * (plv - lb) * s * (1.0 - s) * m / n
    if not detach_mean:
        # d term / d mean = -diff inv (both branches); d mean / d eps_hat = -c1 recipm1 where the clip let x0 through
        g_eps = g_eps + elbo_weight * (-diff * inv) * (-c1 * recipm1) * passes * m / n
    loss = np.array([simple + elbo_weight * elbo, simple, elbo])
    return loss, np.concatenate([g_eps, g_w], axis=1)


def _elbo_inputs(shape, seed, x_scale):
    B, F, V = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x_start, noise = x_scale * r(B, F, V), r(B, F, V)
    out = torch.cat([noise + 0.3 * r(B, F, V), r(B, F, V)], dim=1)
    inside = torch.rand(V, generator=g) < 0.6
    return out, noise, x_start, inside


@pytest.mark.parametrize("detach_mean", [True, False])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("l1", [False, True])
def test_elbo_formulas_agree_with_autograd(l1, clip, detach_mean):
    """The restatement above against torch autograd (float64, CPU) through (a) `normal_kl` / `normal_log_lk` applied to
    the quantities ddpm.py:853-870 hands them, written out here, and (b) the torch formulation the diffusion keeps
    (`_p_losses_elbo_torch`), per-sample means, cell_idx gathers and all.  Random inputs, t = [6, 0, 3]: both branches.
    Float64 on both sides: 1e-12 relative to the largest entry."""
    from turbdiff_amd import schedules
    from turbdiff_amd.models.ddpm import GaussianDiffusion, normal_kl, normal_log_lk

    B, F, V, T, ew = 3, 4, 35, 10, 0.1
    tab32 = schedules.diffusion_tables("log-snr-linear", T)
    tab = {k: v.double() for k, v in tab32.items()}
    t = torch.tensor([6, 0, 3])
    out, noise, x_start, inside = _elbo_inputs((B, F, V), seed=3, x_scale=1.2 if clip else 1.0)
    x_t = tab["sqrt_alphas_cumprod"][t][:, None, None] * x_start + tab["sqrt_one_minus_alphas_cumprod"][t][:, None, None] * noise
    loss, grad = elbo_np(out.numpy(), noise.numpy(), x_start.numpy(), x_t.numpy(), inside.numpy(), t.numpy(),
                         {k: v.numpy() for k, v in tab.items()}, l1, clip, detach_mean, ew)
    if clip:
        raw = tab["sqrt_recip_alphas_cumprod"][t][:, None, None] * x_t - tab["sqrt_recipm1_alphas_cumprod"][t][:, None, None] * out[:, :F]
        assert 0.2 < (raw.abs() > 1).double().mean().item() < 0.8

    # (a) the two helpers, on the reference's arguments
    o = out.clone().requires_grad_()
    eps, w = o.chunk(2, dim=1)
    col = lambda name: tab[name][t][:, None, None]
    log_var = torch.lerp(col("log_betas").expand_as(w), col("posterior_log_var").expand_as(w), torch.sigmoid(w))
    x0 = col("sqrt_recip_alphas_cumprod") * x_t - col("sqrt_recipm1_alphas_cumprod") * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = col("posterior_mean_coef1") * x0 + col("posterior_mean_coef2") * x_t
    if detach_mean:
        mean = mean.detach()
    true_mean = col("posterior_mean_coef1") * x_start + col("posterior_mean_coef2") * x_t
    kl = normal_kl(true_mean, col("posterior_log_var"), mean, log_var)[..., inside]
    ll = normal_log_lk(x_t, mean, log_var)[..., inside]
    elbo = torch.where(t == 0, -ll.flatten(1).mean(1), kl.flatten(1).mean(1)).mean()
    err = (eps - noise)[..., inside]
    simple = (err.abs() if l1 else err**2).flatten(1).mean(1).mean()
    total = simple + ew * elbo
    total.backward()
    want = np.array([total.item(), simple.item(), elbo.item()])
    assert np.abs(loss - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(grad - o.grad.numpy()).max() <= 1e-12 * np.abs(grad).max()
    assert np.abs(grad[..., ~inside.numpy()]).max() == 0.0 and np.abs(grad[:, F:]).max() > 0.0

    # (b) the kept torch formulation
    d = GaussianDiffusion(torch.nn.Identity(), timesteps=T, beta_schedule="log-snr-linear", loss_type="l1" if l1 else "l2",
                          noise_bcs=True, clip_denoised=clip, learned_variances=True, elbo_weight=ew,
                          detach_elbo_mean=detach_mean).double()
    o2 = out.clone().requires_grad_()
    cell_idx = inside.nonzero().flatten()
    five = lambda v: v.reshape(v.shape[0], v.shape[1], 5, 7, 1)
    got = d._p_losses_elbo_torch(five(o2), five(x_start), five(x_t), t, five(noise), inside.to(torch.uint8), cell_idx.numel(),
                                 cell_idx, parts=True)
    got[0].backward()
    assert np.abs(loss - np.array([v.item() for v in got])).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(grad - o2.grad.numpy()).max() <= 1e-12 * np.abs(grad).max()


def test_tools_expose_the_learned_variance_switches():
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    assert "--learned-variances" in (root / "tools" / "sample_bench.py").read_text()
    text = (root / "tools" / "step_bench.py").read_text()
    assert "--learned-variances" in text and "--elbo-weight" in text
