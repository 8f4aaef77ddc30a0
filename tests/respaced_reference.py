"""Float64 restatements for the respaced learned-variance sampler (tests/test_respaced_host.py, tests/test_respaced_gpu.py):
the reference implementation has no respacing, so the yardstick is the formula of DESIGN.md §4a‴ written out
in float64, plus the existing kernels.  Nothing here needs pytest or a GPU."""

import torch

# (schedule, T): the pairs of tests/test_ddim_host.py's CASES.  linear at T = 10 has beta > 1, not a schedule anybody samples
CASES = [(name, T) for name in ("log-linear", "log-snr-linear", "cosine", "sigmoid") for T in (10, 1000)] + [("linear", 1000)]

U = 2.0**-53


def training_chain_f64(name, T):
    """The training chain's own quantities in float64 from `betas_for`: betas, abar, abar_prev, coef1, coef2."""
    from turbdiff_amd import schedules as S

    betas = S.betas_for(name, T).to(torch.float64)
    abar = torch.cumprod(1.0 - betas, dim=0)
    prev = torch.nn.functional.pad(abar[:-1], (1, 0), value=1.0)
    coef1 = betas * torch.sqrt(prev) / (1.0 - abar)
    coef2 = (1.0 - prev) * torch.sqrt(1.0 - betas) / (1.0 - abar)
    return betas, abar, prev, coef1, coef2


def respaced_step_f64(tab, k, x_t, out, z, z2, x_bcs, inside, noise_bcs, clip):
    """One respaced learned-variance step in float64, reading column k of the float32 [8, S] table (rows:
    schedules.RESPACED_PACKED_ORDER).  out = [eps_hat | w]; inside: bool, broadcastable to x_t."""
    F = x_t.shape[1]
    recip, recipm1, c1, c2, lb, plv, sa, sb = (float(v) for v in tab[:, k].double())
    x_t, out, z, z2, x_bcs = (v.double() for v in (x_t, out, z, z2, x_bcs))
    eps, w = out[:, :F], out[:, F:]
    x0 = recip * x_t - recipm1 * eps
    if not noise_bcs:
        x0 = torch.where(inside, x0, x_t)
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = c1 * x0 + c2 * x_t
    if k == 0:
        return torch.where(inside, mean, x_bcs)
    log_var = lb + torch.sigmoid(w) * (plv - lb)
    r = mean + (log_var / 2).exp() * z
    outside = sa * x_bcs + sb * z2 if noise_bcs else mean
    return torch.where(inside, r, outside)
