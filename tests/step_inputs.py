"""Seeded CPU inputs of the reverse-step and loss tests (tests/test_learned_var_gpu.py) and of the pinned-bits cases
(tests/reverse_step_cases.py, which the golden generator loads too): nothing here needs pytest or a GPU."""

import torch


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _mask_idx(V, seed=0):
    """two thirds of the cells, scattered: about a third of every quad is outside the domain"""
    g = torch.Generator().manual_seed(seed)
    return torch.sort(torch.randperm(V, generator=g)[: (2 * V) // 3]).values


def _tables(name, T):
    from turbdiff_amd import schedules

    tab = schedules.diffusion_tables(name, T)
    return tab, schedules.pack_step_tables(tab)


def _loss_inputs(shape, t, clip, tab):
    """x_start, noise ~ N(0, 1); eps_hat = noise + 0.3 N(0, 1); w ~ N(0, 1); x_t = q_sample in float32.  With the clip x_start
    is scaled by 1.2: at t = 0 / 1 (recipm1 < 0.1) x0 ~ x_start then leaves [-1, 1] for 40 % of the elements, at the noisy
    steps for 80-99 %, between 40 % and 70 % over a launch."""
    B, F = shape[:2]
    x_start, noise, e, w = (rnd(*shape, seed=s) for s in (11, 12, 13, 14))
    if clip:
        x_start = 1.2 * x_start
    eps_hat = noise + 0.3 * e
    out = torch.cat([eps_hat, w], dim=1).contiguous()
    col = lambda name: tab[name][t].view(B, 1, 1, 1, 1)
    x_t = col("sqrt_alphas_cumprod") * x_start + col("sqrt_one_minus_alphas_cumprod") * noise
    return out, noise, x_start, x_t
