"""Input builders shared by the attention tests (test_hip_ops.py, test_attention_backward.py)."""

import torch


def growing_scores_qkv(B, N, H, D, seed=5):
    """float32 q, k, v of shape (B, N, H, D) that exercise large logits: scores that keep GROWING along the key index for
    the queries that look along +u, queries of very different norms (0.1 .. 5 times N(0,1)), and one outlier key of norm 40
    that no query aligns with.  |q| |k| / sqrt(D) reaches ~200."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, N, H, D, generator=g) * torch.logspace(-1, 0.7, N).reshape(1, N, 1, 1)[:, torch.randperm(N, generator=g)]
    u = torch.nn.functional.normalize(torch.randn(B, 1, H, D, generator=g), dim=-1)
    ramp = torch.linspace(-6.0, 6.0, N).reshape(1, N, 1, 1)
    k = torch.randn(B, N, H, D, generator=g) * 0.3 + u * ramp          # scores grow with the key index for q along +u
    q = q + 2.0 * u * (torch.rand(B, N, H, 1, generator=g) > 0.5)       # half of the queries look along +u
    k[:, N // 3] = 40.0 * torch.nn.functional.normalize(torch.randn(B, H, D, generator=g), dim=-1)  # the outlier
    v = torch.randn(B, N, H, D, generator=g)
    return q, k, v
