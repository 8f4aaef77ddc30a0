"""Finite-difference flow quantities with the reference's names and semantics (turbdiff/metrics.py:9-92).

``centered_difference_derivative``, ``unpadded_derivative`` and ``vector_gradient`` are plain tensor code (they run on
whatever device their input lives on); ``curl``, ``divergence`` and ``enstrophy`` are one HIP kernel each mode
(``tdx_fd``, csrc/tdx_fd.hip) on a padded ``(..., 3, X, Y, Z)`` fp32 velocity grid, evaluated at the unpadded interior
``(..., C, X-2, Y-2, Z-2)`` with per-axis spacing ``h``.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

FD_CURL, FD_DIVERGENCE, FD_ENSTROPHY = 0, 1, 2  # TDX_FD_* (include/tdx.h)


def centered_difference_derivative(x: torch.Tensor, *, dim: int, h: float):
    """First derivative of ``x`` along ``dim`` by centred differences; 2 shorter along ``dim``."""
    n = x.shape[dim]
    return (x.narrow(dim, 2, n - 2) - x.narrow(dim, 0, n - 2)) / (2 * h)


def unpadded_derivative(x: torch.Tensor, h, *, dim: int):
    """Derivative of ``x`` along ``dim`` (< 0) with the padding layer cut off in the other directions."""
    assert dim < 0
    for i in range(-3, 0, 1):
        if i != dim:
            x = x.narrow(i, 1, x.shape[i] - 2)
    return centered_difference_derivative(x, dim=dim, h=h[dim])


def vector_gradient(u: torch.Tensor, h):
    """Gradient of the vector field ``u`` (..., n, X, Y, Z) -> (..., n, 3, X-2, Y-2, Z-2)."""

    def narrow(x: torch.Tensor, j: int):
        for i in range(3):
            if i != j:
                x = x.narrow(i - 3, 1, x.shape[i - 3] - 2)
        return x

    rows = [torch.stack([narrow(centered_difference_derivative(u.select(dim=-4, index=i), dim=j - 3, h=h[j]), j)
                         for j in range(3)], dim=-4) for i in range(u.shape[-4])]
    return torch.stack(rows, dim=-5)


def spacing(h) -> tuple[float, float, float]:
    """``h`` as three Python floats (a tuple, numpy array or tensor; ``None`` = unit spacing)."""
    if h is None:
        return (1.0, 1.0, 1.0)
    if isinstance(h, torch.Tensor):
        h = h.detach().cpu().double().numpy()
    h = tuple(float(v) for v in np.asarray(h, dtype=np.float64).reshape(-1))
    if len(h) != 3:
        raise ValueError(f"expected three grid spacings, got {h}")
    return h


def _fd(u: torch.Tensor, h, mode: int) -> torch.Tensor:
    if u.ndim < 4 or u.shape[-4] != 3 or u.dtype != torch.float32:
        raise RuntimeError(f"expected fp32 (..., 3, X, Y, Z), got {u.dtype} {tuple(u.shape)}")
    lead, (X, Y, Z) = u.shape[:-4], u.shape[-3:]
    if min(X, Y, Z) < 3:
        raise RuntimeError(f"a padded grid needs at least 3 cells per axis, got {(X, Y, Z)}")
    hx, hy, hz = spacing(h)
    uc = u.reshape(-1, 3, X, Y, Z).contiguous()
    C = 3 if mode == FD_CURL else 1
    out = torch.empty((uc.shape[0], C, X - 2, Y - 2, Z - 2), dtype=torch.float32, device=u.device)
    dv = float(np.prod([hx, hy, hz]))
    L.call("tdx_fd", L.ptr(uc), L.ptr(out), uc.shape[0], X, Y, Z, 2 * hx, 2 * hy, 2 * hz, dv, mode, L.stream())
    return out.reshape(*lead, C, X - 2, Y - 2, Z - 2)


def divergence(u: torch.Tensor, h):
    """Divergence at the inner cells of the padded velocity field ``u``: (..., 1, X-2, Y-2, Z-2)."""
    return _fd(u, h, FD_DIVERGENCE)


def curl(u: torch.Tensor, h):
    """Curl at the inner cells of the padded velocity field ``u``: (..., 3, X-2, Y-2, Z-2)."""
    return _fd(u, h, FD_CURL)


def enstrophy(u: torch.Tensor, h):
    """Squared vorticity integrated over each inner cell, |curl u|^2 prod(h): (..., 1, X-2, Y-2, Z-2)."""
    return _fd(u, h, FD_ENSTROPHY)
