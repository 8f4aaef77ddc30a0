"""Exact Wasserstein-2 for the sample metrics: the batched HIP auction (``tdx_ot_auction``, csrc/tdx_ot.hip), the fused
per-cell features of ``WassersteinMetric`` (``tdx_ot_features``, csrc/tdx_fd.hip), and the exact host solver of the
small outer problems.

With uniform weights on both sides, ``ot.emd2([], [], M)`` of the reference is a transport problem whose optimum is
reached at a vertex of the transport polytope: for an n x n matrix a permutation (Birkhoff), for n x m a permutation
of the lcm(n, m) x lcm(n, m) matrix that repeats every row lcm/n and every column lcm/m times.  ``exact_emd2`` solves
that assignment with ``scipy.optimize.linear_sum_assignment``; the device solver targets the same exact optimum, up
to a documented eps_final (``auction_w2``), and certifies it with a dual bound.  (POT's ``emd2`` stops after
``numItermax=100000`` network-simplex iterations by default, which can end before the optimum on problems of 10^4
points; neither solver here has such a limit below the optimum.)
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

STATUS = {0: "ok", 1: "round cap of a phase reached", 2: "bid cap of the job reached", 3: "bad job", 4: "non-finite features"}
DEFAULT_REL_EPS = 1e-7        # eps_final = DEFAULT_REL_EPS * S, S the job's cost scale (see auction_w2)
DEFAULT_MAX_ROUNDS = 1 << 22  # bidding rounds per eps phase
DEFAULT_MAX_BIDS = 1 << 40    # bids per job
DEFAULT_SLOTS = 512           # workgroups of the persistent grid (two per CU)


def exact_emd2(M) -> float:
    """``ot.emd2([], [], M)`` exactly: the optimal transport cost between uniform weights on the rows and on the
    columns of the cost matrix ``M`` (n x m), by linear assignment on the lcm(n, m) expansion."""
    from scipy.optimize import linear_sum_assignment

    M = np.asarray(M, dtype=np.float64)
    if M.ndim != 2 or M.size == 0:
        raise ValueError(f"expected a non-empty 2-D cost matrix, got shape {M.shape}")
    big = lcm_expand(M)
    r, c = linear_sum_assignment(big)
    return float(big[r, c].sum() / big.shape[0])


def lcm_expand(M: np.ndarray) -> np.ndarray:
    """The lcm(n, m)-square matrix with every row of ``M`` repeated lcm/n times and every column lcm/m times."""
    n, m = M.shape
    k = n * m // math.gcd(n, m)
    return np.repeat(np.repeat(M, k // n, axis=0), k // m, axis=1)


@dataclass
class AuctionResult:
    """Per job (numpy, in the order of the job list): primal mean cost (= W2^2 up to eps_final), dual bound, eps_final,
    number of bids and status (0 = ok)."""

    primal: np.ndarray
    dual: np.ndarray
    eps_final: np.ndarray
    bids: np.ndarray
    status: np.ndarray

    @property
    def gap(self) -> np.ndarray:
        return self.primal - self.dual


def _device_ints(x, device) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(device=device, dtype=torch.int32).contiguous()


def auction_w2(fa: torch.Tensor, fb: torch.Tensor, idx, offsets, jobs, *, rel_eps: float = DEFAULT_REL_EPS,
               max_rounds: int = DEFAULT_MAX_ROUNDS, max_bids: int = DEFAULT_MAX_BIDS, slots: int = DEFAULT_SLOTS,
               check: bool = True) -> AuctionResult:
    """Exact W2^2 of every job (i, j, k) in one launch: region k (cells ``idx[offsets[k]:offsets[k+1]]``) of
    ``fa[i]`` against the same cells of ``fb[j]``, cost ||fa[i, p] - fb[j, q]||^2 with uniform weights.

    ``fa`` (Sa, n_cells, 8), ``fb`` (Sb, n_cells, 8): fp32 device tensors.  Each job stops at eps_final =
    ``rel_eps`` * S, S = (1/n) sum over both point sets of |x - their pooled mean|^2 (any coupling of the sets costs at
    most 2 S on average); its primal then lies within eps_final above the exact optimum, and the device-computed dual
    bound within eps_final below the primal.  Every loop of the kernel is capped (``max_rounds`` rounds per eps phase,
    ``max_bids`` bids per job); a job that reaches a cap comes back with its status set, and with ``check`` a
    non-zero status raises."""
    if fa.dtype != torch.float32 or fb.dtype != torch.float32 or fa.ndim != 3 or fb.ndim != 3 or fa.shape[1:] != fb.shape[1:] \
            or fa.shape[2] != 8:
        raise RuntimeError(f"expected fp32 (S, n_cells, 8) features, got {tuple(fa.shape)} {fa.dtype} / {tuple(fb.shape)} {fb.dtype}")
    dev = fa.device
    L.ptr(fa), L.ptr(fb)  # device + contiguity checks before anything else
    if fa.data_ptr() % 16 or fb.data_ptr() % 16:
        raise RuntimeError("auction_w2: features must be 16-byte aligned")
    if not (torch.isfinite(fa).all() and torch.isfinite(fb).all()):
        raise RuntimeError("auction_w2: non-finite features")
    n_cells = fa.shape[1]
    idx_h = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(-1)
    off_h = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
    jobs_h = np.asarray(jobs.cpu() if isinstance(jobs, torch.Tensor) else jobs, dtype=np.int64).reshape(-1, 3)
    K, J = len(off_h) - 1, len(jobs_h)
    if K < 1 or off_h[0] != 0 or np.any(np.diff(off_h) < 0) or off_h[-1] != len(idx_h):
        raise RuntimeError("offsets must rise from 0 to len(idx)")
    if len(idx_h) and (idx_h.min() < 0 or idx_h.max() >= n_cells):
        raise RuntimeError("region cell index out of range")
    if J == 0:
        z = np.zeros(0)
        return AuctionResult(z, z, z, z, np.zeros(0, dtype=np.int32))
    if (jobs_h[:, 0].min() < 0 or jobs_h[:, 0].max() >= fa.shape[0] or jobs_h[:, 1].min() < 0
            or jobs_h[:, 1].max() >= fb.shape[0] or jobs_h[:, 2].min() < 0 or jobs_h[:, 2].max() >= K):
        raise RuntimeError("job index out of range")
    sizes = np.diff(off_h)
    max_n = max(int(sizes[jobs_h[:, 2]].max()), 1)
    # largest regions first: the persistent grid's workgroups then finish close together
    order = np.argsort(-sizes[jobs_h[:, 2]], kind="stable")
    slots = max(1, min(int(slots), J))
    ws = torch.empty(L.load().tdx_ot_workspace_bytes(max_n, slots), dtype=torch.uint8, device=dev)
    out = torch.empty((J, 4), dtype=torch.float64, device=dev)
    status = torch.empty(J, dtype=torch.int32, device=dev)
    idx_d, off_d, jobs_d = _device_ints(idx_h, dev), _device_ints(off_h, dev), _device_ints(jobs_h[order], dev)
    L.call("tdx_ot_auction", L.ptr(fa), L.ptr(fb), n_cells, L.ptr(idx_d), L.ptr(off_d), K, L.ptr(jobs_d), J, fa.shape[0],
           fb.shape[0], float(rel_eps), int(max_rounds), int(max_bids), L.ptr(ws), max_n, slots, L.ptr(out), L.ptr(status),
           L.stream())
    o = np.empty((J, 4))
    st = np.empty(J, dtype=np.int32)
    o[order] = out.cpu().numpy()
    st[order] = status.cpu().numpy()
    res = AuctionResult(o[:, 0], o[:, 1], o[:, 2], o[:, 3].astype(np.int64), st)
    if check and st.any():
        bad = np.flatnonzero(st)
        raise RuntimeError(f"auction_w2: {len(bad)} of {J} jobs failed, first job {tuple(jobs_h[bad[0]])}: "
                           f"{STATUS.get(int(st[bad[0]]), int(st[bad[0]]))}")
    return res


def features(u_grid: torch.Tensor, u_cells: torch.Tensor, p_cells: torch.Tensor, unpadded_idx: torch.Tensor,
             scale: torch.Tensor, h) -> torch.Tensor:
    """``WassersteinMetric.features`` in one kernel: (S, n_cells, 8) fp32 = [u, curl u, p] / scale at the in-domain
    cells, lane 7 zero.  ``u_grid`` (S, 3, X, Y, Z) the padded velocity grid, ``u_cells`` (S, n_cells, 3), ``p_cells``
    (S, n_cells, 1), ``unpadded_idx`` (n_cells,) flat indices into (X-2, Y-2, Z-2), ``scale`` (7,) the std of
    ``u:norm-std;curl:norm-std;p:mean-std``."""
    from .metrics import spacing

    S, _, X, Y, Z = u_grid.shape
    n = u_cells.shape[1]
    if u_cells.shape != (S, n, 3) or p_cells.shape != (S, n, 1) or unpadded_idx.shape != (n,) or scale.numel() != 7:
        raise RuntimeError(f"feature shapes disagree: {tuple(u_grid.shape)} {tuple(u_cells.shape)} {tuple(p_cells.shape)} "
                           f"{tuple(unpadded_idx.shape)} {tuple(scale.shape)}")
    uidx = unpadded_idx.to(torch.int64).contiguous()
    if n and (int(uidx.min()) < 0 or int(uidx.max()) >= (X - 2) * (Y - 2) * (Z - 2)):
        raise RuntimeError("unpadded cell index out of range")
    hx, hy, hz = spacing(h)
    out = torch.empty((S, n, 8), dtype=torch.float32, device=u_grid.device)
    # named, so the converted copies outlive the launch
    ug, uc, pc, sc = (t.to(torch.float32).contiguous() for t in (u_grid, u_cells, p_cells, scale.reshape(-1)))
    L.call("tdx_ot_features", L.ptr(ug), L.ptr(uc), L.ptr(pc), L.ptr(uidx), L.ptr(sc), L.ptr(out), S, n, X, Y, Z, 2 * hx,
           2 * hy, 2 * hz, L.stream())
    return out
