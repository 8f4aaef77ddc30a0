"""Case preparation: the side files that training and the sample metrics read, made from the raw ``data.h5`` case files.

    <root>/stats.pickle          ``dataset_stats`` / ``write_stats``   (reference scripts/dataset-stats.py)
    <case>/mean-flow.h5          ``mean_flow``                         (scripts/mean-flow.py)
    <case>/regions.npz           ``homogeneous_regions``               (scripts/homogeneous-regions.py)
    <case>/max-mean-tke.npy      ``max_mean_tke``                      (scripts/max-mean-tke.py)

The reductions run in HIP kernels (csrc/tdx_prepare.hip): ``tdx_moments_update`` streams the temporal mean and variance
of a field chunk by chunk, ``tdx_field_stats`` reduces min / max / sum / sum of squares, ``tdx_w2n_assign`` +
``tdx_w2n_reduce`` are one Lloyd pass of the k-means under the 2-Wasserstein distance between diagonal normals.  The host
keeps what is small or sequential: the chunk plan, the k-means++ draws (``np.random.default_rng`` in the reference's order
of calls), the k x k convergence test, the splitting of large clusters.  Frames are read ``chunk_frames`` at a time, so a
case of any length is processed in bounded memory.  There is no CPU path: tensors handed to the kernels must be on the
device.

Case files are opened through the ``opener`` that ``OpenFOAMDataRepository`` takes (default: ``h5py.File``).

One deliberate difference from the reference: a cluster without cells is an error.  After a Lloyd iteration a
``RuntimeError`` names it, where scripts/homogeneous-regions.py would carry the NaN mean of an empty selection forward; the
same holds for the final assignment (before anything is written), where the script would write labels with one of them
missing and a NaN mean distance.
"""

from __future__ import annotations

import math
import pickle
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from .. import _lib as L
from .ofles import OpenFOAMData, OpenFOAMDataRepository, _open_h5, find_data_files
from .ofles import Variable as V

STATS_FIELDS = ("p", "u", "norm(u)", "norm(curl)", "k", "nut")
W2N_MAX_K = 512  # W2_MAX_K of csrc/tdx_prepare.hip


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


# ------------------------------------------------------------------------------------------------ kernels
def moments_update(x: torch.Tensor, mean: torch.Tensor, m2: torch.Tensor, count: int) -> int:
    """Merge the frames ``x`` (T, n) fp32 into the running temporal ``mean`` (n) and centred sum of squares ``m2`` (n),
    both fp64, which hold ``count`` frames (0: their contents are not read).  Returns the new count."""
    if x.dtype != torch.float32 or x.ndim != 2 or mean.dtype != torch.float64 or m2.dtype != torch.float64 \
            or mean.shape != (x.shape[1],) or m2.shape != mean.shape:
        raise RuntimeError(f"moments_update: expected fp32 (T, n) and fp64 (n) state, got {x.dtype} {tuple(x.shape)}, "
                           f"{mean.dtype} {tuple(mean.shape)}, {m2.dtype} {tuple(m2.shape)}")
    T, n = x.shape
    L.call("tdx_moments_update", L.ptr(x), T, n, L.ptr(mean), L.ptr(m2), int(count), L.stream())
    return int(count) + T


def field_stats(x: torch.Tensor, norms=((0, 0), (0, 0))) -> np.ndarray:
    """(C + 2, 4) fp64 [min, max, sum, sum of squares] of the columns of ``x`` (rows, C <= 8) fp32 and, in the last two
    rows, of the row-wise L2 norms over the two column ranges ``norms`` = ((lo0, hi0), (lo1, hi1))."""
    if x.dtype != torch.float32 or x.ndim != 2 or not 1 <= x.shape[1] <= 8 or x.shape[0] < 1:
        raise RuntimeError(f"field_stats: expected fp32 (rows, C <= 8), got {x.dtype} {tuple(x.shape)}")
    rows, C = x.shape
    (lo0, hi0), (lo1, hi1) = norms
    xp = L.ptr(x)
    ws = torch.empty(L.query("tdx_field_stats_workspace_bytes", rows, C), dtype=torch.uint8, device=x.device)
    out = torch.empty((C + 2, 4), dtype=torch.float64, device=x.device)
    L.call("tdx_field_stats", xp, rows, C, lo0, hi0, lo1, hi1, L.ptr(out), L.ptr(ws), L.stream())
    return out.cpu().numpy()


def w2n_assign(mean: torch.Tensor, var: torch.Tensor, cmean, cvar, *, sums: bool = False):
    """Nearest centroid of every cell under the 2-Wasserstein distance between diagonal normals: ``mean``, ``var``
    (n, 3) fp32 device tensors, ``cmean``, ``cvar`` (k, 3) fp64 (numpy or tensor).  Returns (idx (n) int32, dist (n) fp64)
    on the device, and with ``sums`` also the (k, 7) fp64 numpy table [count, sum of means, sum of variances] per cluster."""
    if mean.dtype != torch.float32 or var.dtype != torch.float32 or mean.ndim != 2 or mean.shape[1] != 3 or var.shape != mean.shape \
            or mean.shape[0] < 1:
        raise RuntimeError(f"w2n_assign: expected fp32 (n, 3) cells, got {mean.dtype} {tuple(mean.shape)} / {var.dtype} {tuple(var.shape)}")
    mp, vp = L.ptr(mean), L.ptr(var)
    dev, n = mean.device, mean.shape[0]
    cm = torch.as_tensor(np.ascontiguousarray(cmean, dtype=np.float64) if not isinstance(cmean, torch.Tensor) else cmean)
    cv = torch.as_tensor(np.ascontiguousarray(cvar, dtype=np.float64) if not isinstance(cvar, torch.Tensor) else cvar)
    cm, cv = cm.to(dev, torch.float64).contiguous(), cv.to(dev, torch.float64).contiguous()
    k = cm.shape[0]
    if cm.shape != (k, 3) or cv.shape != (k, 3) or not 1 <= k <= W2N_MAX_K:
        raise RuntimeError(f"w2n_assign: expected (k <= {W2N_MAX_K}, 3) centroids, got {tuple(cm.shape)} / {tuple(cv.shape)}")
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    partials = None
    if sums:
        blocks = L.query("tdx_w2n_blocks", n)
        partials = torch.empty((blocks, k, 7), dtype=torch.float64, device=dev)
    L.call("tdx_w2n_assign", mp, vp, n, L.ptr(cm), L.ptr(cv), k, L.ptr(idx), L.ptr(dist), L.ptr(partials), L.stream())
    if not sums:
        return idx, dist
    table = torch.empty((k, 7), dtype=torch.float64, device=dev)
    L.call("tdx_w2n_reduce", L.ptr(partials), partials.shape[0], k, L.ptr(table), L.stream())
    return idx, dist, table.cpu().numpy()


# ------------------------------------------------------------------------------------------------ host arithmetic
def plan_chunks(frames, chunk_frames: int):
    """The frame indices ``frames`` (or ``range(frames)``) in ``ceil(len / chunk_frames)`` nearly equal runs, as
    ``np.array_split`` cuts them (scripts/dataset-stats.py:57-63)."""
    if chunk_frames < 1:
        raise ValueError(f"chunk_frames must be positive, got {chunk_frames}")
    idxs = np.arange(frames) if np.isscalar(frames) else np.asarray(frames)
    if len(idxs) == 0:
        return []
    return np.array_split(idxs, math.ceil(len(idxs) / chunk_frames))


def frames_after(times, discard_first: float) -> np.ndarray:
    """Indices of the frames with t > discard_first (strictly)."""
    return np.nonzero(np.asarray(times) > discard_first)[0]


def w2_normal(a_mean, a_var, b_mean, b_var) -> np.ndarray:
    """(len(a), len(b)) 2-Wasserstein distances between diagonal normals in fp64 on the host: the k x k convergence test of
    the Lloyd iteration."""
    a_mean, a_var, b_mean, b_var = (np.asarray(t, dtype=np.float64) for t in (a_mean, a_var, b_mean, b_var))
    diff = a_mean[:, None, :] - b_mean[None, :, :]
    d2 = (diff * diff).sum(-1) + a_var.sum(-1)[:, None] + b_var.sum(-1)[None, :] \
        - 2.0 * np.sqrt(a_var[:, None, :] * b_var[None, :, :]).sum(-1)
    return np.sqrt(np.clip(d2, 0.0, None))


def split_large_clusters(assignments: np.ndarray, k: int, max_cluster_size: int) -> np.ndarray:
    """Clusters of more than ``max_cluster_size`` cells are cut into ceil(count / max) pieces in ``np.array_split`` order of
    their cell indices; the first piece keeps the cluster's index, the others take k, k + 1, ... in cluster order."""
    out = assignments.copy()
    counts = np.bincount(assignments, minlength=k)
    nxt = k
    for c in range(k):
        if counts[c] <= max_cluster_size:
            continue
        cells = np.nonzero(assignments == c)[0]
        for piece in np.array_split(cells, math.ceil(counts[c] / max_cluster_size))[1:]:
            out[piece] = nxt
            nxt += 1
    return out


def _finish_stats(mn, mx, total, s, sq) -> dict:
    mean = s / total
    std = np.sqrt(sq / total - mean**2)
    return {"min": mn.astype(np.float32), "max": mx.astype(np.float32), "mean": mean.astype(np.float32),
            "std": std.astype(np.float32)}


class _RunningStats:
    """min / max / count / sum / sum of squares of one field over the chunks, sums in np.longdouble."""

    def __init__(self):
        self.mn = self.mx = None
        self.count = 0
        self.s = self.sq = None

    def add(self, rows4: np.ndarray, count: int):
        rows4 = np.atleast_2d(rows4)
        mn, mx = rows4[:, 0], rows4[:, 1]
        s, sq = rows4[:, 2].astype(np.longdouble), rows4[:, 3].astype(np.longdouble)
        if self.mn is None:
            self.mn, self.mx, self.s, self.sq = mn.copy(), mx.copy(), s, sq
        else:
            self.mn, self.mx = np.minimum(self.mn, mn), np.maximum(self.mx, mx)
            self.s, self.sq = self.s + s, self.sq + sq
        self.count += count

    def finish(self) -> dict:
        return _finish_stats(self.mn, self.mx, np.longdouble(self.count), self.s, self.sq)


# ------------------------------------------------------------------------------------------------ stats.pickle
def dataset_stats(root, *, chunk_frames: int = 10, opener=None, list_cases=None, device=None) -> dict:
    """Statistics over every frame and cell of every case under ``<root>/train``: for ``p``, ``u``, ``norm(u)``,
    ``norm(curl)``, ``k`` and ``nut`` the ``min``, ``max``, ``mean = sum / N`` and ``std = sqrt(sum x^2 / N - mean^2)`` as
    float32 arrays ((3,) for ``u``, (1,) otherwise) -- the contents of ``stats.pickle``.

    Per chunk of frames, ``tdx_ot_features`` with unit scale gives [u, curl u, p] at the in-domain cells and one
    ``tdx_field_stats`` pass reduces it, with the norms of lanes 0-2 and 3-5; ``k`` and ``nut`` are one-column passes."""
    from .. import ot

    dev = _device(device)
    files = (list_cases or find_data_files)(Path(root) / "train")
    if not files:
        raise RuntimeError(f"no case files under {Path(root) / 'train'}")
    repo = OpenFOAMDataRepository(files, (V.U, V.P, V.K, V.NUT), opener=opener)
    acc = {f: _RunningStats() for f in STATS_FIELDS}
    ones = torch.ones(7, dtype=torch.float32, device=dev)
    for case in range(repo.n_cases):
        meta = repo.read_metadata(case).to(dev)
        uidx = meta.unpadded_cell_idx
        for idxs in plan_chunks(len(repo.times[case]), chunk_frames):
            host = repo.read(case, idxs.tolist())
            data = OpenFOAMData(meta, host.t, {v: s.to(dev).contiguous() for v, s in host.samples.items()})
            u, p = data.samples[V.U], data.samples[V.P]
            feat = ot.features(data.grid_embedding((V.U,)), u, p, uidx, ones, meta.h)  # (S, n, 8) = [u, curl u, p, 0]
            n = feat.shape[0] * feat.shape[1]
            st = field_stats(feat.view(n, 8), norms=((0, 3), (3, 6)))
            acc["u"].add(st[0:3], n)
            acc["p"].add(st[6], n)
            acc["norm(u)"].add(st[8], n)
            acc["norm(curl)"].add(st[9], n)
            for name, v in (("k", V.K), ("nut", V.NUT)):
                acc[name].add(field_stats(data.samples[v].view(n, 1))[0], n)
    return {f: acc[f].finish() for f in STATS_FIELDS}


def write_stats(root, **kwargs) -> dict:
    """``dataset_stats`` pickled to ``<root>/stats.pickle``, the file ``OpenFOAMStats.from_file`` loads."""
    stats = dataset_stats(root, **kwargs)
    (Path(root) / "stats.pickle").write_bytes(pickle.dumps(stats))
    return stats


# ------------------------------------------------------------------------------------------------ temporal moments
@dataclass
class Moments:
    """Temporal moments of one field over ``count`` frames: fp64 device tensors shaped like one frame."""

    mean: torch.Tensor
    m2: torch.Tensor
    count: int

    @property
    def var(self) -> torch.Tensor:
        """Population variance, as ``np.var`` computes it."""
        return self.m2 / self.count


def temporal_moments(case_dir, fields=("u", "p"), *, discard_first: float = 0.025, chunk_frames: int = 10, opener=None,
                     device=None) -> dict:
    """{field: Moments} of ``data/<field>`` over the frames with t > ``discard_first``, read ``chunk_frames`` at a time."""
    dev = _device(device)
    out = {}
    with (opener or _open_h5)(Path(case_dir) / "data.h5", "r") as f:
        select = frames_after(np.array(f["data/times"]), discard_first)
        if len(select) == 0:
            raise RuntimeError(f"{case_dir}: no frame with t > {discard_first}")
        for name in fields:
            ds = f["data"][name]
            shape = tuple(ds.shape[1:])
            n = int(np.prod(shape))
            mean = torch.empty(n, dtype=torch.float64, device=dev)
            m2 = torch.empty(n, dtype=torch.float64, device=dev)
            count = 0
            for idxs in plan_chunks(select, chunk_frames):
                x = torch.from_numpy(np.ascontiguousarray(ds[idxs], dtype=np.float32)).to(dev)
                count = moments_update(x.view(len(idxs), n), mean, m2, count)
            out[name] = Moments(mean.view(shape), m2.view(shape), count)
    return out


def mean_flow(case_dir, *, discard_first: float = 0.025, chunk_frames: int = 10, opener=None, device=None, moments=None) -> dict:
    """Temporal mean of ``u`` and ``p`` over the frames with t > ``discard_first``, written as float32 ``data/u`` (n, 3)
    and ``data/p`` (n,) to ``<case_dir>/mean-flow.h5``.  ``moments``: a ``temporal_moments`` result to reuse."""
    if moments is None:
        moments = temporal_moments(case_dir, ("u", "p"), discard_first=discard_first, chunk_frames=chunk_frames,
                                   opener=opener, device=device)
    out = {name: moments[name].mean.to(torch.float32).cpu().numpy() for name in ("u", "p")}
    with (opener or _open_h5)(Path(case_dir) / "mean-flow.h5", "w") as f:
        group = f.require_group("data")
        group.create_dataset("u", data=out["u"])
        group.create_dataset("p", data=out["p"])
    return out


# ------------------------------------------------------------------------------------------------ regions.npz
@dataclass
class RegionsResult:
    assignments: np.ndarray          # (n,) int64, after splitting if max_cluster_size is given
    raw_assignments: np.ndarray      # (n,) int64, the k-means' own
    initial_centroids: np.ndarray    # (k,) the k-means++ picks, in draw order
    iterations: int                  # Lloyd iterations run
    converged: bool
    cluster_distance: np.ndarray     # (k,) mean distance of a cluster's cells to its centroid


def kmeans_w2(u_mean: torch.Tensor, u_var: torch.Tensor, *, seed: int = 713879, k: int = 32, epsilon: float = 1e-3,
              max_iter: int = 100) -> RegionsResult:
    """k-means++ and Lloyd iterations over cells with ``u_mean``, ``u_var`` (n, 3) fp32 device tensors under the
    2-Wasserstein distance between diagonal normals; stops when the mean distance between new and old centroids falls
    below ``epsilon`` (checked after the update), then assigns once more."""
    n = u_mean.shape[0]
    if not 1 <= k <= min(n, W2N_MAX_K):
        raise ValueError(f"k must be in [1, min(n_cells = {n}, {W2N_MAX_K})], got {k}")
    rng = np.random.default_rng(seed)
    mean_h, var_h = u_mean.cpu().numpy().astype(np.float64), u_var.cpu().numpy().astype(np.float64)
    cmean, cvar = np.empty((k, 3)), np.empty((k, 3))
    picks = np.empty(k, dtype=int)
    picks[0] = rng.choice(n)
    for i in range(1, k + 1):
        cmean[i - 1], cvar[i - 1] = mean_h[picks[i - 1]], var_h[picks[i - 1]]
        if i == k:
            break
        _, dist = w2n_assign(u_mean, u_var, cmean[:i], cvar[:i])
        D = dist.cpu().numpy()
        D[picks[:i]] = 0  # never the same cell twice
        D_sq = D**2
        picks[i] = rng.choice(n, p=D_sq / D_sq.sum())

    iterations, converged = 0, False
    for _ in range(max_iter):
        _, _, table = w2n_assign(u_mean, u_var, cmean, cvar, sums=True)
        iterations += 1
        counts = table[:, 0]
        if (counts == 0).any():
            empty = int(np.flatnonzero(counts == 0)[0])
            raise RuntimeError(f"k-means: cluster {empty} has no cells after iteration {iterations}; use a smaller k or another seed")
        old_mean, old_var = cmean, cvar
        cmean, cvar = table[:, 1:4] / counts[:, None], table[:, 4:7] / counts[:, None]
        if np.trace(w2_normal(cmean, cvar, old_mean, old_var)) / k < epsilon:
            converged = True
            break

    idx, dist = w2n_assign(u_mean, u_var, cmean, cvar)
    raw = idx.cpu().numpy().astype(np.int64)
    counts = np.bincount(raw, minlength=k)
    if (counts == 0).any():
        raise RuntimeError(f"k-means: cluster {int(np.flatnonzero(counts == 0)[0])} has no cells in the final assignment")
    cluster_distance = np.bincount(raw, weights=dist.cpu().numpy(), minlength=k) / counts
    return RegionsResult(raw, raw, picks, iterations, converged, cluster_distance)


def homogeneous_regions(case_dir, *, discard_first: float = 0.025, seed: int = 713879, k: int = 32, epsilon: float = 1e-3,
                        max_iter: int = 100, max_cluster_size=None, chunk_frames: int = 10, opener=None, device=None,
                        moments=None) -> RegionsResult:
    """The homogeneous regions of a case: k-means of the cells by the temporal mean and population variance of ``u`` over the
    frames with t > ``discard_first``.  Writes ``<case_dir>/regions.npz`` with ``assignments`` (and ``raw_assignments`` when
    clusters larger than ``max_cluster_size`` are split).  ``moments``: a ``temporal_moments`` result to reuse."""
    if moments is None:
        moments = temporal_moments(case_dir, ("u",), discard_first=discard_first, chunk_frames=chunk_frames, opener=opener,
                                   device=device)
    mo = moments["u"]
    res = kmeans_w2(mo.mean.to(torch.float32).contiguous(), mo.var.to(torch.float32).contiguous(), seed=seed, k=k,
                    epsilon=epsilon, max_iter=max_iter)
    arrays = {"assignments": res.raw_assignments}
    if max_cluster_size is not None:
        res.assignments = split_large_clusters(res.raw_assignments, k, max_cluster_size)
        arrays = {"assignments": res.assignments, "raw_assignments": res.raw_assignments}
    np.savez(Path(case_dir) / "regions.npz", **arrays)
    return res


# ------------------------------------------------------------------------------------------------ max-mean-tke.npy
DEFAULT_TKE_FRAMES = range(2500, 5000, 10)


def max_mean_tke(case_dir, *, frames=DEFAULT_TKE_FRAMES, chunk_frames: int = 10, opener=None, device=None) -> float:
    """Position along the channel of the maximum of the mean TKE profile behind the obstacle (scripts/max-mean-tke.py):
    fluctuation of the embedded ``u`` around its mean over ``frames``, ``[..., 24:, :, :]``, TKE profile over the cross
    section, mean over the frames of its argmax, + 24.  Written to ``<case_dir>/max-mean-tke.npy``.

    The mean over the frames comes from ``tdx_moments_update`` and is embedded once (fixed boundary values are the same in
    every frame); the frames are then embedded ``chunk_frames`` at a time."""
    dev = _device(device)
    frames = np.asarray(list(frames))
    repo = OpenFOAMDataRepository([Path(case_dir) / "data.h5"], (V.U,), opener=opener)
    meta = repo.read_metadata(0).to(dev)
    n = meta.n_cells
    if len(frames) == 0 or frames.max() >= len(repo.times[0]):
        raise RuntimeError(f"{case_dir}: frames up to {frames.max() if len(frames) else None} asked, {len(repo.times[0])} stored")
    mean = torch.empty(n * 3, dtype=torch.float64, device=dev)
    m2 = torch.empty(n * 3, dtype=torch.float64, device=dev)
    chunks = plan_chunks(frames, chunk_frames)
    count = 0
    for idxs in chunks:
        u = repo.read(0, idxs.tolist()).samples[V.U].to(dev).contiguous()
        count = moments_update(u.view(len(idxs), n * 3), mean, m2, count)
    t0 = torch.zeros(1)
    u_mean = OpenFOAMData(meta, t0, {V.U: mean.to(torch.float32).view(1, n, 3)}).grid_embedding((V.U,))[0]
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for idxs in chunks:
        host = repo.read(0, idxs.tolist())
        u = OpenFOAMData(meta, host.t, {V.U: host.samples[V.U].to(dev).contiguous()}).grid_embedding((V.U,))
        u_fluc = (u - u_mean)[..., 24:, :, :]
        tke = 0.5 * (u_fluc**2).sum(dim=-4)
        total += tke.mean(dim=(-1, -2)).argmax(dim=1).double().sum()
    value = float((total / len(frames)).float() + 24)
    np.save(Path(case_dir) / "max-mean-tke.npy", value)
    return value


# ------------------------------------------------------------------------------------------------ drivers
PRODUCTS = ("stats", "mean-flow", "regions", "max-mean-tke")


def prepare_case(case_dir, *, discard_first: float = 0.025, seed: int = 713879, k: int = 32, epsilon: float = 1e-3,
                 max_iter: int = 100, max_cluster_size=None, frames=DEFAULT_TKE_FRAMES, chunk_frames: int = 10, opener=None,
                 device=None, only=None) -> dict:
    """Write ``mean-flow.h5``, ``regions.npz`` and ``max-mean-tke.npy`` of one case (``only``: one of them, or several).
    ``u`` is read once for the mean flow and the regions."""
    only = (only,) if isinstance(only, str) else only
    want = [p for p in PRODUCTS[1:] if only is None or p in only]
    io = dict(chunk_frames=chunk_frames, opener=opener, device=device)
    out = {}
    moments = None
    if "mean-flow" in want or "regions" in want:
        fields = ("u", "p") if "mean-flow" in want else ("u",)
        moments = temporal_moments(case_dir, fields, discard_first=discard_first, **io)
    if "mean-flow" in want:
        out["mean-flow"] = mean_flow(case_dir, discard_first=discard_first, moments=moments, **io)
    if "regions" in want:
        out["regions"] = homogeneous_regions(case_dir, discard_first=discard_first, seed=seed, k=k, epsilon=epsilon,
                                             max_iter=max_iter, max_cluster_size=max_cluster_size, moments=moments, **io)
    if "max-mean-tke" in want:
        out["max-mean-tke"] = max_mean_tke(case_dir, frames=frames, **io)
    return out


def prepare_dataset(root, *, phases=("train", "val", "test"), list_cases=None, only=None, **kwargs) -> dict:
    """``prepare_case`` for every case of every phase directory under ``root`` that exists, and ``stats.pickle`` from the
    training cases.  ``only``: one of ``PRODUCTS``."""
    if only is not None and only not in PRODUCTS:
        raise ValueError(f"unknown product {only!r}, expected one of {PRODUCTS}")
    root = Path(root)
    lister = list_cases or find_data_files
    io = {key: kwargs[key] for key in ("chunk_frames", "opener", "device") if key in kwargs}
    out = {}
    if only in (None, "stats"):
        out["stats"] = write_stats(root, list_cases=list_cases, **io)
    if only != "stats":
        for phase in phases:
            if list_cases is None and not (root / phase).is_dir():
                continue
            for file in lister(root / phase):
                out[str(Path(file).parent)] = prepare_case(Path(file).parent, only=only, **kwargs)
    return out
