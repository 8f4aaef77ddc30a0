"""Case diagnostics: the per-case numbers of the reference's second group of scripts, streamed over time from ``data.h5``.

    <case>/autocorrelation.npz             ``autocorrelation``       (reference scripts/autocorrelation.py)
    <case>/gaussian-smoothing-error.txt    ``smoothing_error``       (scripts/gaussian-smoothing-error.py)
    the trivial-baseline MSE               ``mean_forecast_error``   (scripts/mean-forecast-errors.py)

The reductions run in HIP kernels (csrc/tdx_diagnostics.hip): ``tdx_lagprod_update`` adds the lagged products of the
fluctuating velocity chunk by chunk against a ring of the last ``max_lag`` frames kept on the device,
``tdx_smooth_residual_update`` the energy of ``u - smooth(u)`` for a bank of temporal filters against a halo of the last
``2 half_width`` frames, ``tdx_sqdev_sum`` the squared distance to a mean field.  The host keeps what is small: the chunk
plan, the cell selection, the filter taps (the reference's numpy expression in float64), the decorrelation rule, the files.
There is no CPU path: tensors handed to the kernels must be on the device.  Case files are opened through ``opener``, as in
``turbdiff_amd.data.prepare``.

Memory is bounded by ``chunk_frames`` plus the kernels' state.  At the size of a real case (485 000 cells, the back quarter
about 121 000, chunks of 10 frames):

    autocorrelation      chunk 58 MB + ring 200 x 363 000 x 4 B = 290 MB + staged fluctuations 15 MB
    smoothing_error      chunk 58 MB + halo 100 x 1 455 000 x 4 B = 582 MB
    mean_forecast_error  chunk 58 MB + mean 6 MB

Deliberate differences from the reference, both where it would go on silently:
  * ``autocorrelation`` raises ``ValueError`` when the second half of the case has fewer than ``max_lag + 1`` frames; the
    script would write zeros (and NaN after the division, if there is no frame at all) for the lags it never saw.
  * ``smoothing_error`` raises ``ValueError`` for fewer than ``2 half_width + 1`` frames; ``np.convolve(mode="valid")``
    would swap its operands there and smooth the kernel with the signal.
``mean_forecast_error`` keeps the script's rule as it is -- the last axis is summed, the others are averaged -- so ``u``
(frames, cells, 3) gives the sum over everything / (cells x frames), and ``p`` (frames, cells), whose last axis is the
cells, the sum / frames.
"""

from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from .. import _lib as L
from .ofles import OpenFOAMDataRepository, _open_h5
from .prepare import _device, frames_after, plan_chunks

LAGPROD_MAX_LAG = 255     # LP_MAX_LAG of csrc/tdx_diagnostics.hip
KERNEL_MAX_FRAMES = 64    # LP_MAX_FRAMES, SR_MAX_FRAMES: frames of one kernel call; longer chunks are passed in pieces
SMOOTH_MAX_WIDTHS = 32    # SR_MAX_W
SMOOTH_MAX_HALF = 50      # SR_MAX_H


def _pieces(x: torch.Tensor):
    for at in range(0, x.shape[0], KERNEL_MAX_FRAMES):
        yield x[at:at + KERNEL_MAX_FRAMES]


# ------------------------------------------------------------------------------------------------ streaming kernel states
class LagProducts:
    """Streaming lagged products of the fluctuating velocity (``tdx_lagprod_update``): after ``update`` has seen the frames
    x[0], x[1], ... ``result()[i]`` = sum over t >= i, the selected cells and the 3 components of f[t] f[t - i], with
    f = x[:, cells] - mean[cells] formed in float32 and the sums in fp64.

    ``cells``: ascending indices into the n cells; ``mean``: (n, 3) float32; ``max_lag`` <= 255."""

    def __init__(self, cells, mean, max_lag: int, device=None):
        dev = _device(device)
        cells = np.asarray(cells)
        mean = mean.detach().cpu().numpy() if isinstance(mean, torch.Tensor) else np.asarray(mean)
        if mean.ndim != 2 or mean.shape[1] != 3 or mean.dtype != np.float32:
            raise RuntimeError(f"LagProducts: expected a float32 (n, 3) mean, got {mean.dtype} {mean.shape}")
        n = mean.shape[0]
        if cells.ndim != 1 or len(cells) < 1 or cells.dtype.kind not in "iu" or cells.min() < 0 or cells.max() >= n \
                or (np.diff(cells) <= 0).any():
            raise ValueError(f"LagProducts: cells must be ascending indices into the {n} cells")
        if not 1 <= max_lag <= LAGPROD_MAX_LAG:
            raise ValueError(f"max_lag must be in [1, {LAGPROD_MAX_LAG}], got {max_lag}")
        self.n, self.m, self.max_lag, self.seen = n, len(cells), int(max_lag), 0
        self.cells = torch.from_numpy(cells.astype(np.int32)).to(dev)
        self.mean = torch.from_numpy(np.ascontiguousarray(mean)).to(dev)
        self.ring = torch.empty((self.max_lag, 3 * self.m), dtype=torch.float32, device=dev)
        self.acc = torch.zeros(self.max_lag + 1, dtype=torch.float64, device=dev)
        self._ws = None

    def update(self, x: torch.Tensor) -> int:
        """Add the frames ``x`` (F, n, 3) fp32 (device); returns the number of frames seen."""
        if x.dtype != torch.float32 or x.ndim != 3 or x.shape[1:] != (self.n, 3) or x.shape[0] < 1:
            raise RuntimeError(f"LagProducts.update: expected fp32 (F, {self.n}, 3), got {x.dtype} {tuple(x.shape)}")
        for piece in _pieces(x):
            F = piece.shape[0]
            need = L.query("tdx_lagprod_workspace_bytes", F, self.m, self.max_lag)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.ring.device)
            L.call("tdx_lagprod_update", L.ptr(piece), F, self.n, L.ptr(self.mean), L.ptr(self.cells), self.m, self.max_lag,
                   L.ptr(self.ring), L.ptr(self.acc), self.seen, L.ptr(self._ws), L.stream())
            self.seen += F
        return self.seen

    def result(self) -> np.ndarray:
        return self.acc.cpu().numpy()


class SmoothResidual:
    """Streaming energy of the outputs of a bank of temporal FIR filters (``tdx_smooth_residual_update``): after ``update``
    has seen T frames of n columns, ``result()[w]`` = sum over the T - 2 h output frames t and the columns of
    (sum_k taps[w, k] x[t + k])^2 in fp64.  ``taps``: (W <= 32, 2 h + 1) float64, h <= 50."""

    def __init__(self, taps, n: int, device=None):
        dev = _device(device)
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        if taps.ndim != 2 or not 1 <= taps.shape[0] <= SMOOTH_MAX_WIDTHS or taps.shape[1] % 2 != 1 \
                or not 1 <= taps.shape[1] // 2 <= SMOOTH_MAX_HALF:
            raise ValueError(f"SmoothResidual: expected (W <= {SMOOTH_MAX_WIDTHS}, 2 h + 1) taps with 1 <= h <= {SMOOTH_MAX_HALF}, "
                             f"got {taps.shape}")
        self.W, self.h, self.n, self.seen = taps.shape[0], taps.shape[1] // 2, int(n), 0
        self.taps = torch.from_numpy(taps).to(dev)
        self.halo = torch.empty((2 * self.h, self.n), dtype=torch.float32, device=dev)
        self.acc = torch.zeros(self.W, dtype=torch.float64, device=dev)
        self._ws = torch.empty(L.query("tdx_smooth_residual_workspace_bytes", self.n, self.W), dtype=torch.uint8, device=dev)

    @property
    def out_frames(self) -> int:
        return max(0, self.seen - 2 * self.h)

    def update(self, x: torch.Tensor) -> int:
        """Add the frames ``x`` (F, n) fp32 (device); returns the number of frames seen."""
        if x.dtype != torch.float32 or x.ndim != 2 or x.shape[1] != self.n or x.shape[0] < 1:
            raise RuntimeError(f"SmoothResidual.update: expected fp32 (F, {self.n}), got {x.dtype} {tuple(x.shape)}")
        for piece in _pieces(x):
            F = piece.shape[0]
            L.call("tdx_smooth_residual_update", L.ptr(piece), F, self.n, L.ptr(self.taps), self.W, self.h, L.ptr(self.halo),
                   L.ptr(self.acc), self.seen, L.ptr(self._ws), L.stream())
            self.seen += F
        return self.seen

    def result(self) -> np.ndarray:
        return self.acc.cpu().numpy()


def sqdev_sum(x: torch.Tensor, mean: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The fp64 sum of the float32 values ``(x - mean) ** 2``: ``x`` (T, n, C) or (T, n) fp32, ``mean`` shaped like one frame,
    C <= 4.  With ``out`` (a one-element fp64 device tensor) the sum is added to it."""
    if x.dtype != torch.float32 or mean.dtype != torch.float32 or x.ndim not in (2, 3) or x.shape[1:] != mean.shape \
            or x.shape[0] < 1 or (x.ndim == 3 and not 1 <= x.shape[2] <= 4):
        raise RuntimeError(f"sqdev_sum: expected fp32 (T, n[, C <= 4]) and a mean shaped like a frame, got {x.dtype} "
                           f"{tuple(x.shape)} / {mean.dtype} {tuple(mean.shape)}")
    T, n = x.shape[0], x.shape[1]
    C = x.shape[2] if x.ndim == 3 else 1
    xp, mp = L.ptr(x), L.ptr(mean)
    accumulate = out is not None
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.numel() != 1:
        raise RuntimeError(f"sqdev_sum: out must be one fp64 element, got {out.dtype} {tuple(out.shape)}")
    ws = torch.empty(L.query("tdx_sqdev_workspace_bytes", n, C), dtype=torch.uint8, device=x.device)
    L.call("tdx_sqdev_sum", xp, mp, T, n, C, int(accumulate), L.ptr(out), L.ptr(ws), L.stream())
    return out


# ------------------------------------------------------------------------------------------------ host arithmetic
def back_cells(unpadded_cell_idx, unpadded_cell_counts) -> np.ndarray:
    """Ascending positions (into the case's cell list) of the cells in the back of the channel: unpadded x index >=
    counts[0] - max(counts[1:]) (scripts/autocorrelation.py:28-30)."""
    counts = [int(c) for c in unpadded_cell_counts]
    idx = np.asarray(unpadded_cell_idx)
    x = idx // (counts[1] * counts[2])
    return np.nonzero(x >= counts[0] - max(counts[1:]))[0]


def decorrelation(corrcoeff, tail: int = 100):
    """(decorrelation_steps, max_decorrelated_coeff): the threshold is max |corrcoeff[-tail:]|, the step count the first index
    whose |coefficient| is at or below it, plus one (scripts/autocorrelation.py:53-59).  The last coefficient always
    qualifies."""
    c = np.abs(np.asarray(corrcoeff, dtype=np.float64))
    if not 1 <= tail <= len(c):
        raise ValueError(f"tail must be in [1, {len(c)}], got {tail}")
    threshold = c[-tail:].max()
    return int(np.nonzero(c <= threshold)[0][0]) + 1, float(threshold)


def gaussian_taps(widths=None, half_width: int = 50) -> np.ndarray:
    """(len(widths), 2 half_width + 1) float64: the normalised Gaussian kernels of scripts/gaussian-smoothing-error.py:29-31,
    by the script's own expression."""
    widths = np.linspace(1, 32, 32) if widths is None else np.asarray(widths, dtype=np.float64)
    out = []
    for kernel_width in widths:
        kernel = np.exp(-np.linspace(-half_width, half_width, 2 * half_width + 1) ** 2 / (2 * kernel_width**2))
        kernel /= kernel.sum()
        out.append(kernel)
    return np.stack(out)


def residual_taps(widths=None, half_width: int = 50) -> np.ndarray:
    """delta - g per width: the filter whose output is u - smooth(u), so that the kernel never forms that difference from two
    large numbers."""
    taps = -gaussian_taps(widths, half_width)
    taps[:, half_width] += 1.0
    return taps


def _read_mean_flow(case_dir, opener, fields=("u",)) -> dict:
    path = Path(case_dir) / "mean-flow.h5"
    try:
        with (opener or _open_h5)(path, "r") as f:
            return {name: np.ascontiguousarray(np.array(f[f"data/{name}"]), dtype=np.float32) for name in fields}
    except (FileNotFoundError, KeyError, OSError) as e:
        raise FileNotFoundError(f"{path} is missing or incomplete: write it first with turbdiff_amd.data.prepare.mean_flow "
                                f"(tools/prepare_dataset.py --only mean-flow)") from e


# ------------------------------------------------------------------------------------------------ autocorrelation.npz
@dataclass
class AutocorrelationResult:
    corrcoeff: np.ndarray            # (max_lag + 1,) float64, corrcoeff[0] = 1
    decorrelation_steps: int
    max_decorrelated_coeff: float


def autocorrelation(case_dir, *, max_lag: int = 200, tail: int = 100, chunk_frames: int = 10, write: bool = True,
                    opener=None, device=None) -> AutocorrelationResult:
    """Temporal autocorrelation of the fluctuating velocity in the back of the channel over the second half of the case's
    frames (all of them: this script has no time filter), for the lags 0 ... ``max_lag``, normalised by lag 0; and the
    number of steps after which two frames count as decorrelated.  The mean flow is read from ``<case_dir>/mean-flow.h5``.
    Writes ``<case_dir>/autocorrelation.npz`` with ``decorrelation_steps`` and ``corrcoeff`` (float64)."""
    if not 1 <= tail <= max_lag + 1:
        raise ValueError(f"tail must be in [1, max_lag + 1 = {max_lag + 1}], got {tail}")
    dev = _device(device)
    case_dir = Path(case_dir)
    u_mean = _read_mean_flow(case_dir, opener)["u"]
    repo = OpenFOAMDataRepository([case_dir / "data.h5"], (), opener=opener)
    meta = repo.read_metadata(0)
    cells = back_cells(meta.unpadded_cell_idx.cpu().numpy(), meta.unpadded_cell_counts)
    if len(cells) == 0:
        raise RuntimeError(f"{case_dir}: no cell in the back of the channel")
    with (opener or _open_h5)(case_dir / "data.h5", "r") as f:
        ds = f["data"]["u"]
        n_steps = int(ds.shape[0])
        if tuple(ds.shape[1:]) != u_mean.shape:
            raise RuntimeError(f"{case_dir}: data/u has cells {tuple(ds.shape[1:])}, mean-flow.h5 {u_mean.shape}")
        frames = np.arange(n_steps // 2, n_steps)
        if len(frames) < max_lag + 1:
            raise ValueError(f"{case_dir}: {len(frames)} frames in the second half, lags up to {max_lag} need {max_lag + 1}")
        state = LagProducts(cells, u_mean, max_lag, dev)
        for idxs in plan_chunks(frames, chunk_frames):
            state.update(torch.from_numpy(np.ascontiguousarray(ds[idxs], dtype=np.float32)).to(dev))
    corr = state.result()
    corrcoeff = corr / corr[0]
    steps, threshold = decorrelation(corrcoeff, tail)
    if write:
        np.savez(case_dir / "autocorrelation.npz", decorrelation_steps=steps, corrcoeff=corrcoeff)
    return AutocorrelationResult(corrcoeff, steps, threshold)


# ------------------------------------------------------------------------------------------------ gaussian-smoothing-error.txt
def smoothing_error(case_dir, *, discard_first: float = 0.025, widths=None, half_width: int = 50, chunk_frames: int = 10,
                    write: bool = True, opener=None, device=None) -> np.ndarray:
    """MSE between ``u`` and ``u`` smoothed along time with a normalised Gaussian of ``2 half_width + 1`` taps, per kernel
    width in ``widths`` (default ``np.linspace(1, 32, 32)``), over the frames with t > ``discard_first`` that have a full
    window: sum of squares / (cells x output frames), float64.  Writes ``<case_dir>/gaussian-smoothing-error.txt``."""
    dev = _device(device)
    case_dir = Path(case_dir)
    taps = residual_taps(widths, half_width)
    with (opener or _open_h5)(case_dir / "data.h5", "r") as f:
        select = frames_after(np.array(f["data/times"]), discard_first)
        if len(select) < 2 * half_width + 1:
            raise ValueError(f"{case_dir}: {len(select)} frames with t > {discard_first}, a window needs {2 * half_width + 1}")
        ds = f["data"]["u"]
        n_cells = int(ds.shape[1])
        n = int(np.prod(ds.shape[1:]))
        state = SmoothResidual(taps, n, dev)
        for idxs in plan_chunks(select, chunk_frames):
            x = torch.from_numpy(np.ascontiguousarray(ds[idxs], dtype=np.float32)).to(dev)
            state.update(x.view(len(idxs), n))
    mses = state.result() / (n_cells * state.out_frames)
    if write:
        np.savetxt(case_dir / "gaussian-smoothing-error.txt", mses)
    return mses


# ------------------------------------------------------------------------------------------------ mean-forecast baseline
def mean_forecast_error(data_case, mean_case=None, *, fields=("u", "p"), chunk_frames: int = 10, opener=None,
                        device=None) -> dict:
    """{field: MSE} of forecasting every frame of ``<data_case>/data.h5`` by the mean flow in ``<mean_case>/mean-flow.h5``
    (default: the case's own), by the script's rule ``((x - mean) ** 2).sum(axis=-1).mean(axis=-1).mean()``: the float32
    squares are summed (here in fp64) and divided by the sizes of all axes but the last."""
    dev = _device(device)
    data_case = Path(data_case)
    means = _read_mean_flow(data_case if mean_case is None else mean_case, opener, fields)
    out = {}
    with (opener or _open_h5)(data_case / "data.h5", "r") as f:
        for name in fields:
            ds = f["data"][name]
            shape = tuple(ds.shape)
            if shape[1:] != means[name].shape:
                raise ValueError(f"{data_case}: data/{name} has cells {shape[1:]}, the mean flow {means[name].shape}")
            if shape[0] < 1:
                raise ValueError(f"{data_case}: no frame")
            mean = torch.from_numpy(means[name]).to(dev)
            total = torch.zeros(1, dtype=torch.float64, device=dev)
            for idxs in plan_chunks(shape[0], chunk_frames):
                sqdev_sum(torch.from_numpy(np.ascontiguousarray(ds[idxs], dtype=np.float32)).to(dev), mean, total)
            out[name] = float(total.item() / np.prod(shape[:-1]))
    return out

