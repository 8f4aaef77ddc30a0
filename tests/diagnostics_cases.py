"""Seeded case files for the case-diagnostics tests, shared by tests/golden/make_golden_diagnostics.py (which runs the
reference's scripts on them) and the tests (which run turbdiff_amd.data.diagnostics on them): the inputs are regenerated
from their seeds, only the reference's outputs are stored in tests/golden/diagnostics.npz.

All trees live in tests/h5fake.py's in-memory store under a path the caller chooses; products that are not HDF5
(autocorrelation.npz, gaussian-smoothing-error.txt, the forecast table) are written to the real file system, so the paths
point into a temporary directory.
"""

from pathlib import Path

import numpy as np

import h5fake

RHO = 0.8                      # AR(1) coefficient of the velocity of every cell and component
AUTOCORR_FRAMES = 660          # 330 in the second half, for 201 lags
AUTOCORR_COUNTS = (16, 8, 7)   # padded; unpadded 14 x 6 x 5: the back of the channel is x >= 14 - 6 = 8, a strict subset
SMOOTH_EARLY, SMOOTH_LATE = 4, 137  # frames at t <= 0.025 (one of them at exactly 0.025) and after: 137 - 100 = 37 outputs
DISCARD = 0.025
FORECAST_SEEDS = (21, 22)      # (training case: gives the mean flow, test case: gives the data), same grid size
FORECAST_INFLOW, FORECAST_DIMS = "const", "3D"


def ar1_field(rng, frames, cells):
    """(frames, cells, 3) float32: mean[cell] + amplitude[cell] * a stationary AR(1) sequence of unit variance."""
    amplitude = rng.uniform(0.5, 2.0, (cells, 3))
    mean = 1.5 * rng.standard_normal((cells, 3))
    noise = rng.standard_normal((frames, cells, 3))
    f = np.empty_like(noise)
    f[0] = noise[0]
    for t in range(1, frames):
        f[t] = RHO * f[t - 1] + np.sqrt(1.0 - RHO**2) * noise[t]
    return (mean[None] + amplitude[None] * f).astype(np.float32)


def autocorr_case(path):
    """660 frames on a 14 x 6 x 5 grid with a hole (412 cells, 180 of them in the back, scattered through the cell list
    because grid/cell_idx is a permutation)."""
    tree = h5fake.make_case(31, counts=AUTOCORR_COUNTS, n_times=AUTOCORR_FRAMES)
    n = tree["data/u"].shape[1]
    tree.put("data/u", ar1_field(np.random.default_rng(20261021), AUTOCORR_FRAMES, n))
    h5fake.TREES[str(path)] = tree
    return tree


def smooth_case(path):
    """141 frames on the default 7 x 5 x 4 grid (132 cells): four early frames with values far away, so that a filter on the
    time that lets one through is seen, then 137 frames of the AR(1) field."""
    T = SMOOTH_EARLY + SMOOTH_LATE
    tree = h5fake.make_case(32, n_times=T)
    n = tree["data/u"].shape[1]
    rng = np.random.default_rng(20261022)
    u = np.empty((T, n, 3), dtype=np.float32)
    u[:SMOOTH_EARLY] = (50.0 + 10.0 * rng.standard_normal((SMOOTH_EARLY, n, 3))).astype(np.float32)
    u[SMOOTH_EARLY:] = ar1_field(rng, SMOOTH_LATE, n)
    times = np.concatenate(([0.0, 0.01, 0.02, DISCARD], DISCARD + 0.003 * np.arange(1, SMOOTH_LATE + 1)))
    tree.put("data/times", np.round(times, 4))
    tree.put("data/u", u)
    h5fake.TREES[str(path)] = tree
    return tree


def forecast_dirs(root):
    """(train case directory, test case directory) below the one inflow directory of the forecast walk."""
    base = Path(root) / f"inflow-{FORECAST_INFLOW}" / FORECAST_DIMS
    return base / "train" / "high-step", base / "test" / "high-step"


def forecast_cases(root):
    """Two cases of 132 cells with different seeds, 11 and 12 frames, registered where scripts/mean-forecast-errors.py looks
    for them; the directories are created (the script lists them with Path.glob).  Returns (train dir, test dir)."""
    train, test = forecast_dirs(root)
    for d, seed, frames in ((train, FORECAST_SEEDS[0], 11), (test, FORECAST_SEEDS[1], 12)):
        d.mkdir(parents=True, exist_ok=True)
        tree = h5fake.make_case(seed, n_times=frames)
        rng = np.random.default_rng(seed)
        n = tree["data/u"].shape[1]
        tree.put("data/u", (np.array(tree["data/u"]) + rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)[None]).astype(np.float32))
        tree.put("data/p", (np.array(tree["data/p"]) + rng.uniform(-2.0, 2.0, n).astype(np.float32)[None]).astype(np.float32))
        h5fake.TREES[str(d / "data.h5")] = tree
    return train, test


def install_mean_flow(case_dir, u, p=None):
    """Register <case_dir>/mean-flow.h5 with the given float32 fields (the reference's own, from the golden file)."""
    tree = h5fake.Group()
    tree.put("data/u", np.asarray(u, dtype=np.float32))
    if p is not None:
        tree.put("data/p", np.asarray(p, dtype=np.float32))
    h5fake.TREES[str(Path(case_dir) / "mean-flow.h5")] = tree
    return tree


def case_dir(tmp, name):
    d = Path(tmp) / name
    d.mkdir(parents=True, exist_ok=True)
    return d
