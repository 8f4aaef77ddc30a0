"""Seeded case files for the case-preparation tests, shared by tests/golden/make_golden_prepare.py (which runs the
reference's scripts on them) and the tests (which run turbdiff_amd.data.prepare on them): the inputs are regenerated from
their seeds, only the reference's outputs are stored in tests/golden/prepare.npz.

All trees live in tests/h5fake.py's in-memory store under a path the caller chooses; products that are not HDF5
(regions.npz, max-mean-tke.npy, stats.pickle) are written to the real file system, so the paths point into a temporary
directory.
"""

from pathlib import Path

import numpy as np

import h5fake

STATS_CHUNK = 4           # --chunk-size of the golden dataset-stats.py run: 11 and 12 frames in uneven chunks
PROTO_K = 8               # groups of the prototype case, and -k of the golden homogeneous-regions.py runs
PROTO_SEED = 713879       # the script's default --seed
PROTO_MAX_CLUSTER = 200   # --max-cluster-size of the second run: below the largest groups
PROTO_DISCARD = 0.025
TKE_FRAMES = 5000


def install_stats_cases(root):
    """Two training cases with different grids, 11 and 12 frames: {"train": [paths]}."""
    return h5fake.install_cases(root_dir=str(root), phases=("train",), per_phase=2)


def prototype_groups(n, rng):
    return rng.choice(PROTO_K, size=n, p=[0.3, 0.2, 0.12, 0.1, 0.08, 0.08, 0.07, 0.05])


def prototype_case(path):
    """A case of 1444 cells whose per-cell (mean, variance) of u take PROTO_K well-separated values with a jitter of 1e-3:
    u[t, cell] = m[group] + s[group] w[t] + 1e-3 noise over the 36 frames with t > 0.025, w a fixed sequence of zero mean and
    unit variance; the four frames at t <= 0.025 (one of them at exactly 0.025) hold values far away, so a filter that lets
    one of them through is seen.  Returns (tree, groups)."""
    rng = np.random.default_rng(20261020)
    n_early, n_late = 4, 36
    T = n_early + n_late
    tree = h5fake.make_case(5, counts=(14, 13, 13), n_times=T)
    n = tree["data/u"].shape[1]
    groups = prototype_groups(n, rng)
    g = np.arange(PROTO_K)
    m = 3.0 * np.stack([g % 2, (g // 2) % 2, g // 4], axis=1)                # corners of a cube of side 3
    s = (0.4 + 0.2 * g)[:, None] * np.array([1.0, 0.8, 0.6])[None, :]
    w = rng.standard_normal(n_late)
    w = (w - w.mean()) / w.std()
    u = np.empty((T, n, 3))
    u[:n_early] = 50.0 + 10.0 * rng.standard_normal((n_early, n, 3))
    u[n_early:] = m[groups][None] + s[groups][None] * w[:, None, None] + 1e-3 * rng.standard_normal((n_late, n, 3))
    times = np.concatenate(([0.0, 0.01, 0.02, PROTO_DISCARD], PROTO_DISCARD + 0.005 * np.arange(1, n_late + 1)))
    tree.put("data/times", np.round(times, 4))
    tree.put("data/u", u.astype(np.float32))
    p = np.array(tree["data/p"]).copy()
    p[:n_early] += 30.0
    tree.put("data/p", p)
    h5fake.TREES[str(path)] = tree
    return tree, groups


def tke_case(path):
    """TKE_FRAMES frames on a padded 30 x 6 x 7 grid: just longer than the 24 cells scripts/max-mean-tke.py cuts off, and as
    many frames as its fixed frame list range(2500, 5000, 10) needs."""
    tree = h5fake.make_case(9, counts=(30, 6, 7), n_times=TKE_FRAMES)
    h5fake.TREES[str(path)] = tree
    return tree


def w2n_inputs(seed=3, n=40, k=5):
    """Cells (float32) and centroids (float64) for the distance formula: means ~ N(0, 1), variances in [0.05, 1.5]."""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((n, 3)).astype(np.float32)
    var = rng.uniform(0.05, 1.5, (n, 3)).astype(np.float32)
    cmean = rng.standard_normal((k, 3))
    cvar = rng.uniform(0.05, 1.5, (k, 3))
    return mean, var, cmean, cvar


def case_dir(tmp, name):
    d = Path(tmp) / name
    d.mkdir(parents=True, exist_ok=True)
    return d
