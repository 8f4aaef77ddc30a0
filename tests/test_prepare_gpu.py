"""The case-preparation kernels (csrc/tdx_prepare.hip) and turbdiff_amd.data.prepare end to end on the GPU, against the numpy
statements of tests/prepare_reference.py and the reference scripts' own output in tests/golden/prepare.npz."""

import pickle

import numpy as np
import pytest
import torch

import h5fake
import prepare_cases as PC
import prepare_reference as R
from turbdiff_amd.data import prepare as P
from turbdiff_amd.data.ofles import OpenFOAMStats

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U53 = 2.0**-53


@pytest.fixture(scope="module")
def gold():
    from conftest import GOLDEN

    return np.load(GOLDEN / "prepare.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ moments
def test_moments_update_chunks_of_1_7_3():
    """n = 1031 * 3 columns (n % 4 = 1), chunks of 1, 7 and 3 frames merged in that order, against the two-pass float64
    result on the concatenation: mean and variance, cast to float32, are the oracle's cast or the float32 next to it.
    Column 0 is constant (variance exactly 0); column 1 has mean 1e3 and standard deviation 1e-2, where sum / sum of squares
    in float64 would be off by about 1e-6 relative, far outside one float32 step."""
    rng = np.random.default_rng(11)
    n, T = 1031 * 3, 11
    x = rng.standard_normal((T, n)).astype(np.float32) * rng.uniform(0.1, 3.0, n).astype(np.float32) \
        + rng.standard_normal(n).astype(np.float32)
    x[:, 0] = np.float32(0.7)
    x[:, 1] = (1e3 + 1e-2 * rng.standard_normal(T)).astype(np.float32)
    assert n % 4 != 0
    xd = dev(x)
    mean = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)  # empty state is never read
    m2 = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    count, at = 0, 0
    for t in (1, 7, 3):
        count = P.moments_update(xd[at:at + t].contiguous(), mean, m2, count)
        at += t
        if at == 1:  # T = 1 into empty state: the frame itself, no spread
            assert np.array_equal(mean.cpu().numpy(), x[0].astype(np.float64)) and (m2 == 0).all()
    assert count == T
    want_mean, want_var = R.temporal_moments(x)
    got_mean, got_var = mean.cpu().numpy(), (m2 / count).cpu().numpy()
    assert got_var[0] == 0.0 and (got_var >= 0).all()
    rel = np.abs(got_var[1] - want_var[1]) / want_var[1]
    print(f"moments: column (1e3, 1e-2) variance relative error {rel:.3e}; largest mean error "
          f"{np.abs(got_mean - want_mean).max():.3e}")
    assert R.adjacent_f32(got_mean.astype(np.float32), want_mean).all()
    assert R.adjacent_f32(got_var.astype(np.float32), want_var).all()


# ------------------------------------------------------------------------------------------------ field stats
def stats_oracle(x):
    """(C, 4) [min, max, sum, sum of float32 squares] in np.longdouble, and the bounds rows * 2^-53 * sum |.| of the sums."""
    rows = x.shape[0]
    sq = x * x
    assert sq.dtype == np.float32
    want = np.stack([x.min(0).astype(np.longdouble), x.max(0).astype(np.longdouble), x.sum(0, dtype=np.longdouble),
                     sq.sum(0, dtype=np.longdouble)], axis=1)
    bound = np.stack([rows * U53 * np.abs(x).sum(0, dtype=np.longdouble), rows * U53 * sq.sum(0, dtype=np.longdouble)], axis=1)
    return want, bound


def check_stats(got, x, what):
    want, bound = stats_oracle(x)
    assert np.array_equal(got[:, 0], want[:, 0].astype(np.float64)) and np.array_equal(got[:, 1], want[:, 1].astype(np.float64)), what
    err = np.abs(got[:, 2:].astype(np.longdouble) - want[:, 2:])
    print(f"field stats {what}: largest sum error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
    assert (err <= bound).all(), what


def test_field_stats():
    rng = np.random.default_rng(12)
    rows = 2 * 1031
    x = rng.standard_normal((rows, 8)).astype(np.float32)
    x[:, 0] = -np.abs(x[:, 0]) - 0.5                       # all negative
    x[:, 1] = np.abs(x[:, 1]) + 0.5                        # all positive
    x[:, 2] = np.where(np.arange(rows) % 2 == 0, 0.0, -0.0).astype(np.float32)  # +0 and -0 only
    x[:, 7] = 0.0
    xd = dev(x)
    got = P.field_stats(xd, norms=((0, 3), (3, 6)))
    assert got.shape == (10, 4)
    check_stats(got[:8], x, "columns of C = 8")
    assert got[2, 0] == 0.0 and got[2, 1] == 0.0 and got[2, 2] == 0.0
    norm = lambda a: np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])[:, None]  # float32 throughout
    check_stats(got[8:9], norm(x[:, 0:3]), "norm of lanes 0-2")
    check_stats(got[9:10], norm(x[:, 3:6]), "norm of lanes 3-5")
    assert np.array_equal(P.field_stats(xd, norms=((0, 3), (3, 6))), got), "two calls must give the same bits"
    # the one-column route (four rows per lane, rows % 4 = 2) and a width without a vector route
    one = np.ascontiguousarray(x[:, 3:4])
    g1 = P.field_stats(dev(one))
    check_stats(g1[:1], one, "C = 1")
    assert np.array_equal(g1[1:, :2], [[np.inf, -np.inf]] * 2) and (g1[1:, 2:] == 0).all()  # no norm asked
    three = np.ascontiguousarray(x[:777, 3:6])
    g3 = P.field_stats(dev(three), norms=((0, 3), (1, 2)))
    check_stats(g3[:3], three, "C = 3")
    check_stats(g3[3:4], norm(three), "norm of C = 3")
    check_stats(g3[4:5], np.sqrt(three[:, 1:2] * three[:, 1:2]), "norm of one lane")


def test_field_stats_past_one_grid():
    """300 001 rows at C = 8: more rows than the 1024 x 256 threads of the capped grid (threads take a second row) and more
    block partials than the folding block has threads -- the routes a real case takes."""
    rng = np.random.default_rng(15)
    rows = 300_001
    x = (rng.standard_normal((rows, 8)) * rng.uniform(0.5, 20.0, 8) + rng.uniform(-3, 3, 8)).astype(np.float32)
    xd = dev(x)
    got = P.field_stats(xd, norms=((0, 3), (3, 6)))
    check_stats(got[:8], x, "columns of C = 8, 300 001 rows")
    norm = lambda a: np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])[:, None]
    check_stats(got[8:9], norm(x[:, 0:3]), "norm of lanes 0-2, 300 001 rows")
    check_stats(got[9:10], norm(x[:, 3:6]), "norm of lanes 3-5, 300 001 rows")
    assert np.array_equal(P.field_stats(xd, norms=((0, 3), (3, 6))), got), "two calls must give the same bits"


# ------------------------------------------------------------------------------------------------ assignment
def cells(n, seed=13):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)).astype(np.float32), rng.uniform(0.05, 1.5, (n, 3)).astype(np.float32)


def centroids(k, seed=14):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((k, 3)), rng.uniform(0.05, 1.5, (k, 3))


def check_assignment(mean, var, cmean, cvar, idx, dist):
    """Distances within 1e-12 of the formula's magnitude in d^2; indices equal to the statement's except at cells whose two
    best d^2 are closer than 1e-10 of it, which may be at most 0.1 % of the cells."""
    n = len(mean)
    d2 = R.w2n_distance_sq(mean, var, cmean, cvar)
    mag = R.w2n_magnitude(mean, var, cmean, cvar)
    want = d2.argmin(axis=0)
    at = np.arange(n)
    assert idx.min() >= 0 and idx.max() < len(cmean)
    err = np.abs(dist**2 - d2[idx, at]) / mag[idx, at]
    if len(cmean) > 1:
        two = np.partition(d2, 1, axis=0)[:2]
        near = (two[1] - two[0]) < 1e-10 * mag[want, at]
    else:
        near = np.zeros(n, dtype=bool)
    print(f"assign n = {n}, k = {len(cmean)}: largest d^2 error / magnitude {err.max():.3e}, near-tie cells {int(near.sum())}, "
          f"index mismatches {int((idx != want).sum())}")
    assert (err <= 1e-12).all()
    assert near.sum() <= 1e-3 * n
    assert np.array_equal(idx[~near], want[~near])


@pytest.mark.parametrize("n,k", [(6000, 1), (6000, 32), (6000, 33), (255, 32), (257, 32)])
def test_w2n_assign(n, k):
    mean, var = cells(n)
    cmean, cvar = centroids(k)
    idx, dist = P.w2n_assign(dev(mean), dev(var), cmean, cvar)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float64 and idx.shape == dist.shape == (n,)
    check_assignment(mean, var, cmean, cvar, idx.cpu().numpy(), dist.cpu().numpy())


def test_w2n_assign_ties_and_exact_zero():
    """Two identical centroids: the lower index everywhere.  A cell identical to a centroid: distance exactly 0 -- for a
    cell whose three variances have an exact float32 sum (0.5, 0.25, 0.125), the only place where the formula's float32
    addition could leave a residue; sqrt(v v) = v is exact in float64 for float32 v."""
    mean, var = cells(6000)
    cmean, cvar = centroids(33)
    cmean[7], cvar[7] = cmean[3], cvar[3]
    mean[100], var[100] = (0.75, -1.5, 2.0), (0.5, 0.25, 0.125)
    cmean[20], cvar[20] = mean[100].astype(np.float64), var[100].astype(np.float64)
    idx, dist = P.w2n_assign(dev(mean), dev(var), cmean, cvar)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    want = R.w2n_distance_sq(mean, var, cmean, cvar).argmin(axis=0)
    assert (want == 3).sum() > 50 and (idx != 7).all() and np.array_equal(idx, want)
    assert idx[100] == 20 and dist[100] == 0.0


@pytest.mark.parametrize("n,k", [(6000, 33), (131072 + 257, 5), (257, 256)])
def test_w2n_reduce(n, k):
    """The (k, 7) table of one Lloyd pass against float64 numpy sums per cluster: counts exact, sums within
    count * 2^-53 * sum |x|; two calls give the same bits.  n = 131 329 is the first size range where a block walks more
    than one tile of 256 cells; k = 256 has more (cluster, component) items than a block has threads."""
    mean, var = cells(n)
    cmean, cvar = centroids(k)
    md, vd = dev(mean), dev(var)
    idx, dist, table = P.w2n_assign(md, vd, cmean, cvar, sums=True)
    idx_h = idx.cpu().numpy()
    check_assignment(mean, var, cmean, cvar, idx_h, dist.cpu().numpy())
    counts = np.bincount(idx_h, minlength=k)
    assert table.shape == (k, 7) and np.array_equal(table[:, 0], counts.astype(np.float64))
    x = np.concatenate([mean, var], axis=1).astype(np.float64)
    worst = 0.0
    for c in range(k):
        sel = x[idx_h == c]
        want = sel.sum(axis=0)
        bound = counts[c] * U53 * np.abs(sel).sum(axis=0)
        err = np.abs(table[c, 1:] - want)
        assert (err <= bound).all(), (c, err, bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"reduce n = {n}, k = {k}: largest sum error / bound {worst:.3e}")
    idx2, dist2, table2 = P.w2n_assign(md, vd, cmean, cvar, sums=True)
    assert torch.equal(idx, idx2) and torch.equal(dist, dist2) and np.array_equal(table, table2)
    idx3, dist3 = P.w2n_assign(md, vd, cmean, cvar)  # the pass without sums is the same assignment
    assert torch.equal(idx, idx3) and torch.equal(dist, dist3)


# ------------------------------------------------------------------------------------------------ end to end
def test_mean_flow_and_regions_on_the_prototype_case(tmp_path, gold):
    """prepare_case on the prototype case: mean-flow.h5 within T * 2^-24 * mean |x| per element of the reference's (the bound
    of the reference's own naive float32 sum over T = 36 frames; ours is the more exact side), the reference's k-means++
    picks, and its labels exactly, with and without --max-cluster-size."""
    case = PC.case_dir(tmp_path, "proto")
    tree, _ = PC.prototype_case(case / "data.h5")
    out = P.prepare_case(case, k=PC.PROTO_K, seed=PC.PROTO_SEED, chunk_frames=10, opener=h5fake.File, device=DEV,
                         only=("mean-flow", "regions"))
    sel = P.frames_after(np.array(tree["data/times"]), PC.PROTO_DISCARD)
    written = h5fake.TREES[str(case / "mean-flow.h5")]
    for name in ("u", "p"):
        got, ref = np.array(written[f"data/{name}"]), gold[f"proto/mean_flow/{name}"]
        assert got.dtype == np.float32 and got.shape == ref.shape
        bound = len(sel) * 2.0**-24 * np.abs(np.array(tree[f"data/{name}"])[sel].astype(np.float64)).mean(0)
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        print(f"mean flow {name}: largest error / bound {(err / bound).max():.3e}")
        assert (err <= bound).all()
    res = out["regions"]
    assert res.initial_centroids.tolist() == gold["proto/picks"].tolist()
    z = np.load(case / "regions.npz")
    assert z.files == ["assignments"] and z["assignments"].dtype == np.int64
    assert np.array_equal(z["assignments"], gold["proto/assignments"])
    assert res.converged and (res.cluster_distance < 1e-2).all()
    assert sorted(out) == ["mean-flow", "regions"]

    res = P.homogeneous_regions(case, k=PC.PROTO_K, max_cluster_size=PC.PROTO_MAX_CLUSTER, chunk_frames=7, opener=h5fake.File,
                                device=DEV)
    z = np.load(case / "regions.npz")
    assert np.array_equal(z["assignments"], gold["proto/split/assignments"])
    assert np.array_equal(z["raw_assignments"], gold["proto/split/raw_assignments"])


def test_dataset_stats_on_the_golden_cases(tmp_path, gold):
    """stats.pickle of the two training cases at chunk size 4: min and max exact for u, p, k, nut and within the tolerance
    tests/test_sample_metrics_gpu.py grants the feature kernel's curl (rtol 2e-6, atol 2e-6 max |ref|) for the two norms;
    mean and std equal to the reference's float32 or the float32 next to it."""
    files = PC.install_stats_cases(tmp_path)["train"]
    stats = P.write_stats(tmp_path, chunk_frames=PC.STATS_CHUNK, opener=h5fake.File, list_cases=lambda d: sorted(files), device=DEV)
    assert pickle.loads((tmp_path / "stats.pickle").read_bytes()).keys() == stats.keys()
    assert list(stats) == list(P.STATS_FIELDS)
    loaded = OpenFOAMStats.from_file(tmp_path / "stats.pickle")
    failures = []
    for f in P.STATS_FIELDS:
        for key in ("min", "max", "mean", "std"):
            got, ref = stats[f][key], gold[f"stats/{f}/{key}"]
            assert got.dtype == np.float32 and got.shape == ref.shape, (f, key)
            assert np.array_equal(loaded.stats[f][key].numpy(), got)
            print(f"stats {f} {key}: got {got.tolist()} reference {ref.tolist()}")
            if key in ("min", "max"):
                ok = np.array_equal(got, ref) if f in ("u", "p", "k", "nut") else \
                    np.allclose(got, ref, rtol=2e-6, atol=2e-6 * float(np.abs(ref).max()))
            else:
                ok = R.adjacent_f32(got, ref.astype(np.float64)).all()
            if not ok:
                failures.append((f, key, got.tolist(), ref.tolist()))
    assert not failures, failures


def test_max_mean_tke_on_the_golden_case(tmp_path, gold):
    """5000 frames on a padded 30 x 6 x 7 grid, regenerated from the seed; the script's frame list range(2500, 5000, 10)."""
    case = PC.case_dir(tmp_path, "tke")
    PC.tke_case(case / "data.h5")
    value = P.max_mean_tke(case, chunk_frames=64, opener=h5fake.File, device=DEV)
    assert isinstance(value, float) and value == float(gold["tke/value"])
    assert float(np.load(case / "max-mean-tke.npy")) == value
