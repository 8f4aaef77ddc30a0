"""Host side of the sample-quality metrics: the exact W2 of the small outer problems, the lcm expansion, and the key
naming / mean over cases of SampleMetricsCollection with the device parts faked.  No GPU needed."""

import itertools
import math

import numpy as np
import pytest
import torch


def brute_force_emd2(M):
    """Uniform n x m transport by brute force over permutations of the lcm expansion (tiny n, m only)."""
    n, m = M.shape
    k = n * m // math.gcd(n, m)
    big = np.repeat(np.repeat(M, k // n, axis=0), k // m, axis=1)
    return min(big[np.arange(k), list(p)].sum() for p in itertools.permutations(range(k))) / k


def linprog_emd2(M):
    from scipy.optimize import linprog

    n, m = M.shape
    A = np.zeros((n + m, n * m))
    for i in range(n):
        A[i, i * m:(i + 1) * m] = 1
    for j in range(m):
        A[n + j, j::m] = 1
    b = np.concatenate((np.full(n, 1 / n), np.full(m, 1 / m)))
    res = linprog(M.reshape(-1), A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    assert res.status == 0
    return res.fun


@pytest.mark.parametrize("n,m", [(1, 1), (2, 2), (5, 5), (7, 7), (2, 3), (3, 2), (2, 4), (4, 6), (1, 5)])
def test_exact_emd2_matches_brute_force(n, m):
    from turbdiff_amd.ot import exact_emd2

    rng = np.random.default_rng(n * 31 + m)
    for _ in range(3):
        M = rng.random((n, m)) ** 2
        if n * m // math.gcd(n, m) <= 7:
            assert exact_emd2(M) == pytest.approx(brute_force_emd2(M), rel=1e-12, abs=1e-15)
        assert exact_emd2(M) == pytest.approx(linprog_emd2(M), rel=1e-7, abs=1e-12)


@pytest.mark.parametrize("n,m", [(8, 8), (6, 9), (10, 4), (12, 7)])
def test_exact_emd2_matches_linprog(n, m):
    from turbdiff_amd.ot import exact_emd2

    rng = np.random.default_rng(7 + n * m)
    M = rng.normal(size=(n, m)) ** 2
    assert exact_emd2(M) == pytest.approx(linprog_emd2(M), rel=1e-7, abs=1e-12)


def test_lcm_expansion():
    from turbdiff_amd.ot import lcm_expand

    M = np.arange(6.0).reshape(2, 3)
    big = lcm_expand(M)
    assert big.shape == (6, 6)
    assert np.array_equal(big[0], [0, 0, 1, 1, 2, 2]) and np.array_equal(big[3], [3, 3, 4, 4, 5, 5])
    assert np.array_equal(big[0], big[2]) and np.array_equal(big[3], big[5])
    assert lcm_expand(np.ones((4, 4))).shape == (4, 4)


def test_wasserstein2_squared_of_distances():
    from turbdiff_amd.models.metrics import wasserstein2_squared
    from turbdiff_amd.ot import exact_emd2

    D = np.array([[0.0, 3.0], [4.0, 1.0]])
    assert wasserstein2_squared(D) == pytest.approx(0.5)
    assert wasserstein2_squared(D) == exact_emd2(D**2)


def test_reference_outer_problems_reproduced(golden):
    """The reference handed these D^2 matrices to ot.emd2; the exact host solver returns the values it reported."""
    from turbdiff_amd.ot import exact_emd2

    g = golden("sample_metrics")
    outer = g["case/tke_outer"].numpy()
    names = ["tke-front", "tke-middle", "tke-back", "tke"]
    for M, name in zip(outer, names):
        assert math.sqrt(exact_emd2(M)) == pytest.approx(float(g[f"case/{name}"]), rel=1e-12)
    for t in (0, 40, 71):
        assert exact_emd2(g[f"case/inner/{t}/M"].numpy()) == pytest.approx(float(g[f"case/inner/{t}/opt"]), rel=1e-6)


class _FakeMetric(torch.nn.Module):
    def __init__(self, name, expensive, values):
        super().__init__()
        self.name, self.expensive, self.values = name, expensive, values

    def is_expensive(self):
        return self.expensive

    def forward(self, samples, data, stats):
        return {self.name: torch.tensor(self.values[data.metadata.case_name])} if data.metadata.case_name in self.values else {}


def _store_and_repos(case_names, n_times=10, n_samples=3):
    from pathlib import Path

    from turbdiff_amd.data.ofles import InMemoryRepository, OpenFOAMMetadata, Variable
    from turbdiff_amd.models.metrics import SampleStore

    store = SampleStore(None, (Variable.U, Variable.P))
    repos = {}
    for c, name in enumerate(case_names):
        meta = OpenFOAMMetadata(np.array([5, 5, 5]), torch.arange(27), {}, {}, file=Path(f"{name}/data.h5"))
        u = torch.arange(n_times, dtype=torch.float32)[:, None, None].expand(n_times, 27, 3).clone()
        p = torch.zeros(n_times, 27, 1)
        repos[name] = InMemoryRepository([(meta, np.arange(n_times), {Variable.U: u, Variable.P: p})])
        store.add_cells({Variable.U: torch.randn(n_samples, 27, 3), Variable.P: torch.randn(n_samples, 27, 1)}, meta)
    return store, repos


def test_collection_key_names_and_case_mean():
    from turbdiff_amd.data.ofles import OpenFOAMStats
    from turbdiff_amd.models.metrics import SampleMetricsCollection

    store, repos = _store_and_repos(["case-a", "case-b"])
    seen = []

    class Spy(_FakeMetric):
        def forward(self, samples, data, stats):
            seen.append((data.metadata.case_name, data.t.tolist(), samples.n_samples))
            return super().forward(samples, data, stats)

    metrics = [Spy("tke", False, {"case-a": 1.0, "case-b": 3.0}),
               _FakeMetric("wasserstein", True, {"case-a": 2.0}),
               _FakeMetric("max-mean-tke-pos", False, {"case-b": 5.0})]
    coll = SampleMetricsCollection("val", None, metrics, repository=lambda name: repos[name])
    stats = OpenFOAMStats({})
    vals = coll.compute(store, stats, torch.device("cpu"))
    assert sorted(vals) == sorted(["val/case-a/tke", "val/case-b/tke", "val/case-a/wasserstein", "val/case-b/max-mean-tke-pos",
                                   "val/tke", "val/wasserstein", "val/max-mean-tke-pos"])
    assert float(vals["val/tke"]) == 2.0 and float(vals["val/wasserstein"]) == 2.0
    assert float(vals["val/max-mean-tke-pos"]) == 5.0
    # data samples: linspace over the second half of the case, as many as there are samples
    assert seen[0] == ("case-a", [5.0, 7.0, 9.0], 3)

    cheap = coll.compute(store, stats, torch.device("cpu"), expensive_metrics=False)
    assert "val/wasserstein" not in cheap and "val/case-a/wasserstein" not in cheap and "val/tke" in cheap


def test_metric_modules_and_state_dict_keys():
    from turbdiff_amd.models.metrics import MaxMeanTKEPositionMetric, WassersteinMetric, WassersteinTKE
    from turbdiff_amd.training import _metric_placeholders

    assert not WassersteinTKE().is_expensive() and WassersteinMetric().is_expensive()
    assert not MaxMeanTKEPositionMetric().is_expensive()
    coll = _metric_placeholders()
    assert [type(m).__name__ for m in coll.metrics] == ["WassersteinTKE", "WassersteinMetric", "MaxMeanTKEPositionMetric"]
    assert sorted(coll.state_dict()) == ["metrics.0.distance.legendre_nodes", "metrics.0.distance.legendre_weights",
                                         "metrics.0.distance.tke_spectrum.p", "metrics.0.distance.tke_spectrum.w"]


def test_metadata_unpadded_cell_idx_and_two_dimensional(golden):
    from turbdiff_amd.data.ofles import OpenFOAMMetadata

    g = golden("sample_metrics")
    meta = OpenFOAMMetadata(g["case/grid"].numpy(), g["case/cell_idx"], {}, {})
    assert torch.equal(meta.unpadded_cell_idx, g["case/unpadded_cell_idx"])
    assert not meta.two_dimensional
    assert OpenFOAMMetadata(np.array([10, 3, 8]), torch.arange(3), {}, {}).two_dimensional


def test_auction_refuses_cpu_tensors():
    from turbdiff_amd import ot

    f = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ot.auction_w2(f, f, [0, 1, 2, 3], [0, 4], [(0, 0, 0)])
