"""Sample-quality metrics on the MI355X: the finite-difference kernel, the fused Wasserstein features, the batched
auction against exact linear assignment, and the three metrics of the reference against its golden values."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def exact_w2sq(a: np.ndarray, b: np.ndarray) -> float:
    from scipy.optimize import linear_sum_assignment

    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    M = (((a32[:, None, :] - b32[None, :, :]) ** 2).sum(-1)).astype(np.float64)
    r, c = linear_sum_assignment(M)
    return float(M[r, c].sum() / len(a))


def run_pairs(pairs, **kw):
    """One auction launch over a list of (a (n, 8), b (n, 8)) problems, each its own region of sample 0."""
    from turbdiff_amd import ot

    n_tot = sum(len(a) for a, _ in pairs)
    fa = torch.from_numpy(np.concatenate([a for a, _ in pairs]).astype(np.float32))[None].to(DEV)
    fb = torch.from_numpy(np.concatenate([b for _, b in pairs]).astype(np.float32))[None].to(DEV)
    offsets = np.concatenate(([0], np.cumsum([len(a) for a, _ in pairs])))
    jobs = [(0, 0, k) for k in range(len(pairs))]
    return ot.auction_w2(fa, fb, np.arange(n_tot), offsets, jobs, **kw)


def check_exact(res, pairs, rel=1e-6):
    for k, (a, b) in enumerate(pairs):
        ex = exact_w2sq(a, b)
        eps = res.eps_final[k]
        assert res.status[k] == 0
        assert eps <= 1e-6 * max(ex, 1e-30) or ex == 0 or eps <= 1e-6 * np.mean(((a - b.mean(0)) ** 2).sum(-1))
        # primal within eps_final (+ fp32 rounding of the costs) above the exact optimum; certificate 0 <= gap <= eps_final
        tol = eps + rel * ex + 1e-12
        assert abs(res.primal[k] - ex) <= tol, (k, len(a), res.primal[k], ex, eps)
        assert -1e-9 * max(ex, 1.0) <= res.gap[k] <= eps * (1 + 1e-9) + 1e-12, (k, res.gap[k], eps)


@pytest.mark.parametrize("n", [1, 2, 17, 64, 500, 2000])
def test_auction_matches_linear_sum_assignment(n):
    rng = np.random.default_rng(n)
    pairs = [(rng.normal(size=(n, 8)), rng.normal(size=(n, 8)) + 0.3) for _ in range(2)]
    for a, b in pairs:
        a[:, 7] = b[:, 7] = 0.0
    check_exact(run_pairs(pairs), pairs)


def test_auction_adversarial_cases():
    rng = np.random.default_rng(5)
    same = rng.normal(size=(300, 8))
    dup = np.repeat(rng.normal(size=(10, 8)), 30, axis=0)
    lattice_a = rng.integers(0, 3, size=(256, 8)).astype(np.float64)
    lattice_b = rng.integers(0, 3, size=(256, 8)).astype(np.float64)
    pairs = [(same, same.copy()), (dup, dup[rng.permutation(300)] + 0.0), (dup, rng.normal(size=(300, 8))),
             (lattice_a, lattice_b), (np.zeros((40, 8)), np.zeros((40, 8)))]
    for scale in (1e-3, 1.0, 1e3):
        pairs.append((rng.normal(size=(200, 8)) * scale, rng.normal(size=(200, 8)) * scale))
    pairs += [(rng.normal(size=(n, 8)), rng.normal(size=(n, 8))) for n in (3, 1, 700, 33, 128)]  # mixed sizes
    res = run_pairs(pairs)
    assert res.primal[0] <= res.eps_final[0] and res.primal[1] <= res.eps_final[1]
    assert res.primal[4] == 0.0
    check_exact(res, pairs)


def test_auction_certificate_at_full_region_size():
    """n ~ 14 000 (a full region of the paper's grid): no exact CPU solve, the device certificate alone."""
    rng = np.random.default_rng(14)
    pairs = [(rng.normal(size=(14000, 8)).astype(np.float32), (rng.normal(size=(14000, 8)) * 1.1 + 0.2).astype(np.float32))
             for _ in range(2)]
    res = run_pairs(pairs)
    assert (res.status == 0).all()
    assert (res.gap >= -1e-9 * res.primal).all() and (res.gap <= res.eps_final * (1 + 1e-9)).all()
    assert (res.eps_final <= 1e-6 * res.primal).all()


def test_auction_bit_reproducible_and_slots_independent():
    rng = np.random.default_rng(3)
    pairs = [(rng.normal(size=(n, 8)), rng.normal(size=(n, 8))) for n in (400, 90, 1000)]
    r1, r2, r3 = run_pairs(pairs), run_pairs(pairs), run_pairs(pairs, slots=1)
    for a, b in ((r1, r2), (r1, r3)):
        assert np.array_equal(a.primal.view(np.int64), b.primal.view(np.int64))
        assert np.array_equal(a.dual.view(np.int64), b.dual.view(np.int64))
        assert np.array_equal(a.bids, b.bids)


def test_auction_cap_returns_error_status():
    """A deliberately tiny round cap: the job comes back with its status set (and raises by default), nothing hangs."""
    rng = np.random.default_rng(9)
    pairs = [(rng.normal(size=(300, 8)), rng.normal(size=(300, 8))), (rng.normal(size=(4, 8)) * 0, np.zeros((4, 8)))]
    res = run_pairs(pairs, max_rounds=2, check=False)
    assert res.status[0] == 1 and np.isnan(res.primal[0])
    assert res.status[1] == 0
    with pytest.raises(RuntimeError, match="round cap"):
        run_pairs(pairs, max_rounds=2)
    res = run_pairs(pairs, max_bids=50, check=False)
    assert res.status[0] == 2


def test_auction_weight_zero_region_and_bad_inputs():
    from turbdiff_amd import ot

    rng = np.random.default_rng(1)
    f = torch.from_numpy(rng.normal(size=(2, 10, 8)).astype(np.float32)).to(DEV)
    res = ot.auction_w2(f, f, np.arange(10), [0, 4, 4, 10], [(0, 1, 0), (1, 0, 1), (0, 1, 2)])
    assert res.primal[1] == 0.0 and res.status[1] == 0
    with pytest.raises(RuntimeError, match="out of range"):
        ot.auction_w2(f, f, np.arange(10) + 1, [0, 10], [(0, 0, 0)])
    with pytest.raises(RuntimeError, match="out of range"):
        ot.auction_w2(f, f, np.arange(10), [0, 10], [(2, 0, 0)])
    bad = f.clone()
    bad[0, 3, 2] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        ot.auction_w2(bad, f, np.arange(10), [0, 10], [(0, 0, 0)])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_finite_differences_against_reference(golden, tag):
    from turbdiff_amd import metrics as F

    g = golden("sample_metrics")
    u, h = g[f"fd/{tag}/u"].to(DEV), tuple(g[f"fd/{tag}/h"].tolist())
    for name, fn in (("curl", F.curl), ("divergence", F.divergence), ("enstrophy", F.enstrophy),
                     ("vector_gradient", F.vector_gradient)):
        got, ref = fn(u, h).cpu(), g[f"fd/{tag}/{name}"]
        assert got.shape == ref.shape, name
        torch.testing.assert_close(got, ref, rtol=2e-6, atol=2e-6 * float(ref.abs().max()), msg=name)


def _case(g):
    from pathlib import Path

    from turbdiff_amd.data.ofles import BoundaryCondition, OpenFOAMData, OpenFOAMMetadata, OpenFOAMStats, Variable as V

    X, Y, Z = (int(v) for v in g["case/grid"])
    flat = torch.arange(X * Y * Z).view(X, Y, Z)
    boundaries = {"inlets": {"idx": flat[0, 1:-1, 1:-1].flatten()}, "outlets": {"idx": flat[-1, 1:-1, 1:-1].flatten()},
                  "walls": {"idx": torch.cat((flat[1:-1, 0].flatten(), flat[1:-1, -1].flatten()))}}
    FV, ZG = BoundaryCondition.Type.FIXED_VALUE, BoundaryCondition.Type.ZERO_GRADIENT
    bcs = {V.U: {"inlets": BoundaryCondition(FV, torch.tensor([1.0, 0.0, 0.0])), "walls": BoundaryCondition(FV, torch.zeros(3)),
                 "outlets": BoundaryCondition(ZG, None)},
           V.P: {"inlets": BoundaryCondition(ZG, None), "walls": BoundaryCondition(ZG, None),
                 "outlets": BoundaryCondition(FV, torch.zeros(1))}}
    meta = OpenFOAMMetadata(np.array([X, Y, Z]), g["case/cell_idx"], boundaries, bcs, file=Path("case-g/data.h5"),
                            h=g["case/h"].numpy())
    stats = OpenFOAMStats({v: {k: g[f"case/stats/{v}/{k}"] for k in ("mean", "std", "min", "max")}
                           for v in ("u", "p", "norm(u)", "norm(p)", "norm(curl)")})
    mk = lambda name, t: OpenFOAMData(meta.to(DEV), torch.full((3,), t, device=DEV),
                                      {V.U: g[f"case/{name}/u"].to(DEV), V.P: g[f"case/{name}/p"].to(DEV)})
    side = {"case-g": {"regions.npz": g["case/regions"].numpy(), "max-mean-tke.npy": float(g["case/max-mean-tke"])}}
    return mk("samples", 0.0), mk("data", 1.0), stats.to(DEV), side, meta


def test_wasserstein_features_against_reference(golden):
    from turbdiff_amd.models.metrics import WassersteinMetric

    g = golden("sample_metrics")
    samples, data, stats, _, _ = _case(g)
    for name, d in (("samples", samples), ("data", data)):
        got = WassersteinMetric().features(d, stats).cpu()
        ref = g[f"case/features/{name}"]
        assert got.shape == (*ref.shape[:2], 8) and torch.all(got[..., 7] == 0)
        torch.testing.assert_close(got[..., :7], ref, rtol=2e-6, atol=2e-6 * float(ref.abs().max()))


def test_metrics_against_reference(golden):
    from turbdiff_amd.models.metrics import MaxMeanTKEPositionMetric, WassersteinMetric, WassersteinTKE

    g = golden("sample_metrics")
    samples, data, stats, side, _ = _case(g)
    wm = WassersteinMetric(side=side)
    D = wm.region_distances(samples, data, stats, side["case-g"]["regions.npz"])
    np.testing.assert_allclose(D, g["case/inner_w2sq"].numpy(), rtol=2e-6)
    assert float(wm(samples, data, stats)["wasserstein"]) == pytest.approx(float(g["case/wasserstein"]), rel=2e-6)
    tke = WassersteinTKE(side=side).to(DEV)(samples, data, stats)
    for name in ("tke-front", "tke-middle", "tke-back", "tke"):
        assert float(tke[name]) == pytest.approx(float(g[f"case/{name}"]), rel=2e-4), name
    mm = MaxMeanTKEPositionMetric(side=side)(samples, data, stats)
    assert float(mm["max-mean-tke-pos"]) == pytest.approx(float(g["case/max-mean-tke-pos"]), rel=1e-6)
    assert WassersteinMetric()(samples, data, stats) == {}  # no regions anywhere: the reference's warning and {}


def test_collection_compute_against_reference(golden):
    from turbdiff_amd.data.ofles import InMemoryRepository, Variable as V
    from turbdiff_amd.models.metrics import (MaxMeanTKEPositionMetric, SampleMetricsCollection, SampleStore, WassersteinMetric,
                                             WassersteinTKE)

    g = golden("sample_metrics")
    samples, data, stats, side, meta = _case(g)
    store = SampleStore(None, (V.U, V.P))
    store.add_cells({V.U: samples.samples[V.U], V.P: samples.samples[V.P]}, meta)
    # a case whose second half holds exactly the golden data samples (linspace(3, 5, 3) = 3, 4, 5)
    T = 6
    u = torch.zeros(T, *g["case/data/u"].shape[1:])
    p = torch.zeros(T, *g["case/data/p"].shape[1:])
    for t, s in zip((3, 4, 5), range(3)):
        u[t], p[t] = g["case/data/u"][s], g["case/data/p"][s]
    repo = InMemoryRepository([(meta, np.arange(T), {V.U: u, V.P: p})])
    coll = SampleMetricsCollection("val", None, [WassersteinTKE(side=side), WassersteinMetric(side=side),
                                                 MaxMeanTKEPositionMetric(side=side)], repository=lambda name: repo).to(DEV)
    vals = coll.compute(store, stats, DEV)
    assert float(vals["val/case-g/wasserstein"]) == pytest.approx(float(g["case/wasserstein"]), rel=2e-6)
    assert float(vals["val/wasserstein"]) == float(vals["val/case-g/wasserstein"])
    assert float(vals["val/tke"]) == pytest.approx(float(g["case/tke"]), rel=2e-4)
    assert float(vals["val/max-mean-tke-pos"]) == pytest.approx(float(g["case/max-mean-tke-pos"]), rel=1e-6)


def test_eval_ckpt_prints_sample_metrics(tmp_path):
    """``eval_ckpt --sample-metrics --expensive-metrics --synthetic 2`` prints the reference's metric keys beside the
    unchanged ``val/log_tke_l2``."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    from turbdiff_amd.training import DiffusionTrainer

    root = Path(__file__).resolve().parent.parent
    run = json.loads((root / "tests" / "golden" / "task_configs.json").read_text())["shipped"]["run_config"]
    run["model"].update(dim=8, timesteps=10, eval_batch_size=2)
    run["matmul_precision"] = "highest"
    torch.manual_seed(3)
    src = DiffusionTrainer.from_config(run, max_train_steps=1)
    torch.save({"config": run, "state_dict": src.state_dict()}, tmp_path / "model.ckpt")
    out = subprocess.run([sys.executable, str(root / "tools" / "eval_ckpt.py"), str(tmp_path / "model.ckpt"), str(tmp_path / "s.npz"),
                          "--synthetic", "2", "--start-from", "2", "--sample-metrics", "--expensive-metrics",
                          "model.eval_batch_size=2"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    keys = {line.split(":")[0] for line in out.stdout.splitlines() if ": " in line}
    for name in ("tke-front", "tke-middle", "tke-back", "tke", "max-mean-tke-pos", "wasserstein"):
        assert f"val/{name}" in keys and f"val/case-00/{name}" in keys and f"val/case-01/{name}" in keys, (name, sorted(keys))
    assert "val/log_tke_l2" in keys
