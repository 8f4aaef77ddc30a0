#!/usr/bin/env python3
"""Generate tests/golden/sample_metrics.npz by running the *reference's* finite differences and sample metrics (build
container only).

Imports the unmodified ``turbdiff.metrics`` and ``turbdiff.models.metrics`` with the usual stand-ins for packages that
are not installed, two of them replaced: ``ot.emd2`` records every matrix it is handed and returns its exact optimum by
``scipy.optimize.linear_sum_assignment`` (all matrices here are square), and ``deadpool.Deadpool`` becomes a synchronous
executor whose ``submit`` returns a completed future.  Stores inputs and outputs as numbers only.

    python tests/golden/make_golden_sample_metrics.py

Contents: ``fd/<tag>/*`` curl, divergence, vector_gradient and enstrophy on odd grids with anisotropic h;
``case/*`` a small synthetic channel case (padded 34 x 8 x 9 grid with a box obstacle, 3 samples against 3 data samples,
8 regions) with ``WassersteinMetric.features`` of both sets, the regional distance matrices of ``WassersteinTKE``, the
reference's inner W2^2 for every (i, j, k), a few of its inner matrices with their optima, and all three metrics' outputs.
"""
import sys
from concurrent.futures import Future
from pathlib import Path

import numpy as np
import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden import REF, install_stubs, to_np  # noqa: E402

RECORDED = []


def emd2_exact(a, b, M):
    from scipy.optimize import linear_sum_assignment

    M = np.asarray(M, dtype=np.float64)
    r, c = linear_sum_assignment(M)
    value = float(M[r, c].sum() / M.shape[0])
    RECORDED.append((M.copy(), value))
    return value


class SyncPool:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def submit(self, fn, *args, **kwargs):
        f = Future()
        f.set_result(fn(*args, **kwargs))
        return f


def main():
    install_stubs()
    sys.modules["ot"].emd2 = emd2_exact
    sys.modules["deadpool"].Deadpool = SyncPool
    sys.path.insert(0, str(REF))
    import turbdiff.metrics as F
    import turbdiff.models.metrics as M
    from turbdiff.data.ofles import BoundaryCondition, OpenFOAMData, OpenFOAMMetadata, OpenFOAMStats
    from turbdiff.data.ofles import Variable as V

    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(20261016)
    out = {}
    for tag, shape, h in (("a", (2, 3, 9, 7, 11), (0.1, 0.23, 0.37)), ("b", (1, 3, 13, 6, 5), (1.5, 0.5, 0.75))):
        u = torch.randn(*shape, generator=g)
        out[f"fd/{tag}/u"], out[f"fd/{tag}/h"] = to_np(u), np.array(h)
        out[f"fd/{tag}/curl"] = to_np(F.curl(u, h))
        out[f"fd/{tag}/divergence"] = to_np(F.divergence(u, h))
        out[f"fd/{tag}/vector_gradient"] = to_np(F.vector_gradient(u, h))
        out[f"fd/{tag}/enstrophy"] = to_np(F.enstrophy(u, h))

    # a small channel case: padded grid, box obstacle, inlet / wall / outlet boundaries
    X, Y, Z = grid = (34, 8, 9)
    inside = torch.zeros(grid, dtype=torch.bool)
    inside[1:-1, 1:-1, 1:-1] = True
    inside[5:9, 3:6, 1:5] = False
    cell_idx = inside.flatten().nonzero().flatten()
    flat = torch.arange(X * Y * Z).view(grid)
    boundaries = {"inlets": {"idx": flat[0, 1:-1, 1:-1].flatten()}, "outlets": {"idx": flat[-1, 1:-1, 1:-1].flatten()},
                  "walls": {"idx": torch.cat((flat[1:-1, 0].flatten(), flat[1:-1, -1].flatten()))}}
    FV, ZG = BoundaryCondition.Type.FIXED_VALUE, BoundaryCondition.Type.ZERO_GRADIENT
    bcs = {V.U: {"inlets": BoundaryCondition(FV, torch.tensor([1.0, 0.0, 0.0])), "walls": BoundaryCondition(FV, torch.zeros(3)),
                 "outlets": BoundaryCondition(ZG, None)},
           V.P: {"inlets": BoundaryCondition(ZG, None), "walls": BoundaryCondition(ZG, None),
                 "outlets": BoundaryCondition(FV, torch.zeros(1))}}
    h = np.array([0.05, 0.07, 0.06])
    meta = OpenFOAMMetadata(Path("/nonexistent/case-g/data.h5"), 1e-5, h, np.array(grid), cell_idx, boundaries, bcs, [])
    n_cells, S = len(cell_idx), 3

    def fields():
        u = torch.randn(S, n_cells, 3, generator=g) * 0.3 + torch.tensor([1.0, 0.0, 0.0])
        p = torch.randn(S, n_cells, 1, generator=g) * 0.1
        return {V.U: u, V.P: p}

    samples = OpenFOAMData(meta, torch.zeros(S), fields())
    data = OpenFOAMData(meta, torch.ones(S), fields())
    rec = lambda t: {"mean": t.mean(0), "std": t.std(0), "min": t.amin(0), "max": t.amax(0)}
    nrm = lambda t: {k: v.reshape(()) for k, v in rec(t.norm(dim=-1, keepdim=True)).items()}
    allu = torch.cat([samples.samples[V.U], data.samples[V.U]]).reshape(-1, 3)
    allp = torch.cat([samples.samples[V.P], data.samples[V.P]]).reshape(-1, 1)
    curl_cells = M.select_cells(F.curl(data.grid_embedding((V.U,)), h), meta.unpadded_cell_idx).transpose(-1, -2)
    stats_raw = {"u": rec(allu), "p": rec(allp), "norm(u)": nrm(allu), "norm(p)": nrm(allp),
                 "norm(curl)": nrm(curl_cells.reshape(-1, 3))}
    stats = OpenFOAMStats(stats_raw)
    for v, st in stats_raw.items():
        for k, t in st.items():
            out[f"case/stats/{v}/{k}"] = to_np(t)
    out["case/grid"], out["case/h"], out["case/cell_idx"] = np.array(grid), h, to_np(cell_idx)
    for name, d in (("samples", samples), ("data", data)):
        out[f"case/{name}/u"], out[f"case/{name}/p"] = to_np(d.samples[V.U]), to_np(d.samples[V.P])
    out["case/unpadded_cell_idx"] = to_np(meta.unpadded_cell_idx)

    wm = M.WassersteinMetric()
    out["case/features/samples"] = to_np(wm.features(samples, stats))
    out["case/features/data"] = to_np(wm.features(data, stats))

    K = 8
    assignments = (torch.arange(n_cells) * K // n_cells).numpy()  # contiguous blocks along the channel
    perm = torch.randperm(n_cells, generator=g)[: n_cells // 5].numpy()
    assignments[perm] = torch.randint(0, K, (len(perm),), generator=g).numpy()
    out["case/regions"] = assignments
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        case_dir = Path(tmp) / "case-g"
        case_dir.mkdir()
        np.savez(case_dir / "regions.npz", assignments=assignments)
        np.save(case_dir / "max-mean-tke.npy", np.float64(27.5))
        meta.file = case_dir / "data.h5"
        RECORDED.clear()
        w = wm(samples, data, stats)
        inner = list(RECORDED)
        RECORDED.clear()
        out["case/wasserstein"] = to_np(w["wasserstein"])
        # the inner problems, in the reference's (k, i, j) submission order
        D = np.zeros((S, S, K))
        t = 0
        for k in range(K):
            for i in range(S):
                for j in range(S):
                    D[i, j, k] = inner[t][1]
                    t += 1
        out["case/inner_w2sq"] = D
        for t in (0, 40, 71):
            out[f"case/inner/{t}/M"] = inner[t][0].astype(np.float32)
            out[f"case/inner/{t}/opt"] = np.array(inner[t][1])
        out["case/outer/M"] = inner[-1][0]

        tke = M.WassersteinTKE()
        RECORDED.clear()
        vals = tke(samples, data, stats)
        for name, v in vals.items():
            out[f"case/{name}"] = to_np(v)
        out["case/tke_outer"] = np.stack([m for m, _ in RECORDED])  # D^2 of front, middle, back, combined
        mm = M.MaxMeanTKEPositionMetric()(samples, data, stats)
        out["case/max-mean-tke"] = np.float64(27.5)
        out["case/max-mean-tke-pos"] = to_np(mm["max-mean-tke-pos"])
    np.savez_compressed(OUT / "sample_metrics.npz", **out)
    size = (OUT / "sample_metrics.npz").stat().st_size
    print(f"wrote {OUT / 'sample_metrics.npz'} ({len(out)} arrays, {size} bytes)")


if __name__ == "__main__":
    main()
