#!/usr/bin/env python3
"""Time WassersteinMetric on a paper-sized synthetic case and print one JSON line.

    python tools/ot_bench.py [--samples 8] [--regions 32] [--grid 192 48 48] [--cpu-n 1000 2000]

Case: an unpadded 192 x 48 x 48 interior (padded by one cell) with a box obstacle behind the inlet, 8 generated samples
against 8 data samples of random channel-like fields, 32 regions as a 4 x 4 x 2 block partition of the interior (about
13 800 cells each: the size of the reference's k-means regions).  Measured: the GPU time of the whole metric (features,
one batched auction of n*m*K jobs, the host outer problem), per job (that time over the jobs) and bids per job.  The CPU way of the
reference (a dense cost matrix per job, then an exact solver on one core) is timed with scipy's linear_sum_assignment
on a few jobs at the smaller sizes ``--cpu-n`` and extrapolated to the mean region size with the solver's n^3 scaling:
``cpu_*_extrapolated`` are NOT measurements.
"""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "generative-turbulence_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_case(grid, S, K, device, seed=0):
    from turbdiff_amd.data.ofles import BoundaryCondition, OpenFOAMData, OpenFOAMMetadata, OpenFOAMStats, Variable as V

    g = torch.Generator().manual_seed(seed)
    X, Y, Z = (c + 2 for c in grid)
    inside = torch.zeros((X, Y, Z), dtype=torch.bool)
    inside[1:-1, 1:-1, 1:-1] = True
    inside[20:28, Y // 2 - 6:Y // 2 + 6, 1:Z // 2] = False
    cell_idx = inside.flatten().nonzero().flatten()
    flat = torch.arange(X * Y * Z).view(X, Y, Z)
    boundaries = {"inlets": {"idx": flat[0].flatten()}, "outlets": {"idx": flat[-1].flatten()},
                  "walls": {"idx": torch.cat((flat[1:-1, 0].flatten(), flat[1:-1, -1].flatten()))}}
    bcs = {V.U: {"inlets": BoundaryCondition(BoundaryCondition.Type.FIXED_VALUE, torch.tensor([1.0, 0.0, 0.0]))}}
    meta = OpenFOAMMetadata(np.array([X, Y, Z]), cell_idx, boundaries, bcs, file=Path("bench-case/data.h5"),
                            h=np.array([0.01, 0.01, 0.01])).to(device)
    n = len(cell_idx)

    def fields(t):
        u = torch.randn(S, n, 3, generator=g) * 0.3 + torch.tensor([1.0, 0.0, 0.0])
        p = torch.randn(S, n, 1, generator=g) * 0.1
        return OpenFOAMData(meta, torch.full((S,), t), {V.U: u.to(device), V.P: p.to(device)})

    samples, data = fields(0.0), fields(1.0)
    ones = {"mean": torch.tensor(1.0), "std": torch.tensor(1.0), "min": torch.tensor(0.0), "max": torch.tensor(2.0)}
    stats = OpenFOAMStats({"norm(u)": ones, "norm(curl)": {**ones, "std": torch.tensor(100.0)},
                           "p": {k: v.reshape(1) for k, v in ones.items()}}).to(device)
    # regions: a 4 x 4 x 2 block partition of the interior (or the nearest split into K blocks along x)
    c = cell_idx
    x, y, z = c // (Y * Z) - 1, (c // Z) % Y - 1, c % Z - 1
    if K == 32:
        regions = (x * 4 // grid[0]) * 8 + (y * 4 // grid[1]) * 2 + (z * 2 // grid[2])
    else:
        regions = x * K // grid[0]
    return samples, data, stats, regions.numpy().astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--regions", type=int, default=32)
    ap.add_argument("--grid", type=int, nargs=3, default=(192, 48, 48))
    ap.add_argument("--cpu-n", type=int, nargs="*", default=(1000, 2000))
    ap.add_argument("--cpu-jobs", type=int, default=2)
    args = ap.parse_args()

    from turbdiff_amd.models.metrics import WassersteinMetric

    dev = torch.device("cuda:0")
    samples, data, stats, regions = build_case(tuple(args.grid), args.samples, args.regions, dev)
    counts = np.bincount(regions)
    side = {"bench-case": {"regions.npz": regions}}
    wm = WassersteinMetric(side=side)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = wm(samples, data, stats)["wasserstein"]
    torch.cuda.synchronize()
    t_metric = time.perf_counter() - t0
    jobs, res = wm.last_jobs, wm.last_result
    S = args.samples

    # the reference's way on one core: dense cost matrix + exact solve, at smaller n, extrapolated by n^3
    from scipy.optimize import linear_sum_assignment

    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    cpu = {}
    for n in args.cpu_n:
        ts = []
        for _ in range(args.cpu_jobs):
            a, b = rng.normal(size=(n, 8)).astype(np.float32), rng.normal(size=(n, 8)).astype(np.float32)
            t0 = time.perf_counter()
            M = ((a[:, None] - b[None]) ** 2).sum(-1)
            linear_sum_assignment(M)
            ts.append(time.perf_counter() - t0)
        cpu[n] = float(np.mean(ts))
    n_mean = float(counts[counts > 0].mean())
    n_big = max(cpu)
    per_job_cpu = cpu[n_big] * (n_mean / n_big) ** 3
    print(json.dumps({
        "case": {"interior": list(args.grid), "samples": S, "data_samples": S, "regions": int((counts > 0).sum()),
                 "cells": int(len(regions)), "mean_region": round(n_mean, 1), "jobs": int(len(jobs))},
        "gpu_wasserstein_metric_s": round(t_metric, 3), "gpu_per_job_ms": round(1e3 * t_metric / len(jobs), 3),
        "bids_per_job_mean": float(res.bids.mean()), "bids_per_job_max": int(res.bids.max()),
        "bids_per_person_mean": float((res.bids / counts[jobs[:, 2]]).mean()),
        "max_gap_over_eps": float((res.gap / res.eps_final).max()), "wasserstein": float(w),
        "cpu_lsa_measured_s": {str(k): round(v, 3) for k, v in cpu.items()},
        "cpu_per_job_s_extrapolated": round(per_job_cpu, 2),
        "cpu_total_s_extrapolated_one_core": round(per_job_cpu * len(jobs), 1),
    }))


if __name__ == "__main__":
    main()
