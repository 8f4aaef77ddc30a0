#!/usr/bin/env python3
"""Time the case-preparation kernels at the size of a real case and print a small report.

    python tools/prepare_bench.py [--cells 485000] [-k 32] [--frames 10] [--reps 200] [--rounds 3]

Measured on the GPU with device events, after a warm-up, each figure over ``--reps`` back-to-back launches:

  * one Lloyd pass of the k-means (``tdx_w2n_assign`` with sums + ``tdx_w2n_reduce``) at ``--cells`` cells and ``-k``
    centroids, alternating in one process with a numpy evaluation of the same distances on the host (``host_pass``: (k, n)
    float64 arrays built component by component, then argmin; numpy's elementwise work runs on one thread);
  * ``tdx_moments_update`` on chunks of ``--frames`` frames of u (n = 3 * cells columns): the bytes the algorithm must move,
    4 T n in and 32 n of state in and out, over the kernel time, and the chunk's 4 T n bytes alone over the same time (the
    state is the same 16 n bytes on every launch, as in the product, and fits the memory-side cache: only the chunk is
    certain to come from HBM);
  * ``tdx_field_stats`` on the (frames * cells, 8) feature matrix with both norms, and on a one-column field: 4 rows C bytes
    over the kernel time.

The streaming kernels read a different chunk on every launch (the chunks rotate through more than the 256 MiB of the
memory-side cache), as they do when chunks arrive from a file.  The rates are set beside the 6.3 TB/s a plain device copy
reaches on this chip (profiles/r11_hbm_write_probe.txt).  Nothing here reads a disk: the end-to-end time of
preparing a real case is bounded by reading data.h5 and is not measured.
"""

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "generative-turbulence_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_ROOF = 6.3e12  # bytes / s of a plain device copy


def host_pass(mean, var, cmean, cvar):
    """Nearest centroid of every cell on the host: d^2 = |cm - m|^2 + sum cvar + sum var - 2 sum sqrt(cvar var), gathered
    one component at a time into a (k, n) float64 array; the cell's variance sum is the float32 one, as in the kernel."""
    cell_var = ((var[:, 0] + var[:, 1]) + var[:, 2]).astype(np.float64)
    d2 = ((cvar[:, 0] + cvar[:, 1]) + cvar[:, 2])[:, None] + cell_var[None, :]
    for e in range(3):
        m, v = mean[:, e].astype(np.float64), var[:, e].astype(np.float64)
        diff = cmean[:, e, None] - m[None, :]
        d2 += diff * diff - 2.0 * np.sqrt(cvar[:, e, None] * v[None, :])
    return np.maximum(d2, 0.0).argmin(axis=0)


def timed(fn, reps):
    """ms per call over `reps` back-to-back calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(reps):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=485_000)
    ap.add_argument("-k", type=int, default=32)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_bench.py measures on the GPU; none is visible")
    from turbdiff_amd import _lib as L
    from turbdiff_amd.data import prepare as P

    dev = torch.device("cuda:0")
    n, k, T = args.cells, args.k, args.frames
    rng = np.random.default_rng(0)
    mean_h = rng.standard_normal((n, 3)).astype(np.float32)
    var_h = rng.uniform(0.05, 1.5, (n, 3)).astype(np.float32)
    cmean, cvar = rng.standard_normal((k, 3)), rng.uniform(0.05, 1.5, (k, 3))
    mean_d, var_d = torch.from_numpy(mean_h).to(dev), torch.from_numpy(var_h).to(dev)
    print(f"device {torch.cuda.get_device_name(0)}, library {L.load().tdx_arch().decode()}, cells {n}, k {k}, frames per chunk {T}, "
          f"{args.reps} launches per figure, {args.rounds} alternating rounds")

    # ---- one Lloyd pass, device and host alternating
    idx, _, table = P.w2n_assign(mean_d, var_d, cmean, cvar, sums=True)  # warm-up, and the check that both sides agree
    want = host_pass(mean_h, var_h, cmean, cvar)
    agree = float((idx.cpu().numpy() == want).mean())
    print(f"lloyd pass: device and host labels agree on {agree:.6f} of the cells; counts sum {int(table[:, 0].sum())}")
    cm_d, cv_d = torch.from_numpy(cmean).to(dev), torch.from_numpy(cvar).to(dev)
    blocks = L.query("tdx_w2n_blocks", n)
    partials = torch.empty((blocks, k, 7), dtype=torch.float64, device=dev)
    idx_d = torch.empty(n, dtype=torch.int32, device=dev)
    dist_d = torch.empty(n, dtype=torch.float64, device=dev)
    table_d = torch.empty((k, 7), dtype=torch.float64, device=dev)

    def lloyd(_):
        L.call("tdx_w2n_assign", L.ptr(mean_d), L.ptr(var_d), n, L.ptr(cm_d), L.ptr(cv_d), k, L.ptr(idx_d), L.ptr(dist_d),
               L.ptr(partials), L.stream())
        L.call("tdx_w2n_reduce", L.ptr(partials), blocks, k, L.ptr(table_d), L.stream())

    def assign_only(_):
        L.call("tdx_w2n_assign", L.ptr(mean_d), L.ptr(var_d), n, L.ptr(cm_d), L.ptr(cv_d), k, L.ptr(idx_d), L.ptr(dist_d),
               None, L.stream())

    timed(lloyd, 3)
    for r in range(args.rounds):
        ms = timed(lloyd, args.reps)
        ms_a = timed(assign_only, args.reps)
        t0 = time.perf_counter()
        host_pass(mean_h, var_h, cmean, cvar)
        host_s = time.perf_counter() - t0
        print(f"lloyd pass round {r}: assign + sums + reduce {ms:.3f} ms, assign alone {ms_a:.3f} ms "
              f"({n * k / ms_a / 1e6:.1f} G pairs/s); numpy on the host, one process, {host_s * 1e3:.0f} ms "
              f"= {host_s * 1e3 / ms:.0f} x")

    # ---- streaming kernels: a different chunk per launch
    cols = 3 * n
    chunk_bytes = 4 * T * cols
    n_chunks = max(2, -(-(320 << 20) // chunk_bytes))
    pool = torch.randn(n_chunks, T, cols, dtype=torch.float32, device=dev)
    state_mean = torch.zeros(cols, dtype=torch.float64, device=dev)
    state_m2 = torch.zeros(cols, dtype=torch.float64, device=dev)

    def moments(i):
        L.call("tdx_moments_update", L.ptr(pool[i % n_chunks]), T, cols, L.ptr(state_mean), L.ptr(state_m2), T * (i + 1), L.stream())

    timed(moments, 3)
    mom_bytes = chunk_bytes + 32 * cols
    for r in range(args.rounds):
        ms = timed(moments, args.reps)
        rate = mom_bytes / (ms * 1e-3)
        print(f"moments round {r}: T = {T}, n = {cols}: {ms:.4f} ms, {mom_bytes / 1e6:.1f} MB with the state -> {rate / 1e12:.2f} TB/s "
              f"= {100 * rate / COPY_ROOF:.0f} % of the copy rate; the chunk's {chunk_bytes / 1e6:.1f} MB alone -> "
              f"{chunk_bytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * chunk_bytes / (ms * 1e-3) / COPY_ROOF:.0f} %")
    del pool

    rows = T * n
    for C, norms, what in ((8, ((0, 3), (3, 6)), "features (rows, 8), two norms"), (1, ((0, 0), (0, 0)), "one column")):
        mat_bytes = 4 * rows * C
        n_mats = max(2, -(-(320 << 20) // mat_bytes))
        mats = torch.randn(n_mats, rows, C, dtype=torch.float32, device=dev)
        ws = torch.empty(L.query("tdx_field_stats_workspace_bytes", rows, C), dtype=torch.uint8, device=dev)
        out = torch.empty((C + 2, 4), dtype=torch.float64, device=dev)

        def stats(i):
            L.call("tdx_field_stats", L.ptr(mats[i % n_mats]), rows, C, norms[0][0], norms[0][1], norms[1][0], norms[1][1],
                   L.ptr(out), L.ptr(ws), L.stream())

        timed(stats, 3)
        for r in range(args.rounds):
            ms = timed(stats, args.reps)
            rate = mat_bytes / (ms * 1e-3)
            print(f"field stats round {r}: {what}, rows = {rows}: {ms:.4f} ms, {mat_bytes / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s "
                  f"= {100 * rate / COPY_ROOF:.0f} % of the copy rate")
        del mats


if __name__ == "__main__":
    main()
