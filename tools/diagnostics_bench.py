#!/usr/bin/env python3
"""Time the case-diagnostics kernels at the size of a real case and print a small report.

    python tools/diagnostics_bench.py [--cells 485000] [--back 121000] [--lags 200] [--frames 10] [--reps 30] [--rounds 3]

One process, the kernels alone between device events, after a warm-up that fills the ring and the halo (so every timed call
is a steady-state call), ``--rounds`` figures of ``--reps`` back-to-back calls each, printed one by one so that the spread is
seen.  The chunks rotate through more than the 256 MiB of the memory-side cache, as they do when they arrive from a file.

  * ``tdx_lagprod_update`` on chunks of ``--frames`` frames, ``--back`` selected cells (the last ones of the cell list),
    ``--lags`` lags: ms per chunk, and the bytes the algorithm must move -- the ring 4 L 3m once, the chunk's selected
    columns 4 F 3m in, the same out into the ring -- over that time, beside the rate of a plain device copy measured in
    the same run (read + write bytes of a 512 MiB ``copy_`` over its time).
  * ``tdx_smooth_residual_update`` on the same chunks, all 3 x cells columns, 32 widths x 101 taps: ms per chunk and fp64
    FMA/s counting F n W (2 h + 1) useful FMAs, beside ``tdx_fma64_probe`` (dependent fp64 FMAs on registers, nothing else)
    timed in the same run: the guides give no fp64 rate, so the probe is the only roof quoted.
  * ``tdx_sqdev_sum`` on the same chunks: ms per chunk and bytes over time.
  * numpy on the host, vectorised, for the same two quantities at ``--host-columns`` columns, scaled linearly to the full
    column count: labelled *extrapolated*, it is not a measurement of the full size.

Nothing here reads a disk: the end-to-end time of a real case is bounded by reading data.h5 and is not measured.
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


def timed(fn, reps):
    """ms per call over `reps` back-to-back calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(reps):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def spread(values):
    return f"min {min(values):.4f} / median {sorted(values)[len(values) // 2]:.4f} / max {max(values):.4f}"


def host_lagprod(window, F, L):
    """acc[i] += sum_t f[L + t] . f[L + t - i] for the F newest rows of a (L + F, cols) float32 window, float64 sums."""
    w = window.astype(np.float64)
    acc = np.zeros(L + 1)
    for t in range(F):
        acc += w[t:L + t + 1][::-1] @ w[L + t]
    return acc


def host_smooth(window, taps):
    """sum over the outputs of a (F + 2 h, cols) window of (taps @ window)^2, float64."""
    K = taps.shape[1]
    win = np.lib.stride_tricks.sliding_window_view(window.astype(np.float64), K, axis=0)  # (F, cols, K)
    o = win @ taps.T
    return (o * o).sum(axis=(0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=485_000)
    ap.add_argument("--back", type=int, default=121_000)
    ap.add_argument("--lags", type=int, default=200)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-columns", type=int, default=3000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diagnostics_bench.py measures on the GPU; none is visible")
    from turbdiff_amd import _lib as L
    from turbdiff_amd.data import diagnostics as D

    dev = torch.device("cuda:0")
    n, m, lags, F = args.cells, args.back, args.lags, args.frames
    cols_a, cols_b = 3 * m, 3 * n
    print(f"device {torch.cuda.get_device_name(0)}, library {L.load().tdx_arch().decode()}, cells {n}, selected {m}, lags {lags}, "
          f"frames per chunk {F}, {args.reps} calls per figure, {args.rounds} rounds")

    chunk_bytes = 4 * F * cols_b
    n_chunks = max(2, -(-(320 << 20) // chunk_bytes))
    pool = torch.randn(n_chunks, F, n, 3, dtype=torch.float32, device=dev)
    mean = torch.randn(n, 3, dtype=torch.float32, device=dev)

    # ---- the copy rate of this device, now
    src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    timed(lambda i: dst.copy_(src), 3)
    copy_rates = [2 * src.numel() / (timed(lambda i: dst.copy_(src), 20) * 1e-3) for _ in range(args.rounds)]
    copy_rate = sorted(copy_rates)[len(copy_rates) // 2]
    print("device copy of 512 MiB, read + write bytes over time: " + ", ".join(f"{r / 1e12:.2f}" for r in copy_rates) + " TB/s")
    del src, dst

    # ---- (a) lagged products
    state = D.LagProducts(np.arange(n - m, n), mean.cpu().numpy(), lags, dev)
    warm = -(-lags // F) + 2
    for i in range(warm):  # fills the ring: from here on every call reads the full window
        state.update(pool[i % n_chunks])
    torch.cuda.synchronize()
    bytes_a = 4 * lags * cols_a + 2 * 4 * F * cols_a
    times = [timed(lambda i: state.update(pool[i % n_chunks]), args.reps) for _ in range(args.rounds)]
    for r, ms in enumerate(times):
        rate = bytes_a / (ms * 1e-3)
        print(f"lag products round {r}: {ms:.4f} ms per chunk, {bytes_a / 1e6:.1f} MB (ring {4 * lags * cols_a / 1e6:.1f} + chunk in and "
              f"out) -> {rate / 1e12:.2f} TB/s = {100 * rate / copy_rate:.0f} % of the copy rate; "
              f"{F * (lags + 1) * cols_a / (ms * 1e-3) / 1e12:.2f} T fp64 FMA/s")
    print(f"lag products: ms per chunk {spread(times)}; finite {bool(np.isfinite(state.result()).all())}")
    ring_bytes = state.ring.numel() * 4
    del state

    # ---- (b) smoothing residual
    taps = D.residual_taps()
    W, K = taps.shape
    sm = D.SmoothResidual(taps, cols_b, dev)
    for i in range(-(-(K - 1) // F) + 2):
        sm.update(pool[i % n_chunks].view(F, cols_b))
    torch.cuda.synchronize()
    fma_b = F * cols_b * W * K
    times = [timed(lambda i: sm.update(pool[i % n_chunks].view(F, cols_b)), max(3, args.reps // 3)) for _ in range(args.rounds)]
    blocks, iters = 256 * 8, 16384
    probe_out = torch.empty(blocks * 256, dtype=torch.float64, device=dev)

    def probe(_):
        L.call("tdx_fma64_probe", L.ptr(probe_out), blocks, iters, L.stream())

    timed(probe, 3)
    probe_rates = [blocks * 256 * iters * 8 / (timed(probe, 10) * 1e-3) for _ in range(args.rounds)]
    probe_rate = sorted(probe_rates)[len(probe_rates) // 2]
    print("fp64 FMA probe (registers only): " + ", ".join(f"{r / 1e12:.2f}" for r in probe_rates) + " T FMA/s")
    for r, ms in enumerate(times):
        rate = fma_b / (ms * 1e-3)
        print(f"smoothing residual round {r}: {ms:.4f} ms per chunk, {fma_b / 1e9:.1f} G useful fp64 FMAs -> {rate / 1e12:.2f} T FMA/s "
              f"= {100 * rate / probe_rate:.0f} % of the probe; the chunk's {chunk_bytes / 1e6:.1f} MB -> "
              f"{chunk_bytes / (ms * 1e-3) / 1e12:.3f} TB/s")
    print(f"smoothing residual: ms per chunk {spread(times)}; finite {bool(np.isfinite(sm.result()).all())}")
    halo_bytes = sm.halo.numel() * 4
    del sm

    # ---- (c) squared deviation
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    timed(lambda i: D.sqdev_sum(pool[i % n_chunks], mean, total), 3)
    times = [timed(lambda i: D.sqdev_sum(pool[i % n_chunks], mean, total), args.reps) for _ in range(args.rounds)]
    for r, ms in enumerate(times):
        rate = chunk_bytes / (ms * 1e-3)
        print(f"squared deviation round {r}: {ms:.4f} ms per chunk, {chunk_bytes / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s "
              f"= {100 * rate / copy_rate:.0f} % of the copy rate")
    print(f"resident state: ring {ring_bytes / 1e6:.0f} MB, halo {halo_bytes / 1e6:.0f} MB, one chunk {chunk_bytes / 1e6:.0f} MB")

    # ---- numpy on the host at a reduced column count, scaled linearly
    hc = args.host_columns
    rng = np.random.default_rng(0)
    window = rng.standard_normal((lags + F, hc)).astype(np.float32)
    host_lagprod(window, F, lags)
    t0 = time.perf_counter()
    host_lagprod(window, F, lags)
    t_a = time.perf_counter() - t0
    window = rng.standard_normal((F + K - 1, hc)).astype(np.float32)
    host_smooth(window, taps)
    t0 = time.perf_counter()
    host_smooth(window, taps)
    t_b = time.perf_counter() - t0
    print(f"numpy on the host at {hc} columns: lag products {t_a * 1e3:.2f} ms per chunk, smoothing {t_b * 1e3:.2f} ms per chunk; "
          f"EXTRAPOLATED linearly to {cols_a} / {cols_b} columns: {t_a * cols_a / hc * 1e3:.0f} ms and {t_b * cols_b / hc * 1e3:.0f} ms "
          f"per chunk (not measured at that size)")


if __name__ == "__main__":
    main()
