#!/usr/bin/env python3
"""Evaluate a checkpoint: counterpart of the reference's scripts/eval_ckpt.py:43-76 on the MI355X build.

    python tools/eval_ckpt.py CKPT SAMPLES.npz [--cases CASES.pt | --synthetic N] [key=value ...]

Flow, step for step as in the reference: load the checkpoint -> take the run configuration from ``ckpt["config"]``
-> merge dotted ``key=value`` overrides -> seed -> build the task from the configuration
(``DiffusionTrainer.from_config``; ``matmul_precision`` picks the compute mode) -> ``load_state_dict(strict)``
-> for every validation batch: ``task.sample`` -> ``SampleStore`` -> metrics over the stored samples.

Differences, all on the I/O side (no h5py / POT in this image): validation cases come from ``--cases`` (a
``torch.save``d list of ``(OpenFOAMMetadata, times, {Variable: (T, n_cells, dims)})`` tuples plus the statistics, see
``turbdiff_amd.data.ofles.InMemoryRepository``) or are synthesised; the store lives in memory and is written as one
``.npz``.  By default it prints the log-TKE-spectrum L2 distance (``val/log_tke_l2``, computed on the device), which no
paper table reports; ``--sample-metrics`` adds the reference's own ``SampleMetricsCollection`` metrics without the
expensive one (``tke-front``, ``tke-middle``, ``tke-back``, ``tke``, ``max-mean-tke-pos``, as the reference's
eval_ckpt.py computes them with ``expensive_metrics=False``), ``--expensive-metrics`` also ``wasserstein`` (exact W2 by
the batched device auction).  ``--sampling-steps N [--eta E]`` draws the samples with the DDIM sampler over N of the training
timesteps instead of the full ancestral chain (what that does to the metrics has not been measured); a checkpoint with
learned variances also needs ``--sampling-method respaced|ddim`` for that (equally unmeasured).  Their side files (``regions.npz``, ``max-mean-tke.npy``, ``mean-flow.h5``) come from an
optional ``side`` entry of the ``--cases`` blob, ``{case_name: {file name: value}}``; ``--synthetic`` cases bring their
own (channel-aligned region blocks, a nominal max-mean-TKE position).  Those stand-ins are not the reference's regions, so
``wasserstein`` on them is not the paper's metric: for real cases ``tools/prepare_dataset.py`` writes the three side files
(and ``stats.pickle``) from the raw ``data.h5`` files, as the reference's scripts do.
"""

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "generative-turbulence_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def merge_overrides(config: dict, overrides):
    """``a.b.c=value`` items onto a nested dict (OmegaConf.merge(run_config, OmegaConf.from_cli(overrides)))."""
    import yaml

    for item in overrides:
        key, _, value = item.partition("=")
        node = config
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = yaml.safe_load(value)
    return config


def synthetic_cases(n_cases, grid=(48, 32, 32), n_times=12, seed=0):
    """Channel-flow-like cases with a box obstacle: metadata, times and (u, p) samples at the in-domain cells."""
    from turbdiff_amd.data.ofles import BoundaryCondition, OpenFOAMMetadata, OpenFOAMStats, Variable

    g = torch.Generator().manual_seed(seed)
    X, Y, Z = grid
    cases = []
    for c in range(n_cases):
        inside = torch.zeros(grid, dtype=torch.bool)
        inside[1:-1, 1:-1, 1:-1] = True
        x0 = 6 + 3 * c
        inside[x0:x0 + 6, Y // 2 - 4:Y // 2 + 4, 0:Z // 2] = False
        cell_idx = inside.flatten().nonzero().flatten()
        flat = torch.arange(X * Y * Z).view(grid)
        boundaries = {"inlets": {"idx": flat[0].flatten()}, "outlets": {"idx": flat[-1].flatten()},
                      "walls": {"idx": torch.cat((flat[1:-1, 0].flatten(), flat[1:-1, -1].flatten()))}}
        bcs = {Variable.U: {"inlets": BoundaryCondition(BoundaryCondition.Type.FIXED_VALUE, torch.tensor([1.0, 0.0, 0.0])),
                            "walls": BoundaryCondition(BoundaryCondition.Type.FIXED_VALUE, torch.zeros(3)),
                            "outlets": BoundaryCondition(BoundaryCondition.Type.ZERO_GRADIENT)},
               Variable.P: {"inlets": BoundaryCondition(BoundaryCondition.Type.ZERO_GRADIENT),
                            "walls": BoundaryCondition(BoundaryCondition.Type.ZERO_GRADIENT),
                            "outlets": BoundaryCondition(BoundaryCondition.Type.FIXED_VALUE, torch.zeros(1))}}
        meta = OpenFOAMMetadata(np.array(grid), cell_idx, boundaries, bcs, file=Path(f"case-{c:02d}/data.h5"))
        n = len(cell_idx)
        u = torch.randn(n_times, n, 3, generator=g) * 0.3 + torch.tensor([1.0, 0.0, 0.0])
        p = torch.randn(n_times, n, 1, generator=g) * 0.1
        cases.append((meta, np.linspace(0.0, 1.1, n_times), {Variable.U: u, Variable.P: p}))
    allu = torch.cat([c[2][Variable.U].reshape(-1, 3) for c in cases])
    allp = torch.cat([c[2][Variable.P].reshape(-1, 1) for c in cases])
    rec = lambda t: {"mean": t.mean(0), "std": t.std(0), "min": t.amin(0), "max": t.amax(0)}
    nrm = lambda t: {k: v.reshape(()) for k, v in rec(t.norm(dim=-1, keepdim=True)).items()}
    stats = OpenFOAMStats({"u": rec(allu), "p": rec(allp), "norm(u)": nrm(allu), "norm(p)": nrm(allp)})
    return cases, stats


def synthetic_side(cases, n_regions=8):
    """Side data of synthetic cases: regions = ``n_regions`` contiguous blocks of cells along the channel, the
    max-mean-TKE position at a third of the channel length."""
    from turbdiff_amd.data.ofles import Variable

    side = {}
    for meta, _, fields in cases:
        n = fields[Variable.U].shape[1]
        side[meta.case_name] = {"regions.npz": (np.arange(n) * n_regions // n).astype(np.int64),
                                "max-mean-tke.npy": float(int(meta.cell_counts[0]) // 3)}
    return side


def add_curl_statistics(cases, stats, device):
    """The ``norm(curl)`` record of the statistics (WassersteinMetric's feature scale), from every sample of the cases."""
    from turbdiff_amd.data.ofles import OpenFOAMData, Variable
    from turbdiff_amd.metrics import curl

    norms = []
    for meta, times, fields in cases:
        m = meta.to(device)
        d = OpenFOAMData(m, torch.as_tensor(times, device=device), {v: f.to(device) for v, f in fields.items()})
        c = curl(d.grid_embedding((Variable.U,)), meta.h).flatten(-3)[..., m.unpadded_cell_idx]  # (T, 3, n_cells)
        norms.append(c.norm(dim=1).reshape(-1).cpu())
    n = torch.cat(norms)
    stats.stats["norm(curl)"] = {"mean": n.mean(), "std": n.std(), "min": n.min(), "max": n.max()}
    stats._normalizers.clear()
    return stats


def sample_metrics(store, cases, stats, device, *, side=None, expensive=False, prefix="val"):
    """The reference's SampleMetricsCollection over the stored samples, the case data held in memory."""
    from turbdiff_amd.data.ofles import InMemoryRepository
    from turbdiff_amd.models.metrics import (MaxMeanTKEPositionMetric, SampleMetricsCollection, WassersteinMetric,
                                             WassersteinTKE)

    repos = {c[0].case_name: InMemoryRepository([c]) for c in cases}
    coll = SampleMetricsCollection(prefix, None, [WassersteinTKE(side=side), WassersteinMetric(side=side),
                                                  MaxMeanTKEPositionMetric(side=side)], repository=repos.__getitem__).to(device)
    if "norm(curl)" not in stats.stats:
        stats = add_curl_statistics(cases, stats, device)
    return {k: float(v) for k, v in coll.compute(store, stats, device, expensive_metrics=expensive).items()}


def evaluate(ckpt: dict, cases, stats, device, *, overrides=(), seed=2883413570083077179, samples_path=None,
             eval_batch_size=None, val_samples=2, discard_first_seconds=0.0, start_from=None, compute_mode=None,
             sampling_steps=None, eta=0.0, sampling_method=None):
    """The body of eval_ckpt.py:43-76.  Returns (store, metrics dict, task).  `sampling_steps`: sample with the DDIM
    sampler over that many of the training timesteps (and `eta`) instead of the full ancestral chain; `sampling_method`:
    the sampler a learned-variance model takes for that ("respaced" / "ddim", GaussianDiffusion.p_sample_loop)."""
    from turbdiff_amd.data.ofles import InMemoryRepository, OpenFOAMDataset, OpenFOAMEvaluationSampler
    from turbdiff_amd.data.staging import DeviceStager
    from turbdiff_amd.models.metrics import LogTKESpectrumL2Distance, SampleStore
    from turbdiff_amd.training import DiffusionTrainer

    if "config" not in ckpt:
        raise SystemExit("Checkpoint has no config")
    config = merge_overrides(dict(ckpt["config"]), overrides)
    torch.manual_seed(seed % (2**63))
    task = DiffusionTrainer.from_config(config, max_train_steps=1, compute_mode=compute_mode)
    task.load_state_dict(ckpt["state_dict"], strict=True)
    task = task.to(device).eval()
    task.sampling_timesteps, task.sampling_eta, task.sampling_method = sampling_steps, eta, sampling_method

    dataset = OpenFOAMDataset(InMemoryRepository(cases), stats, discard_first_seconds)
    bs = eval_batch_size or int(config["model"].get("eval_batch_size", 8))
    sampler = OpenFOAMEvaluationSampler(dataset, batch_size=bs, samples_per_file=val_samples)
    store = SampleStore(samples_path, task.variables)
    batches = (dataset[idxs] for idxs in sampler)
    with torch.no_grad():
        for batch in DeviceStager(batches, device):  # pinned staging + copy stream (move_data_to_device)
            if start_from is None:
                task.validation_step(batch, store)
            else:  # short runs: start the reverse process from a noised data sample
                store.add_cells(task.sample_cells(batch, start_from=start_from), batch.data.metadata)
    if samples_path is not None:
        store.save()

    # metric over the stored samples: log-TKE-spectrum L2 distance between generated and data velocity fields of
    # each case, on the largest obstacle-free box behind the inlet plane (metrics.py:319-380)
    from turbdiff_amd.data.ofles import Variable

    dist = LogTKESpectrumL2Distance(task.val_sample_metrics.metrics[0].distance.tke_spectrum).to(device)
    metrics = {}
    for meta, _, fields in cases:
        if meta.case_name not in store.case_names:
            continue
        gen = store.load_samples(meta).samples[Variable.U].to(device)       # (n, n_cells, 3)
        dat = fields[Variable.U][-gen.shape[0]:].to(device)
        X, Y, Z = (int(c) for c in meta.cell_counts)
        dense = lambda cells: torch.zeros(cells.shape[0], 3, X * Y * Z, device=device).index_copy_(
            2, meta.cell_idx.to(device), cells.transpose(1, 2)).view(-1, 3, X, Y, Z)
        box = (slice(None), slice(None), slice(X // 2, X - 1), slice(1, Y - 1), slice(1, Z - 1))
        ug, ud = dense(gen)[box].contiguous(), dense(dat)[box].contiguous()
        D, *_ = dist(ug, ud, ud.mean(0))
        metrics[f"val/{meta.case_name}/log_tke_l2"] = float(D.mean().item())
    if metrics:
        metrics["val/log_tke_l2"] = float(np.mean(list(metrics.values())))
    return store, metrics, task


def main():
    ap = argparse.ArgumentParser(description="Evaluate a checkpoint with overrides")
    ap.add_argument("-d", "--device", default="cuda")
    ap.add_argument("-s", "--seed", default=2883413570083077179, type=int)
    ap.add_argument("--cases", help="torch.save'd {'cases': [...], 'stats': OpenFOAMStats.stats} of the validation cases")
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate on N synthetic cases instead")
    ap.add_argument("--start-from", type=int, default=None, help="start the reverse process at this step (smoke runs)")
    ap.add_argument("--sampling-steps", type=int, default=None,
                    help="DDIM sampling over this many of the training timesteps instead of the full ancestral chain")
    ap.add_argument("--eta", type=float, default=0.0, help="with --sampling-steps: 0 = deterministic DDIM ... 1 = posterior variance")
    ap.add_argument("--sampling-method", default=None, choices=["ddim", "respaced"],
                    help="with --sampling-steps on a model with learned variances: the respaced ancestral step or DDIM on eps_hat")
    ap.add_argument("--compute-mode", default=None, choices=[None, "f32", "f32s", "bf16", "fp16"])
    ap.add_argument("--sample-metrics", action="store_true", help="also print the reference's cheap sample metrics")
    ap.add_argument("--expensive-metrics", action="store_true", help="with --sample-metrics, also the Wasserstein metric")
    ap.add_argument("ckpt", help="Path to .ckpt file")
    ap.add_argument("samples_path", help=".npz file for storing samples")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_intermixed_args()  # options may sit between the positionals and the overrides
    samples_path = Path(args.samples_path)
    assert samples_path.suffix == ".npz" and not samples_path.exists()
    ckpt = torch.load(args.ckpt, map_location="cpu", weights_only=False)
    if args.cases:
        from turbdiff_amd.data.ofles import OpenFOAMStats

        blob = torch.load(args.cases, weights_only=False)
        cases, stats, side = blob["cases"], OpenFOAMStats(blob["stats"]), blob.get("side")
    elif args.sample_metrics or args.expensive_metrics:
        # long enough for WassersteinTKE's three channel cubes and the max-mean-TKE window behind x = 24
        cases, stats = synthetic_cases(max(args.synthetic, 1), grid=(64, 18, 18))
        side = synthetic_side(cases)
    else:
        cases, stats = synthetic_cases(max(args.synthetic, 1))
    device = torch.device(args.device)
    store, metrics, _ = evaluate(ckpt, cases, stats, device, overrides=args.overrides, seed=args.seed,
                                 samples_path=samples_path, start_from=args.start_from, compute_mode=args.compute_mode,
                                 sampling_steps=args.sampling_steps, eta=args.eta, sampling_method=args.sampling_method)
    if args.sample_metrics or args.expensive_metrics:
        metrics.update(sample_metrics(store, cases, stats, device, side=side, expensive=args.expensive_metrics))
    for key in sorted(metrics):
        print(f"{key}: {metrics[key]}")


if __name__ == "__main__":
    main()
