#!/usr/bin/env python3
"""BASELINE config 4: T-step DDPM sampling of N trajectories sharded over the GPUs of one node,
one hipGraph-captured reverse step per replay (no collective inside the loop).

  python tools/sample_bench.py --trajectories 8 --timesteps 1000            # 1 GPU
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/sample_bench.py --trajectories 64

  python tools/sample_bench.py --trajectories 8 --sampling-steps 50 --eta 0  # DDIM over 50 of the 1000 timesteps; the
                                                                            # ancestral sampler is timed in the same process

  python tools/sample_bench.py --trajectories 8 --learned-variances --steps 50
      # the U-Net with 2F output channels and the per-voxel variance (tdx_p_sample_step_lv_rng); timed in the same process,
      # alternating: this captured step, the eager torch loop it replaces on the default route (`general_loop`, what
      # TDX_GRAPH_SAMPLER=0 runs) and the fixed-variance captured step (`fixed_variance`)

  python tools/sample_bench.py --trajectories 8 --learned-variances --sampling-steps 50 --sampling-method respaced
      # the learned-variance model over 50 of the 1000 timesteps (`respaced`: tdx_p_sample_step_lv_respaced_rng, `ddim`:
      # tdx_ddim_step_lv_rng); its captured step and the captured T-step learned-variance step (`ancestral`) alternate in
      # this process, --rounds times each

  python tools/sample_bench.py --trajectories 8 --actfn gelu --steps 50 --ab 3
      # the U-Net built with another of the reference's activations; --ab N: the captured step with models.ddpm.FUSE_ACTFNS on
      # (activation inside the GroupNorm kernels) and off (act = 0 pass + torch module per Block), N times each, alternating

Prints one JSON line (rank 0): whole-job samples/s = trajectories / max-over-ranks wall time."""
import argparse, json, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))
import torch
import bench
from turbdiff_amd import parallel
from turbdiff_amd.models.conditioning import Conditioning
from turbdiff_amd.sampling import GraphSampler

ap = argparse.ArgumentParser()
ap.add_argument("--trajectories", type=int, default=8)
ap.add_argument("--timesteps", type=int, default=1000)
ap.add_argument("--steps", type=int, default=0, help="time only this many reverse steps and extrapolate (0 = full loop)")
ap.add_argument("--sampling-steps", type=int, default=None,
                help="DDIM sampling over this many of the training timesteps; the ancestral loop is timed first, as `ancestral`")
ap.add_argument("--eta", type=float, default=0.0, help="with --sampling-steps: 0 = deterministic DDIM ... 1 = posterior variance")
ap.add_argument("--sampling-method", default=None, choices=["ddim", "respaced"],
                help="with --learned-variances --sampling-steps: the sampler over the subsequence; see above")
ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "f32", "f32s"])
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--learned-variances", action="store_true", help="out_features = 2F, learned_variances=True; see above")
ap.add_argument("--actfn", default="silu", choices=["silu", "gelu", "relu", "softplus", "tanh"], help="activation of the U-Net")
ap.add_argument("--ab", type=int, default=0, help="with --actfn: time FUSE_ACTFNS on and off alternately, this many times each")
ap.add_argument("--rounds", type=int, default=3, help="with --learned-variances: how often the sides are timed in turn")
a = ap.parse_args()
if a.dtype == "f32s":  # fp32 tensors, split-precision convs
    import os
    os.environ["TDX_CONV_IMPL"] = "split"
rank, world, local = parallel.init_from_env("nccl")
torch.cuda.set_device(local)
dev = torch.device("cuda", local)
fixed = bench.build_model(dev, bench.MODE_DTYPE[a.dtype], timesteps=a.timesteps)
diff = fixed
if a.learned_variances:
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion
    if (a.sampling_steps is None) != (a.sampling_method is None):
        ap.error("--learned-variances takes --sampling-steps and --sampling-method together")
    torch.manual_seed(0)
    net = DenoisingModel(in_features=4, out_features=8, c_local_features=4, c_global_features=0, timesteps=a.timesteps, dim=32,
                         u_net_levels=4, norm_type="group")
    diff = GaussianDiffusion(net, timesteps=a.timesteps, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True,
                             learned_variances=True).to(dev)
    diff.model.set_compute_dtype(bench.MODE_DTYPE[a.dtype])
if a.actfn != "silu":
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion
    from turbdiff_amd.training import ACTFNS
    if a.learned_variances or a.sampling_steps is not None:
        ap.error("--actfn times the ancestral fixed-variance sampler")
    torch.manual_seed(0)
    net = DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=a.timesteps, dim=32,
                         u_net_levels=4, norm_type="group", actfn=ACTFNS[a.actfn])  # bench.new_denoiser with the activation
    diff = GaussianDiffusion(net, timesteps=a.timesteps, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True).to(dev)
    diff.model.set_compute_dtype(bench.MODE_DTYPE[a.dtype])
ids = list(parallel.shard_trajectories(a.trajectories, rank, world))
x, c, cell_idx = bench.synthetic_inputs(len(ids), dev)
C = {Conditioning.Type.CELL_TYPE: c}


def measure(total, s=None, model=None, **kw):
    """(seconds for the timed steps, timed steps, sampler) of a sampler whose full loop has `total` reverse steps"""
    if s is None:
        s = GraphSampler(model or diff, x, C, cell_idx, seed=0, trajectory_ids=ids, use_graph=not a.no_graph, **kw)
        s.run_steps(2)                 # warm-up incl. graph capture
    s.reset()
    torch.cuda.synchronize()
    if world > 1: torch.distributed.barrier()
    t0 = time.perf_counter()
    n = min(a.steps, total) if a.steps > 0 else total
    s.run_steps(n)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX); dt = t.item()
    return dt, n, s


def record(dt, n, total):
    return {"timed_steps": n, "extrapolated": n != total, "ms_per_reverse_step": 1e3 * dt / n, "seconds_per_batch": dt * total / n}


def measure_general_loop(n):
    """seconds for n reverse steps of the eager learned-variance loop (GaussianDiffusion._general_sample: one launch
    sequence and a dozen torch elementwise ops per step, torch.randn_like noise), started at timestep n"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    diff.p_sample_loop(x, C, cell_idx, start_from=n, noise_fn=torch.randn_like)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


total = a.timesteps if a.sampling_steps is None else a.sampling_steps
extra = {}
if a.learned_variances and a.sampling_steps is not None:
    # the S-step sampler and the T-step learned-variance step it stands in for, alternating; both per-step figures are of
    # min(--steps, S) replays (0 = S) of one captured step each
    kw = dict(sampling_timesteps=a.sampling_steps, eta=a.eta, sampling_method=a.sampling_method)
    dt, n, s = measure(total, **kw)
    _, _, sa = measure(total)
    sides = {a.sampling_method: [], "ancestral": []}
    for _ in range(a.rounds):
        dt, n, s = measure(total, s=s)
        sides[a.sampling_method].append(1e3 * dt / n)
        sides["ancestral"].append(1e3 * measure(total, s=sa)[0] / n)
    med = lambda v: sorted(v)[len(v) // 2]
    anc = med(sides["ancestral"])
    extra = {"learned_variances": True, "sampling_steps": a.sampling_steps, "eta": a.eta, "sampling_method": a.sampling_method,
             "rounds_ms_per_reverse_step": sides,
             "ancestral": {"timed_steps": n, "ms_per_reverse_step": anc, "seconds_per_batch": 1e-3 * anc * a.timesteps}}
    dt = 1e-3 * med(sides[a.sampling_method]) * n
elif a.learned_variances:
    n_gen = min(a.steps, total) if a.steps > 0 else total
    measure_general_loop(2)  # warm-up
    dt, n, s = measure(total)
    _, _, sf = measure(total, model=fixed)
    sides = {"captured": [], "general_loop": [], "fixed_variance": []}
    for _ in range(a.rounds):
        dt, n, s = measure(total, s=s)
        sides["captured"].append(1e3 * dt / n)
        sides["general_loop"].append(1e3 * measure_general_loop(n_gen) / n_gen)
        sides["fixed_variance"].append(1e3 * measure(total, s=sf)[0] / n)
    med = lambda v: sorted(v)[len(v) // 2]
    extra = {"learned_variances": True, "rounds_ms_per_reverse_step": sides,
             "general_loop": {"timed_steps": n_gen, "ms_per_reverse_step": med(sides["general_loop"])},
             "fixed_variance": {"timed_steps": n, "ms_per_reverse_step": med(sides["fixed_variance"])}}
    dt = 1e-3 * med(sides["captured"]) * n
elif a.ab:
    from turbdiff_amd.models import ddpm as D
    sides, samplers = {"fused": [], "unfused": []}, {}
    for _ in range(a.ab):
        for name, on in (("fused", True), ("unfused", False)):
            D.FUSE_ACTFNS = on  # read per forward: at capture for the graph, at every step with --no-graph
            dt, n, samplers[name] = measure(total, s=samplers.get(name))
            sides[name].append(1e3 * dt / n)
    D.FUSE_ACTFNS = True
    med = lambda v: sorted(v)[len(v) // 2]
    extra = {"actfn": a.actfn, "rounds_ms_per_reverse_step": sides, "unfused": {"timed_steps": n, "ms_per_reverse_step": med(sides["unfused"])}}
    dt, s = 1e-3 * med(sides["fused"]) * n, samplers["fused"]
elif a.sampling_steps is not None:
    dt, n, s = measure(a.timesteps)
    extra = {"sampling_steps": a.sampling_steps, "eta": a.eta, "ancestral": record(dt, n, a.timesteps)}
    del s
    dt, n, s = measure(total, sampling_timesteps=a.sampling_steps, eta=a.eta)
else:
    dt, n, s = measure(total)
if rank == 0:
    full = dt * total / n
    print(json.dumps({"metric": "DDPM samples/sec (192x64x48x4)", "value": a.trajectories / full, "unit": "samples/s",
                      "n_gpus": world, "trajectories": a.trajectories, "per_gpu": len(ids), "timesteps": a.timesteps,
                      **record(dt, n, total), "dtype": a.dtype, "hipgraph": not a.no_graph,
                      "finite": bool(torch.isfinite(s.x_t).all()), **({"actfn": a.actfn} if a.actfn != "silu" else {}), **extra}))
if world > 1:
    torch.distributed.barrier(); torch.distributed.destroy_process_group()
