#!/usr/bin/env python3
"""One training step (fwd + bwd + clip + RAdam; --optimizer adam | adamw: optim.ClipAdam / ClipAdamW) of the BASELINE configs[1] U-Net on an arbitrary grid, for profiling:
    python tools/step_bench.py --grid 194 50 50 --mode bf16 --batch 6 --steps 5
--model cfg1: the 2-level U-Net of BASELINE configs[0] instead (with --grid 48 32 32 --batch 1 its host-bound eager step).
--learned-variances --elbo-weight W: the same U-Net with 2F output channels and the simple + ELBO loss (ops.elbo_loss);
--torch-elbo (or TDX_STEP_BENCH_TORCH_ELBO=1, so that tools/ab_step.sh can flip it) evaluates that loss with the torch formulation the
kernel replaced (GaussianDiffusion._p_losses_elbo_torch), --ab N times both N times in this process, alternating.
--actfn NAME: the same U-Net built with another of the reference's activations (training.ACTFNS); with --ab N the step is timed
N times each with models.ddpm.FUSE_ACTFNS on (the activation inside the GroupNorm kernels, fused ResnetBlocks) and off (act = 0
pass + torch module + torch add per Block: the route of every non-SiLU model before the kernels had activation codes), alternating.
prints ms per step; under `rocprofv3 --kernel-trace --stats` the per-kernel table of exactly these steps."""
import argparse, os, sys, time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))
import torch
import bench
from turbdiff_amd.models.conditioning import Conditioning

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=[194, 50, 50])
ap.add_argument("--mode", default="bf16")
ap.add_argument("--batch", type=int, default=6)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--model", default="bench", choices=["bench", "cfg1"])
ap.add_argument("--optimizer", default="radam", choices=["radam", "adam", "adamw"], help="the fused optimiser that ends the step")
ap.add_argument("--learned-variances", action="store_true", help="2F output channels, per-voxel variance")
ap.add_argument("--elbo-weight", type=float, default=None, help="with --learned-variances: weight of the ELBO term (None: simple loss only)")
ap.add_argument("--torch-elbo", action="store_true", default=os.environ.get("TDX_STEP_BENCH_TORCH_ELBO", "0") not in ("", "0"),
                help="the ELBO loss by torch ops (the route before ops.elbo_loss) instead of the fused kernel")
ap.add_argument("--ab", type=int, default=0, help="with --elbo-weight: time fused and torch ELBO alternately, this many times each; "
                                                  "with --actfn: FUSE_ACTFNS on and off")
ap.add_argument("--actfn", default="silu", choices=["silu", "gelu", "relu", "softplus", "tanh"], help="activation of the U-Net (--model bench)")
a = ap.parse_args()
dev = torch.device("cuda:0")


def torch_elbo_p_losses(diff):
    """p_losses as it ran before the fused loss: q_sample, model, then GaussianDiffusion._p_losses_elbo_torch"""
    from turbdiff_amd import ops

    def p_losses(x_start, t, C, metadata, variables, noise=None):
        x_start = x_start.contiguous().float()
        mask, n_cells = diff.domain_mask(metadata.cell_idx, x_start[0, 0].numel())
        noise = torch.randn_like(x_start) if noise is None else noise
        x_t = ops.q_sample(x_start, noise, diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod, t, mask=mask,
                           keep_bcs=not diff.noise_bcs)
        return diff._p_losses_elbo_torch(diff.model(x_t, t, C), x_start, x_t, t, noise, mask, n_cells, metadata.cell_idx), t

    return p_losses


if a.optimizer != "radam":
    def new_optimizer(diff, mode, n_loss_elements):
        """bench.new_optimizer with the chosen update rule"""
        from turbdiff_amd import optim
        from turbdiff_amd.training import DiffusionTrainer

        scale = DiffusionTrainer.initial_loss_scale(n_loss_elements) if mode == "fp16" else None
        return {"adam": optim.ClipAdam, "adamw": optim.ClipAdamW}[a.optimizer](diff.parameters(), lr=1e-4, max_norm=0.1, loss_scale=scale)

    bench.new_optimizer = new_optimizer  # (what bench.timed_train_steps builds its optimiser with)

if a.model == "cfg1":
    from turbdiff_amd.models.ddpm import GaussianDiffusion
    diff = GaussianDiffusion(bench.new_cfg1_denoiser(), timesteps=10, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True).to(dev)
elif a.learned_variances:
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion
    torch.manual_seed(0)
    net = DenoisingModel(in_features=4, out_features=8, c_local_features=4, c_global_features=0, timesteps=500, dim=32,
                         u_net_levels=4, norm_type="group")
    diff = GaussianDiffusion(net, timesteps=500, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True,
                             learned_variances=True, elbo_weight=a.elbo_weight).to(dev)
elif a.actfn != "silu":
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion
    from turbdiff_amd.training import ACTFNS
    torch.manual_seed(0)
    net = DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=500, dim=32,
                         u_net_levels=4, norm_type="group", actfn=ACTFNS[a.actfn])  # bench.new_denoiser with the activation
    diff = GaussianDiffusion(net, timesteps=500, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True).to(dev)
else:
    diff = bench.build_model(dev)
x, c, idx = bench.synthetic_inputs(a.batch, dev, tuple(a.grid))
C, md = {Conditioning.Type.CELL_TYPE: c}, SimpleNamespace(cell_idx=idx)
v = a.grid[0] * a.grid[1] * a.grid[2]
if a.learned_variances and a.elbo_weight is not None and (a.torch_elbo or a.ab):
    fused = diff.p_losses
    for i in range(max(a.ab, 1)):
        for name, fn in (("fused-elbo", fused), ("torch-elbo", torch_elbo_p_losses(diff))):
            if name == "fused-elbo" and not a.ab:
                continue
            diff.p_losses = fn  # (an instance attribute: GaussianDiffusion.forward calls self.p_losses)
            ms = bench.timed_train_steps(diff, x, C, md, a.mode, a.steps, a.warmup)
            print(f"{name}: grid {a.grid} B {a.batch} {a.mode}: {ms:.3f} ms/step = {a.batch * v / ms / 1e3:.1f} M voxels/s")
    sys.exit(0)
if a.ab and not a.learned_variances:
    from turbdiff_amd.models import ddpm as D
    for i in range(a.ab):
        for name, on in (("fused-act", True), ("unfused-act", False)):
            D.FUSE_ACTFNS = on  # read per call by Block / ResnetBlock
            ms = bench.timed_train_steps(diff, x, C, md, a.mode, a.steps, a.warmup)
            print(f"{name}: actfn {a.actfn} grid {a.grid} B {a.batch} {a.mode}: {ms:.3f} ms/step = {a.batch * v / ms / 1e3:.1f} M voxels/s")
    sys.exit(0)
ms = bench.timed_train_steps(diff, x, C, md, a.mode, a.steps, a.warmup)
print(f"actfn {a.actfn} grid {a.grid} B {a.batch} {a.mode} {a.optimizer}: {ms:.3f} ms/step = {a.batch * v / ms / 1e3:.1f} M voxels/s")
