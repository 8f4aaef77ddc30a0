#!/usr/bin/env python3
"""The optimiser tail of a training step -- clip-by-global-norm 0.1 + the update -- fused (optim.ClipAdam / ClipAdamW /
ClipRAdam: three launches) against stock torch (clip_grad_norm_ + the foreach optimiser), on two parameter sets:

  dilresnet   DilResNet(hidden 48, N 4), the regression baseline
  diffusion   the benchmark U-Net (dim 32 x 4 levels)

Only the tail is timed: between two HIP events around just those calls (the device is drained before the first), and the
host's time to enqueue them beside it.  Gradients are random tensors of the parameters' shapes.  The two implementations
alternate call by call within a block; --blocks blocks give the run-to-run spread of each block's median.  GPU only.

    python tools/optim_tail_bench.py [--sets dilresnet diffusion] [--rules adam adamw radam] [--reps 40] [--blocks 5]
"""

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))

import torch  # noqa: E402


def parameter_set(name, dev):
    if name == "dilresnet":
        from turbdiff_amd.models.dilresnet import DilResNet

        return list(DilResNet(4, 8, 0, N=4, hidden_dim=48).to(dev).parameters())
    import bench

    return list(bench.build_model(dev).parameters())


def tails(rule, params, clip):
    """{"fused": fn, "torch": fn} on two copies of the parameters; each fn is one tail."""
    from turbdiff_amd import optim

    fused_cls = {"adam": optim.ClipAdam, "adamw": optim.ClipAdamW, "radam": optim.ClipRAdam}[rule]
    torch_cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "radam": torch.optim.RAdam}[rule]
    g = torch.Generator(device=params[0].device).manual_seed(2)
    grads = [torch.randn(p.shape, device=p.device, generator=g) for p in params]
    pf = [p.detach().clone().requires_grad_() for p in params]
    pt = [p.detach().clone().requires_grad_() for p in params]
    for group in (pf, pt):
        for p, gr in zip(group, grads):
            p.grad = gr.clone()
    of, ot = fused_cls(pf, lr=1e-6, max_norm=clip), torch_cls(pt, lr=1e-6)

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(pt, clip)
        ot.step()

    return {"fused": of.step, "torch": torch_tail}


def timed(fn):
    """(ms between HIP events around fn, ms the host spent enqueueing it)"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e.record()
    e.synchronize()
    return s.elapsed_time(e), host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["dilresnet", "diffusion"], choices=["dilresnet", "diffusion"])
    ap.add_argument("--rules", nargs="+", default=["adam", "adamw", "radam"], choices=["adam", "adamw", "radam"])
    ap.add_argument("--reps", type=int, default=40, help="tails per implementation and block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--clip", type=float, default=0.1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_tail_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"# torch {torch.__version__}  device {torch.cuda.get_device_name(0)}  clip {args.clip}  "
          f"{args.blocks} blocks x {args.reps} alternating tails")
    for sname in args.sets:
        params = parameter_set(sname, dev)
        print(f"# {sname}: {len(params)} tensors, {sum(p.numel() for p in params)} elements")
        for rule in args.rules:
            fns = tails(rule, params, args.clip)
            for _ in range(args.warmup):
                for fn in fns.values():
                    fn()
            med = {k: [] for k in fns}
            host = {k: [] for k in fns}
            for _ in range(args.blocks):
                ev = {k: [] for k in fns}
                for _ in range(args.reps):  # alternate the implementations
                    for k, fn in fns.items():
                        d, h = timed(fn)
                        ev[k].append(d)
                        host[k].append(h)
                for k in fns:
                    med[k].append(statistics.median(ev[k]))
            for k in fns:
                print(f"{sname:10s} {rule:6s} {k:6s} tail {statistics.median(med[k]):8.3f} ms  (block medians {min(med[k]):.3f} .. "
                      f"{max(med[k]):.3f}, spread {max(med[k]) - min(med[k]):.3f})  host enqueue {statistics.median(host[k]):.3f} ms")
            gain = statistics.median(med["torch"]) - statistics.median(med["fused"])
            spread = max(max(med[k]) - min(med[k]) for k in fns)
            print(f"{sname:10s} {rule:6s} torch - fused = {gain:+.3f} ms; run-to-run spread of the A/B {spread:.3f} ms")
    sys.stdout.flush()


if __name__ == "__main__":
    main()
