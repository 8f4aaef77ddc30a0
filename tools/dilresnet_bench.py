#!/usr/bin/env python3
"""DilResNet on one MI355X: a training step (B = 3) and the rollout (B = 8, one step and a 30-step unroll) on the shapes
dataset's 194 x 50 x 50 grid, hidden 48, N 4, dilations 1/2/4/8, synthetic seeded data, four implementations timed
alternately in one process after warm-up:

  fused      the bf16 chain of models.dilresnet (epilogue-fused convs, fused backward folds; rollout update in the decode conv)
  unfused    the same bf16 network composed from ops.conv3d and torch ReLU / adds (forward_unfused)
  f32        the fp32 parity path (vector-ALU convg kernels + torch elementwise ops)
  torch      stock PyTorch-ROCm: F.pad(replicate) + F.conv3d, bf16 autocast and fp32

Prints max-abs / rel-L2 of fused against unfused on the same inputs, then one line per (workload, implementation) with the
median ms over --reps.  GPU only: exits with an error without one.

--optimizer: what ends the training steps -- fused (optim.ClipAdam, clip 0.1 + Adam in three launches: what DilResNetTrainer
uses on a GPU), torch (clip_grad_norm_ 0.1 + torch.optim.Adam), or both: the HIP bf16 chain then gets one row per optimiser,
"fused" and "fused/torch-opt", alternating like the other columns (the remaining rows end with the torch pair).  The tail
alone, between HIP events: tools/optim_tail_bench.py.

    python tools/dilresnet_bench.py [--reps 5] [--steps 30] [--optimizer fused|torch|both]
"""

import argparse
import hashlib
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def kernel_source_hash():
    h = hashlib.sha256()
    for p in sorted((ROOT / "generative-turbulence_amd" / "csrc").glob("*.h*")):
        h.update(p.read_bytes())
    return h.hexdigest()[:16]


def torch_forward(net, x, c):
    """Stock PyTorch: the reference's forward with replicate padding spelled out, NCDHW."""
    def conv(m, v, d):
        return F.conv3d(F.pad(v, (d,) * 6, mode="replicate"), m.weight, m.bias, dilation=d)

    u = conv(net.encode, x, 1)
    ce = conv(net.encode_c_local, c[None], 1)
    for blk in net.blocks:
        u = u + ce
        h = u
        for layer in blk.layers:
            h = F.relu(conv(layer, h, layer.dilation[0]))
        u = u + h
    return conv(net.decode, u, 1)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="rollout length (eval_unroll_steps of dilresnet.yaml)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--optimizer", default="both", choices=["fused", "torch", "both"], help="the optimiser tail of the training steps")
    ap.add_argument("--only", default=None, help="time one implementation only (profiling runs): fused | unfused | f32 | torch")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dilresnet_bench.py needs a GPU")
    from turbdiff_amd.models.conditioning import Conditioning
    from turbdiff_amd.models.dilresnet import DilResNet

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    X, Y, Z = 194, 50, 50
    net = DilResNet(4, 8, 0, N=4, hidden_dim=48).to(dev)
    from turbdiff_amd.optim import ClipAdam

    # (lr 1e-6: both optimisers step the same parameters, which barely move over the run)
    opts = {"fused": ClipAdam(net.parameters(), lr=1e-6, max_norm=0.1), "torch": torch.optim.Adam(net.parameters(), lr=1e-6)}
    g = torch.Generator(device=dev).manual_seed(1)
    c = torch.randn(8, X, Y, Z, device=dev, generator=g)
    C = {Conditioning.Type.CELL_TYPE: c}
    x3 = torch.randn(3, 4, X, Y, Z, device=dev, generator=g)
    t3 = torch.randn(3, 4, X, Y, Z, device=dev, generator=g)
    x8 = torch.randn(8, 4, X, Y, Z, device=dev, generator=g)
    inside = torch.rand(X, Y, Z, device=dev, generator=g) > 0.1
    mean, std = torch.zeros(4, device=dev), torch.full((4,), 1e-2, device=dev)

    print(f"# kernel-source hash {kernel_source_hash()}  torch {torch.__version__}  device {torch.cuda.get_device_name(0)}")
    if not args.only:  # (profiling runs time one implementation and nothing else)
        # ---- agreement on identical bf16-rounded operands: fused and unfused bf16 against each other and against fp32.  The
        # block-internal weight gradients move by ~10 % in bf16 on either path (sums with heavy cancellation); the fused
        # chain is judged by being no farther from fp32 than the unfused composition
        res = {}
        for name, dt in (("f32", torch.float32), ("fused", torch.bfloat16), ("unfused", torch.bfloat16)):
            xb = net.state_input(x3, torch.bfloat16).to(dt)
            cl = net.encode_conditioning(C, torch.bfloat16).detach().to(dt).requires_grad_()
            net.zero_grad(set_to_none=True)
            y = (net.forward_unfused if name != "fused" else net.forward_nvc)(xb, cl)
            (y[..., :4] * t3.movedim(1, -1)).sum().backward()
            res[name] = [y.detach().float()[..., :4], cl.grad.float()] + [p.grad.clone() for p in net.parameters() if p.grad is not None]
            del y
        labels = ["output", "d c_enc"] + [n for n, p in net.named_parameters() if p.grad is not None]
        rel = lambda a, b: ((a - b).norm() / b.norm()).item()
        ms = {"fused": [], "unfused": []}
        for k, lab in enumerate(labels):
            f, u, r = res["fused"][k], res["unfused"][k], res["f32"][k]
            ms["fused"].append(rel(f, r))
            ms["unfused"].append(rel(u, r))
            if lab in ("output", "d c_enc", "encode.weight", "blocks.0.layers.0.weight", "blocks.3.layers.6.weight", "decode.weight"):
                print(f"# {lab:26s} fused-unfused max-abs {(f - u).abs().max().item():.3e} rel-L2 {rel(f, u):.3e}  |  rel-L2 to fp32: "
                      f"fused {rel(f, r):.3e}  unfused {rel(u, r):.3e}")
        rms = lambda v: (sum(e * e for e in v) / len(v)) ** 0.5
        print(f"# rms over all {len(labels)} outputs / gradients of the rel-L2 to fp32: fused {rms(ms['fused']):.3e}  "
              f"unfused {rms(ms['unfused']):.3e}")
        del res
        net.zero_grad(set_to_none=True)

    def train_step(impl):
        # the HIP bf16 chain ends with the chosen optimiser ("fused/torch-opt": the same chain with the torch pair)
        opt = opts["fused" if impl == "fused" and args.optimizer != "torch" else "torch"]
        impl = impl.split("/")[0]

        def run():
            opt.zero_grad(set_to_none=True)
            if impl == "torch-f32" or impl == "torch-bf16":
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=impl == "torch-bf16"):
                    y = torch_forward(net, x3, c)
                loss = F.mse_loss(y.float(), t3)
            else:
                dt = torch.float32 if impl == "f32" else torch.bfloat16
                if impl == "unfused":
                    y = net.forward_unfused(net.state_input(x3, dt), net.encode_conditioning(C, dt))[..., :4].movedim(-1, 1)
                else:
                    y = net(x3.to(dt), C)
                loss = F.mse_loss(y, t3)
            loss.backward()
            if opt is opts["torch"]:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.1)
            opt.step()
        return run

    def rollout(impl, steps):
        @torch.no_grad()
        def run():
            if impl.startswith("torch"):
                xs = x8
                for _ in range(steps):
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=impl == "torch-bf16"):
                        y = torch_forward(net, xs, c).float()
                    xs = torch.where(inside, xs + mean.view(-1, 1, 1, 1) + std.view(-1, 1, 1, 1) * y, xs)
            elif impl == "unfused":
                ce = net.encode_conditioning(C, torch.bfloat16)
                xs = x8.movedim(1, -1).contiguous()
                for _ in range(steps):
                    y = net.forward_unfused(net.state_input(xs.movedim(-1, 1), torch.bfloat16), ce)[..., :4]
                    xs = torch.where(inside[..., None], xs + torch.addcmul(mean, std, y), xs)
            else:
                net.unroll(x8, C, inside, mean, std, steps, dtype=torch.float32 if impl == "f32" else torch.bfloat16)
        return run

    impls = ["fused", "unfused", "f32", "torch-bf16", "torch-f32"]
    if args.only:
        impls = [i for i in impls if i.startswith(args.only)]
    work = [("train B=3", lambda i: train_step(i)), ("rollout step B=8", lambda i: rollout(i, 1)),
            (f"unroll {args.steps} B=8", lambda i: rollout(i, args.steps))]
    for wname, make in work:
        # the 30-step unroll only for the two HIP bf16 paths: through MIOpen it would take minutes (the per-step row above
        # gives the others)
        w_impls = [i for i in impls if i in ("fused", "unfused")] if "unroll" in wname else list(impls)
        if wname.startswith("train") and args.optimizer == "both" and "fused" in w_impls:
            w_impls.insert(w_impls.index("fused") + 1, "fused/torch-opt")
        fns = {i: make(i) for i in w_impls}
        reps = 1 if "unroll" in wname else args.reps
        for i in w_impls:
            for _ in range(args.warmup if "unroll" not in wname else 1):
                fns[i]()
        times = {i: [] for i in w_impls}
        for _ in range(reps):  # alternate the implementations
            for i in w_impls:
                times[i] += timed(fns[i], 1)
        for i in w_impls:
            print(f"{wname:18s} {i:15s} {statistics.median(times[i]):10.2f} ms  (min {min(times[i]):.2f}, n {len(times[i])})")
    sys.stdout.flush()


if __name__ == "__main__":
    main()
