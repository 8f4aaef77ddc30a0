#!/usr/bin/env python3
"""TF-Net on one MI355X: a training step (B = 8, unroll 4) and one eval rollout step (B = 16) of the shipped configuration
(config/model/tfnet.yaml: context 6, temporal filter 4, kernel 3) on the shapes dataset's 194 x 50 x 50 grid, synthetic
seeded data, the implementations timed alternately in one process after warm-up:

  fused      bf16, every ConvBlock tail on ops.batch_norm_act (csrc/tdx_batchnorm.hip) and the flow decomposition on
             ops.flow_decompose (csrc/tdx_flow_decompose.hip), the default
  decomp-off bf16, tfnet.FUSE_DECOMPOSE = False: LES.decompose + three _to_nvc_padded calls in torch, tails fused
  unfused    bf16, baseline_convs.FUSE_BATCHNORM = False: F.batch_norm + F.leaky_relu + casts + adds in torch
  f32        the fp32 parity path (vector-ALU convg kernels), fused tails
  torch      (--torch) stock PyTorch-ROCm nn modules, bf16 autocast and fp32, NCDHW

and the BatchNorm tail alone at each level's shape, fused against the torch sequence, forward (statistics + apply) and
backward: between HIP events on the stream (launch gaps and the (C,)-sized running-statistics ops included), median and min-max
over --tail-reps alternating runs; and the kernel time alone (sum of the device-kernel durations from torch.profiler).  The
bytes the passes must move (computed from the shapes below) over either time are set against the HBM roof (8.0 TB/s spec; a
float4 copy reaches 6.3).  The flow decomposition alone is measured the same way (kernel time of the torch chain against the
op: forward at the eval batch, forward + backward at the training batch with and without a gradient to xx), each step prints
its peak memory per implementation, and the chain's kernel time is set against the step of the torch route.

    python tools/tfnet_bench.py [--reps 3] [--train-batch 8] [--eval-batch 16] [--unroll 4] [--torch]
                                [--skip-tails] [--skip-decompose] [--skip-model] [--impls fused,decomp-off,unfused,f32]

GPU only: exits with an error without one.
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
from torch import nn  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
GRID = (194, 50, 50)
CFG = dict(n_features=4, c_local_features=8, c_global_features=0, context_window=6, kernel_size=3, dropout_rate=0.0,
           temporal_filtering_length=4)


def kernel_source_hash():
    h = hashlib.sha256()
    for p in sorted((ROOT / "generative-turbulence_amd" / "csrc").glob("*.h*")):
        h.update(p.read_bytes())
    return h.hexdigest()[:16]


class TorchLES(nn.Module):
    """The same network from stock nn modules (NCDHW), sharing the parameters of a turbdiff_amd LES."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    @staticmethod
    def _seq(blk, x):
        for layer in blk:
            x = layer(x)
        return x

    def forward(self, xx, c_local):
        m = self.m
        bar, tilde, prime = m.decompose(xx)
        outs = []
        for enc, u in zip(m.encoders, (bar, tilde, prime)):
            o1 = self._seq(enc.conv1, u) + self._seq(enc.conv1_local, c_local[None])
            o2 = self._seq(enc.conv2, o1)
            o3 = self._seq(enc.conv3, o2)
            outs.append((o1, o2, o3, self._seq(enc.conv4, o3)))
        o1, o2, o3, o4 = (a + b + c for a, b, c in zip(*outs))
        clip = lambda a, b: a[..., :b.shape[-3], :b.shape[-2], :b.shape[-1]]
        d3 = self._seq(m.deconv3, o4)
        d2 = self._seq(m.deconv2, o3 + clip(d3, o3))
        d1 = self._seq(m.deconv1, o2 + clip(d2, o2))
        d0 = self._seq(m.deconv0, o1 + clip(d1, o1))
        return m.output_layer(clip(d0, xx))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_ms(fn, reps=5):
    """Sum of the device-kernel durations of one call of fn (the profiler's device activity records), median over reps; None
    where the profiler delivers no device records."""
    from torch.profiler import ProfilerActivity, profile

    out = []
    try:
        for _ in range(reps):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            us = sum(e.device_time_total for e in prof.key_averages())  # microseconds
            if us <= 0:
                return None
            out.append(us * 1e-3)
    except Exception as exc:  # noqa: BLE001 -- a profiler that cannot start must not end the benchmark
        print(f"# profiler unavailable ({type(exc).__name__}: {exc}): kernel times not measured")
        return None
    return statistics.median(out)


def level_shapes(batch):
    """(name, rows, C) of every BatchNorm tail of one model call: the four encoder levels (stride-2 convs, padding 1:
    extent e -> (e + 1) // 2) at `batch` samples, and the conditioning branch at batch 1."""
    half = lambda e: (e + 1) // 2
    g, out = GRID, []
    for lvl, C in enumerate((64, 128, 256, 512), 1):
        g = tuple(half(e) for e in g)
        out.append((f"level {lvl}", batch * g[0] * g[1] * g[2], C, g))
    g1 = tuple(half(e) for e in GRID)
    out.insert(1, ("conv1_local", g1[0] * g1[1] * g1[2], 64, g1))
    return out


def tail_bytes(rows, C, es):
    """Bytes the tail must move: forward = statistics pass reads x, apply pass reads x and writes y; backward = reduce pass
    reads x and dy, apply pass reads x and dy and writes dx.  (Parameters and the (C, 2) tables are negligible.)"""
    n = rows * C * es
    return 3 * n, 5 * n


def bench_tails(args, dev):
    from turbdiff_amd.models import baseline_convs

    print(f"# BatchNorm tail alone, bf16, training mode, B = {args.train_batch}: ms median [min-max] over {args.tail_reps} "
          f"alternating runs (HIP events); fused GB/s = bytes moved / time, share of the {HBM_SPEC / 1e12:.1f} TB/s spec roof "
          f"(copy roof {HBM_COPY / 1e12:.1f} TB/s)")
    for name, rows, C, g in level_shapes(args.train_batch):
        B = 1 if name == "conv1_local" else args.train_batch
        x = torch.randn(B, *g, C, device=dev).to(torch.bfloat16)
        dy = torch.randn_like(x)
        blk = baseline_convs.ConvBlock(8, C, 3, 2, 0.0).to(dev).train()

        def run(fused):
            baseline_convs.FUSE_BATCHNORM = fused
            xl = x.detach().requires_grad_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            y = blk.tail(xl)
            ev[1].record()
            y.backward(dy)
            ev[2].record()
            torch.cuda.synchronize()
            blk.zero_grad(set_to_none=True)
            return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

        for fused in (True, False):
            run(fused), run(fused)
        t = {True: ([], []), False: ([], [])}
        for _ in range(args.tail_reps):
            for fused in (True, False):
                f, b = run(fused)
                t[fused][0].append(f)
                t[fused][1].append(b)
        # kernel-only time of each direction: the device records of a forward alone, and of forward + backward
        kt = {}
        for fused in (True, False):
            baseline_convs.FUSE_BATCHNORM = fused

            def fwd():
                with torch.no_grad():
                    blk.tail(x)

            def both():
                xl = x.detach().requires_grad_()
                blk.tail(xl).backward(dy)
                blk.zero_grad(set_to_none=True)

            kf, kb = kernel_ms(fwd), kernel_ms(both)
            kt[fused] = (kf, None if kf is None or kb is None else kb - kf)
        baseline_convs.FUSE_BATCHNORM = True
        fb, bb = tail_bytes(rows, C, 2)
        for i, (what, nbytes) in enumerate((("fwd", fb), ("bwd", bb))):
            mf, mu = statistics.median(t[True][i]), statistics.median(t[False][i])
            rate = nbytes / (mf * 1e-3)
            print(f"tail {name:11s} rows {rows:8d} C {C:3d} {what}: fused {mf:7.3f} [{min(t[True][i]):.3f}-{max(t[True][i]):.3f}]  "
                  f"torch {mu:7.3f} [{min(t[False][i]):.3f}-{max(t[False][i]):.3f}]  x{mu / mf:5.2f}  "
                  f"{nbytes / 1e6:8.1f} MB -> {rate / 1e9:7.0f} GB/s = {100 * rate / HBM_SPEC:4.1f} % of spec, "
                  f"{100 * rate / HBM_COPY:4.1f} % of copy")
            kf, ku = kt[True][i], kt[False][i]
            if kf is None or ku is None:
                print(f"tail {name:11s} {what} kernel time: not measured")
            else:
                krate = nbytes / (kf * 1e-3)
                print(f"tail {name:11s} {what} kernel time: fused {kf:7.4f}  torch {ku:7.4f}  x{ku / kf:5.2f}  -> {krate / 1e9:7.0f} GB/s = "
                      f"{100 * krate / HBM_SPEC:4.1f} % of spec, {100 * krate / HBM_COPY:4.1f} % of copy")
        sys.stdout.flush()


def decompose_bytes(B, V, es, backward=False, gxx=False):
    """Bytes the decomposition must move: xx read once, three Cp-channel grids written; the backward adds the three gradient
    grids read and, with a gradient to xx, gxx written.  (The backward's second read of xx for the recomputed u* is not
    counted: it is the price of saving nothing.)"""
    T, Fn, Ln = CFG["context_window"], CFG["n_features"], CFG["temporal_filtering_length"]
    cp = -(-(T - Ln + 1) * Fn // 8) * 8
    n = B * T * Fn * V * 4 + 3 * B * V * cp * es
    if backward:
        n += 3 * B * V * cp * es + (B * T * Fn * V * 4 if gxx else 0)
    return n


def bench_decompose(args, dev, net):
    """The decomposition + layout chain (LES.decompose + three _to_nvc_padded, autograd) against ops.flow_decompose, bf16:
    kernel time (device records) of both routes, alternating.  Returns {case: (chain ms, op ms)}."""
    from turbdiff_amd import ops
    from turbdiff_amd.models.dilresnet import _to_nvc_padded, _up8

    T, Fn = CFG["context_window"], CFG["n_features"]
    V = GRID[0] * GRID[1] * GRID[2]
    sw, tw = net.spatial_filter.weight, net.temporal_filter.weight
    dt = torch.bfloat16

    def chain(xx):
        stacks = net.decompose(xx)
        return tuple(_to_nvc_padded(u, _up8(u.shape[1]), dt) for u in stacks)

    def op(xx):
        return ops.flow_decompose(xx, sw, tw, dt)

    print(f"# flow decomposition at {GRID}, T = {T}, L = {CFG['temporal_filtering_length']}, F = {Fn}, bf16: kernel time (sum of the "
          f"device records), median [min-max] over {args.decompose_reps} alternating runs; bytes = xx + 3 grids (+ 3 gradient grids "
          f"+ gxx), over the op's time against the {HBM_SPEC / 1e12:.1f} TB/s spec roof and the {HBM_COPY / 1e12:.1f} TB/s copy roof")
    out = {}
    cases = (("fwd", args.eval_batch, False, False), ("fwd+bwd, gxx", args.train_batch, True, True),
             ("fwd+bwd, no gxx", args.train_batch, True, False))
    for name, B, backward, gxx in cases:
        g = torch.Generator(device=dev).manual_seed(7)
        xx = torch.randn(B, T, Fn, *GRID, device=dev, generator=g)
        grads = None
        if backward:
            cp = _up8((T - CFG["temporal_filtering_length"] + 1) * Fn)
            grads = [torch.randn(B, *GRID, cp, device=dev, generator=g).to(dt) for _ in range(3)]

        def run(route):
            def fn():
                if not backward:
                    with torch.no_grad():
                        route(xx)
                    return
                xl = xx.detach().requires_grad_(gxx)
                torch.autograd.backward(route(xl), grads)
                net.spatial_filter.weight.grad = net.temporal_filter.weight.grad = None
            return fn

        fns = {"chain": run(chain), "op": run(op)}
        for f in fns.values():
            f(), f()
        ms = {k: [] for k in fns}
        for _ in range(args.decompose_reps):
            for k, f in fns.items():
                t = kernel_ms(f, reps=1)
                if t is not None:
                    ms[k].append(t)
        if not ms["chain"] or not ms["op"]:
            print(f"decompose {name:16s} B {B:2d}: kernel time not measured")
            continue
        mc, mo = statistics.median(ms["chain"]), statistics.median(ms["op"])
        nbytes = decompose_bytes(B, V, 2, backward, gxx)
        rate = nbytes / (mo * 1e-3)
        print(f"decompose {name:16s} B {B:2d}: chain {mc:8.3f} [{min(ms['chain']):.3f}-{max(ms['chain']):.3f}]  op {mo:7.3f} "
              f"[{min(ms['op']):.3f}-{max(ms['op']):.3f}]  x{mc / mo:5.2f}  {nbytes / 1e6:8.1f} MB -> {rate / 1e9:6.0f} GB/s = "
              f"{100 * rate / HBM_SPEC:4.1f} % of spec, {100 * rate / HBM_COPY:4.1f} % of copy")
        out[name] = (mc, mo)
        del xx, grads
        sys.stdout.flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tail-reps", type=int, default=9)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--eval-batch", type=int, default=16)
    ap.add_argument("--unroll", type=int, default=4)
    ap.add_argument("--torch", action="store_true", help="also time stock PyTorch-ROCm nn modules (bf16 autocast and fp32)")
    ap.add_argument("--decompose-reps", type=int, default=5)
    ap.add_argument("--skip-tails", action="store_true", help="skip the BatchNorm tails")
    ap.add_argument("--skip-decompose", action="store_true", help="skip the flow decomposition alone")
    ap.add_argument("--skip-model", action="store_true", help="only the BatchNorm tails and the flow decomposition")
    ap.add_argument("--impls", default="fused,decomp-off,unfused,f32", help="comma list of the HIP implementations to time")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tfnet_bench.py needs a GPU")
    from turbdiff_amd.models import baseline_convs, tfnet
    from turbdiff_amd.models.conditioning import Conditioning
    from turbdiff_amd.models.tfnet import LES
    from turbdiff_amd.optim import ClipAdam

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"# kernel-source hash {kernel_source_hash()}  torch {torch.__version__}  device {torch.cuda.get_device_name(0)}")
    print(f"# grid {GRID}, train B = {args.train_batch} unroll {args.unroll}, eval B = {args.eval_batch}")
    if not args.skip_tails:
        bench_tails(args, dev)
    net = LES(**CFG).to(dev)
    with torch.no_grad():  # the reference's 0.002 / n initialisation gives activations of 1e-9: use visible weights
        for p in net.parameters():
            if p.ndim == 5:
                p.normal_(0, (1.0 / p[0].numel()) ** 0.5)
    chain = {} if args.skip_decompose else bench_decompose(args, dev, net)
    if args.skip_model:
        return
    tnet = TorchLES(net)
    opt = ClipAdam(net.parameters(), lr=1e-7, max_norm=None)
    g = torch.Generator(device=dev).manual_seed(1)
    T, Fn = CFG["context_window"], CFG["n_features"]
    c = torch.randn(8, *GRID, device=dev, generator=g)
    C = {Conditioning.Type.CELL_TYPE: c}
    inside = torch.rand(*GRID, device=dev, generator=g) > 0.1
    xt = torch.randn(args.train_batch, T, Fn, *GRID, device=dev, generator=g)
    tt = torch.randn(args.train_batch, args.unroll, Fn, *GRID, device=dev, generator=g)
    xe = torch.randn(args.eval_batch, T, Fn, *GRID, device=dev, generator=g)

    def model(impl, xx):
        if impl.startswith("torch"):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=impl == "torch-bf16"):
                return tnet(xx, c).float()
        baseline_convs.FUSE_BATCHNORM = impl != "unfused"
        tfnet.FUSE_DECOMPOSE = impl != "decomp-off"
        try:
            return net(xx, C, dtype=torch.float32 if impl == "f32" else torch.bfloat16)
        finally:
            baseline_convs.FUSE_BATCHNORM = True
            tfnet.FUSE_DECOMPOSE = fuse_decompose_default

    def unroll(impl, xx, steps):
        out = []
        for _ in range(steps):
            x_i = torch.where(inside, model(impl, xx), xx[:, -1])
            out.append(x_i)
            xx = torch.cat((xx[:, 1:], x_i.unsqueeze(1)), dim=1)
        return torch.stack(out, dim=1)

    def train_step(impl):
        def run():
            net.train()
            opt.zero_grad(set_to_none=True)
            F.mse_loss(unroll(impl, xt, args.unroll), tt).backward()
            opt.step()
        return run

    def eval_step(impl):
        @torch.no_grad()
        def run():
            net.eval()
            unroll(impl, xe, 1)
        return run

    fuse_decompose_default = tfnet.FUSE_DECOMPOSE
    print(f"# fused = bf16, FUSE_BATCHNORM and FUSE_DECOMPOSE on; decomp-off = fused with tfnet.FUSE_DECOMPOSE = False (LES.decompose + "
          f"_to_nvc_padded in torch); shipped default FUSE_DECOMPOSE = {fuse_decompose_default}")
    impls = args.impls.split(",") + (["torch-bf16", "torch-f32"] if args.torch else [])
    for wname, make in ((f"train B={args.train_batch} unroll {args.unroll}", train_step), (f"eval step B={args.eval_batch}", eval_step)):
        fns = {i: make(i) for i in impls}
        times = {i: [] for i in impls}
        for i in impls:
            for _ in range(args.warmup):
                fns[i]()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fns[i]()
            torch.cuda.synchronize()
            print(f"{wname:22s} {i:11s} peak memory {torch.cuda.max_memory_allocated() / 2**30:7.2f} GiB")
        for _ in range(args.reps):  # alternate the implementations
            for i in impls:
                times[i].append(timed(fns[i]))
        for i in impls:
            print(f"{wname:22s} {i:11s} {statistics.median(times[i]):10.2f} ms  [min {min(times[i]):.2f} max {max(times[i]):.2f}, n {len(times[i])}]")
        for other in ("unfused", "decomp-off"):
            if not {"fused", other} <= set(impls):
                continue
            f, u = times["fused"], times[other]
            print(f"{wname:22s} {other} - fused = {statistics.median(u) - statistics.median(f):.2f} ms; run-to-run spread: fused "
                  f"{max(f) - min(f):.2f} ms, {other} {max(u) - min(u):.2f} ms")
        if "decomp-off" in impls and chain:  # the chain's share of the step on the torch route (kernel time over wall time)
            if make is train_step and {"fwd+bwd, gxx", "fwd+bwd, no gxx"} <= set(chain):
                ms = chain["fwd+bwd, no gxx"][0] + (args.unroll - 1) * chain["fwd+bwd, gxx"][0]
            elif make is eval_step and "fwd" in chain:
                ms = chain["fwd"][0]
            else:
                ms = None
            if ms is not None:
                step = statistics.median(times["decomp-off"])
                print(f"{wname:22s} decomposition + layout chain on the torch route: {ms:.2f} ms of kernel time = {100 * ms / step:.1f} % "
                      f"of the {step:.2f} ms step")
        sys.stdout.flush()
    print(f"# peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    main()
