#!/usr/bin/env python3
"""The streaming GroupNorm entries at the U-Net's level-0 / level-1 shapes, B = 6, bf16: microseconds per call (two
measurements of 20 calls each) and the bandwidth over the entry's activation passes.
  tdx_gn_bwd            reduce pass + group pass + apply pass, act + FiLM: 5 passes
  tdx_gn_apply          act + residual: 3 passes
  tdx_gn_apply_encoded  192x64x48 x 64 channels only (D = 32 + c_raw): 2 passes + the raw planes
  tdx_gn_apply_decode   192x64x48 x 64 channels only: 2 passes + the 4 output planes
(Round 3 measured an apply pass that walks each sample back to front, so that what the reduce pass left in the 256 MiB
Infinity Cache is read first: 199 vs 192 us at 192x64x48 x 32 channels, 437 vs 431 at 64 channels -- no gain, not kept.)
GPU box: python tools/gn_bench.py [--lib <another build's libtdx_hip.so>]    (--lib sets TDX_LIB: A/B against that library)
         python tools/gn_bench.py --act 2    (TDX_ACT_*: 1 SiLU (default), 2 GELU, 3 ReLU, 4 Softplus, 5 Tanh; the two tails
                                              then go through their *_act entries)"""
import argparse, os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "generative-turbulence_amd"))
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--lib", help="libtdx_hip.so to measure instead of the package's own")
ap.add_argument("--act", type=int, default=1, help="TDX_ACT_* code of the activation")
args = ap.parse_args()
if args.lib:
    os.environ["TDX_LIB"] = str(Path(args.lib).resolve())  # read when turbdiff_amd._lib is imported
import torch
from turbdiff_amd import _lib as L

assert not args.lib or Path(L.LIB_PATH).resolve() == Path(args.lib).resolve(), L.LIB_PATH
print(f"library: {L.LIB_PATH}  act = {args.act}", flush=True)
ACT = args.act
TAIL = ("", ()) if ACT == 1 else ("_act", (ACT,))  # SiLU: the entries without an `act` argument
dev = torch.device("cuda:0")
B, G = 6, 8


def timed(go):
    out = []
    for rep in range(2):
        for _ in range(5): go()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): go()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / 20 * 1e3)
    return out


def report(name, grid, C, us, nbytes):
    cells = "  ".join(f"{u:7.1f} us ({nbytes / u / 1e6:5.2f} TB/s)" for u in us)
    print(f"{name} {grid[0]}x{grid[1]}x{grid[2]} C={C:3d} ({B * grid[0] * grid[1] * grid[2] * C * 2 / 1e6:.0f} MB per tensor): {cells}", flush=True)


for (grid, C) in (((192, 64, 48), 64), ((192, 64, 48), 32), ((96, 32, 24), 128), ((96, 32, 24), 64)):
    V = grid[0] * grid[1] * grid[2]
    x = torch.randn(B, V, C, device=dev).bfloat16(); dy = torch.randn(B, V, C, device=dev).bfloat16(); dx = torch.empty_like(x)
    f = lambda *s: torch.randn(*s, device=dev)
    gamma, beta, scale, shift = f(C), f(C), 0.1 * f(B, C), f(B, C)
    dg, db, ds, dsh = f(C), f(C), f(B, C), f(B, C)
    ws = torch.zeros(L.query("tdx_gn_workspace_bytes", B, C) + (1 << 24), dtype=torch.uint8, device=dev)
    stats = torch.empty(B, G, 2, device=dev)
    st = L.stream()
    L.call("tdx_gn_stats", L.ptr(x), L.ptr(stats), B, V, C, G, 1e-5, L.BF16, L.ptr(ws), st)
    act_bytes = x.numel() * 2
    report("gn_bwd", grid, C, timed(lambda: L.call(
        "tdx_gn_bwd", L.ptr(x), L.ptr(dy), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(scale), L.ptr(shift), L.ptr(dx), L.ptr(dg),
        L.ptr(db), L.ptr(ds), L.ptr(dsh), B, V, C, G, ACT, L.BF16, L.ptr(ws), st)), 5 * act_bytes)
    report("gn_apply", grid, C, timed(lambda: L.call(
        "tdx_gn_apply", L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(beta), None, None, L.ptr(dy), L.ptr(dx), B, V, C, G, ACT, L.BF16,
        st)), 3 * act_bytes)
    if (grid, C) != ((192, 64, 48), 64):
        continue
    D = C // 2
    xr, cr, wx, wc, bx, bc = f(B, 4, V), f(4, V), f(D, 4), f(D, 4), f(D), f(D)
    report("gn_apply_encoded", grid, C, timed(lambda: L.call(
        "tdx_gn_apply_encoded" + TAIL[0], L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(xr), 4, L.ptr(wx), L.ptr(bx), L.ptr(cr), 4,
        L.ptr(wc), L.ptr(bc), L.ptr(dx), B, V, D, G, L.BF16, *TAIL[1], st)), 2 * act_bytes + (B + 1) * 4 * V * 4)
    w, bias, out = f(4, C), f(4), torch.empty(B, 4, V, device=dev)
    report("gn_apply_decode", grid, C, timed(lambda: L.call(
        "tdx_gn_apply_decode" + TAIL[0], L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(dy), L.ptr(w), L.ptr(bias), L.ptr(out), B, V,
        C, G, 4, L.BF16, *TAIL[1], st)), 2 * act_bytes + B * 4 * V * 4)
