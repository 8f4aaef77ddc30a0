"""Shared by the flow-decomposition tests (test_flow_decompose_host.py, test_flow_decompose_gpu.py): the float64 torch
restatement of the four forward lines of include/tdx.h ("TF-Net flow decomposition"), the float64 numpy restatement of the
four backward formulas the kernel is written from, the NDHWC packing of the three stacks, and the launcher's tile rule of
csrc/tdx_flow_decompose.hip restated.

    u*[t]     = sum_d S[d] xx[t, f, v + d]        (outside the grid: 0)        t  = 0..T-1
    bar[t']   = sum_l w[l] u*[t' + l]                                           t' = 0..n-1, n = T - L + 1
    tilde[t'] = u*[L-1+t'] - bar[t']
    prime[t'] = xx[L-1+t'] - u*[L-1+t']

    d = gb - gt
    g*[t]  = sum_{t': 0 <= t-t' < L} w[t-t'] d[t']  +  [t >= L-1] (gt - gp)[t-L+1]
    gxx[t] = [t >= L-1] gp[t-L+1]  +  sum_d S[d] g*[t, f, v - d]
    dS[d]  = sum g*[t, f, v] xx[t, f, v + d]
    dw[l]  = sum d[t', f, v] u*[t'+l, f, v]
"""

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

# (T, L, F) of the issue's list; the first is the shipped configuration
CONFIGS = [(6, 4, 4), (4, 4, 4), (5, 4, 4), (6, 1, 4), (6, 4, 3)]
HOST_GRID = (7, 5, 6)
FIXTURE_GRID = (34, 18, 17)
MULTI_GRID = (6, 7, 19)  # by tile_geometry: two tiles and a ragged remainder along every axis (asserted in the host test)
GRIDS = [(1, 1, 1), (3, 1, 2), HOST_GRID, FIXTURE_GRID, MULTI_GRID]

# ---- the launcher's tile rule (csrc/tdx_flow_decompose.hip: fld_shape, fld_tile) ----------------------------------------

TILE = (4, 4, 16)  # voxels of a workgroup along X, Y, Z: one per thread, 256 threads
MAX_T, MAX_F, MAX_PLANES = 8, 8, 32
GRID_Y = 65535  # samples along the launch's y axis; a larger B continues along z, so B itself has no bound
MAX_TILES = 2**24 - 1  # tiles x 256 threads < 2^32, what one axis of a launch takes
TileGeometry = namedtuple("TileGeometry", "tiles remainder blocks")


def tile_geometry(grid, B=1):
    """Tiles per axis, the voxels of the last tile per axis that lie inside the grid (== TILE: not ragged), workgroups."""
    tiles = tuple(-(-e // t) for e, t in zip(grid, TILE))
    rem = tuple(e - (n - 1) * t for e, n, t in zip(grid, tiles, TILE))
    return TileGeometry(tiles, rem, B * tiles[0] * tiles[1] * tiles[2])


def supported(B, T, L, Fn, grid):
    X, Y, Z = grid
    return (1 <= B and 1 <= L <= T <= MAX_T and 1 <= Fn <= MAX_F and T * Fn <= MAX_PLANES and min(grid) >= 1
            and X * Y * Z < 2**31 and tile_geometry(grid).blocks <= MAX_TILES)


def up8(c):
    return -(-c // 8) * 8


# ---- float64 forward (torch, differentiable) ---------------------------------------------------------------------------

def spatial_filter(xx, S):
    """u* of xx (..., X, Y, Z) with S (3, 3, 3): cross-correlation, zero padding."""
    X, Y, Z = xx.shape[-3:]
    p = F.pad(xx, (1, 1, 1, 1, 1, 1))
    return sum(S[i, j, k] * p[..., i:i + X, j:j + Y, k:k + Z] for i in range(3) for j in range(3) for k in range(3))


def decompose_ref(xx, S, w):
    """float64 (bar, tilde, prime), each (B, n, F, X, Y, Z), of xx (B, T, F, X, Y, Z), S (3, 3, 3), w (L,)."""
    xx, S, w = xx.double(), S.double().reshape(3, 3, 3), w.double().reshape(-1)
    L = w.numel()
    n = xx.shape[1] - L + 1
    u = spatial_filter(xx, S)
    bar = sum(w[l] * u[:, l:l + n] for l in range(L))
    return bar, u[:, L - 1:] - bar, xx[:, L - 1:] - u[:, L - 1:]


def to_nvc(stack, cp=None):
    """(B, n, F, X, Y, Z) -> (B, X, Y, Z, cp): channel t' F + f, zero channels appended (cp: up8(n F))."""
    x = stack.flatten(1, 2).movedim(1, -1)
    cp = up8(x.shape[-1]) if cp is None else cp
    return F.pad(x, (0, cp - x.shape[-1])).contiguous()


def from_nvc(x, n, Fn):
    """The inverse on the real channels: (B, X, Y, Z, cp) -> (B, n, F, X, Y, Z)."""
    return x[..., :n * Fn].movedim(-1, 1).unflatten(1, (n, Fn))


# ---- float64 backward (numpy, the four formulas) -----------------------------------------------------------------------

def decompose_bwd_ref(xx, S, w, gb, gt, gp):
    """(gxx, dS (3, 3, 3), dw (L,)) in float64 from xx (B, T, F, X, Y, Z), S, w and the incoming gradients (B, n, F, X, Y, Z)."""
    xx, S, w, gb, gt, gp = (np.asarray(a, dtype=np.float64) for a in (xx, S, w, gb, gt, gp))
    S, w = S.reshape(3, 3, 3), w.reshape(-1)
    L, T = w.size, xx.shape[1]
    n = T - L + 1
    X, Y, Z = xx.shape[-3:]
    halo = [(0, 0)] * 3 + [(1, 1)] * 3
    d = gb - gt
    gs = np.zeros_like(xx)
    for t in range(T):
        for tp in range(n):
            if 0 <= t - tp < L:
                gs[:, t] += w[t - tp] * d[:, tp]
        if t >= L - 1:
            gs[:, t] += (gt - gp)[:, t - L + 1]
    pg, px = np.pad(gs, halo), np.pad(xx, halo)
    gxx = np.zeros_like(xx)
    gxx[:, L - 1:] += gp
    dS = np.zeros((3, 3, 3))
    u = np.zeros_like(xx)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                gxx += S[i, j, k] * pg[..., 2 - i:2 - i + X, 2 - j:2 - j + Y, 2 - k:2 - k + Z]  # g*[v - d], d = (i, j, k) - 1
                shifted = px[..., i:i + X, j:j + Y, k:k + Z]                                  # xx[v + d]
                dS[i, j, k] = np.sum(gs * shifted)
                u += S[i, j, k] * shifted
    dw = np.array([np.sum(d * u[:, l:l + n]) for l in range(L)])
    return gxx, dS, dw
