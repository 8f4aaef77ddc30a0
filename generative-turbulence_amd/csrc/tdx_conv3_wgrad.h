// What the weight-gradient kernels of the 3x3x3 convolution share (tdx_conv3_wgrad_*.hip):
//
//   dW[tap][ci][co] = sum_v x[clamp(v + tap)][ci] * dy[v][co]
//
// A TN GEMM per tap over the voxels of bricks (K = voxels, both operands voxel-major).  A workgroup owns a 32 (ci) x
// 32 NT (co) tile of all 27 taps and walks every nsplit-th brick; per brick the halo'd x brick and the dy brick are staged
// in LDS as rows of 32 channels.  This header holds the view of the grid the launcher passes in, the brick geometry, the
// decode of brick / halo-piece / tap indices and the lane geometry of the transposed fragment reads.  How a kernel stages
// (registers or LDS-DMA, one role or loader + computing waves), which MFMA it issues and how it merges stay in its file.
// So does the choice of the input tensor a ci tile reads (`if (ci0 < C1) { xs = x1; ... }`): behind a function, in any of
// the forms tried, the compiler schedules every one of these kernels differently (profiles/r16_wgrad_shared_header.txt).
#pragma once
#include "tdx_common.h"
#include "tdx_conv3.h"
#include "tdx_mfma.h"

// grid in the kernel's local axes (local axis k = global axis perm[k]; the brick's short edge is local axis 0, put where
// it leaves the fewest bricks)
struct WgradView {
    int B;
    int E[3];     // extents
    int s[3];     // voxel strides
    int ws[3];    // weight-tap strides: global tap = sum_k (e_k + 1) * ws[k]
    int nb[3];    // bricks per axis
    int batch;    // voxels per sample
};

// Launch geometry: bricks of bx x by x bz voxels in the kernel's LOCAL axes.  The three axis orders a kernel may run in
// (local axis k = grid axis WGRAD_ORDERS[order][k]):
static const int WGRAD_ORDERS[3][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}};
// the order that puts the short axis on the grid axis that leaves the fewest bricks (the first such; permute false: the
// grid's own order, 0): decided once, by the kernel's *_plan function
static inline int conv3_wgrad_view_order(const Conv3WgradCall& c, int bx, int by, int bz, bool permute = true) {
    const int E[3] = {c.X, c.Y, c.Z};
    int best = 0;
    int64_t best_n = -1;
    for (int k = 0; k < (permute ? 3 : 1); ++k) {
        const int64_t n = (int64_t)ceil_div(E[WGRAD_ORDERS[k][0]], bx) * ceil_div(E[WGRAD_ORDERS[k][1]], by) * ceil_div(E[WGRAD_ORDERS[k][2]], bz);
        if (best_n < 0 || n < best_n) { best_n = n; best = k; }
    }
    return best;
}
// the view of the grid in that order; returns the number of bricks
static inline int conv3_wgrad_view(WgradView& g, const Conv3WgradCall& c, int bx, int by, int bz, int order) {
    const int E[3] = {c.X, c.Y, c.Z}, gs[3] = {c.Y * c.Z, c.Z, 1}, gw[3] = {9, 3, 1}, bdim[3] = {bx, by, bz};
    g.B = c.B; g.batch = c.X * c.Y * c.Z;
    for (int k = 0; k < 3; ++k) {
        const int a = WGRAD_ORDERS[order][k];
        g.E[k] = E[a]; g.s[k] = gs[a]; g.ws[k] = gw[a]; g.nb[k] = ceil_div(E[a], bdim[k]);
    }
    return c.B * g.nb[0] * g.nb[1] * g.nb[2];
}

// voxel (x, y, z) in local axes of sample b -> row of the NDHWC tensors
__device__ __forceinline__ int64_t wgrad_voxel(const WgradView& gv, int b, int x, int y, int z) {
    return (int64_t)b * gv.batch + x * gv.s[0] + y * gv.s[1] + z * gv.s[2];
}

// Brick of BX x 8 x 8 voxels (BX = 4: 256 voxels, 600 with the halo; BX = 2: 128 and 400) and its LDS images: the halo'd
// x brick (BX + 2) x 10 x 10 and the dy brick, one row of ROW bytes per voxel (32 channels: 64 B of 16-bit words, 128 B
// of fp32).  4 x 8 x 8 with 64-B rows: x image 38 400 B, dy plane 16 384 B.
template <int BX_, int ROW_ = 64>
struct WgradBrick {
    static constexpr int BX = BX_, BY = 8, BZ = 8;
    static constexpr int HY = BY + 2, HZ = BZ + 2;
    static constexpr int ROW = ROW_;
    static constexpr int NVOX = BX * BY * BZ;
    static constexpr int NHALO = (BX + 2) * HY * HZ;
    static constexpr int XBYTES = NHALO * ROW;   // one image of the halo'd x brick
    static constexpr int GPLANE = NVOX * ROW;    // one 32-channel plane of the dy brick

    // row of the x image -> halo position
    __device__ __forceinline__ static void halo_coords(int hv, int& hx, int& hy, int& hz) {
        hx = hv / (HY * HZ);
        const int rem = hv - hx * (HY * HZ);
        hy = rem / HZ; hz = rem - hy * HZ;
    }
    // voxel of the tensor that halo position (hx, hy, hz) of brick (bx, by, bz) of sample b reads: clamped into the
    // grid (replicate padding)
    __device__ __forceinline__ static int64_t halo_source(const WgradView& gv, int b, int bx, int by, int bz, int hx, int hy,
                                                          int hz) {
        const int sx = min(max(bx * BX + hx - 1, 0), gv.E[0] - 1), sy = min(max(by * BY + hy - 1, 0), gv.E[1] - 1),
                  sz = min(max(bz * BZ + hz - 1, 0), gv.E[2] - 1);
        return wgrad_voxel(gv, b, sx, sy, sz);
    }
    // offset in rows of local tap 0 .. 26 inside the x image
    __device__ __forceinline__ static int tap_offset(int tap) {
        const int ex = tap / 9 - 1, ey = (tap / 3) % 3 - 1, ez = tap % 3 - 1;
        return (ex * HY + ey) * HZ + ez;
    }
};

// brick id -> brick coordinates; returns the sample index
__device__ __forceinline__ int wgrad_brick_coords(const WgradView& gv, int brick, int& bx, int& by, int& bz) {
    bz = brick % gv.nb[2]; brick /= gv.nb[2];
    by = brick % gv.nb[1]; brick /= gv.nb[1];
    bx = brick % gv.nb[0]; brick /= gv.nb[0];
    return brick;
}

// Lane geometry of the transposed fragment reads (16-bit operands, 64-B rows).  A K step is 16 voxel rows; lane group
// lane >> 4 reads rows 8 kh + q and + 4 (tr_frag's lo and hi), columns 16 (group & 1) + 4 p .. + 3.
struct WgradLane {
    int q;
    int col_off;  // byte offset of this lane's 4 columns in a row
    int kh;       // which 8-row half of the K step
};
__device__ __forceinline__ WgradLane wgrad_lane(int lane) {
    const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
    const int col_off = (16 * (g & 1) + 4 * p) * 2;
    const int kh = g >> 1;
    return WgradLane{q, col_off, kh};
}
// K step s of a brick is the 16 voxels (x = s >> 2, y = 2 (s & 3) + kh, z = q and q + 4).  Row of the x image that this
// lane's fragment starts at in step 0 for the tap at row offset toff = BR::tap_offset(tap): halo voxel (1, kh + 1, q + 1)
// + tap (the fragment's bytes: row * 64 + col_off); and the byte offset of step s from there
template <class BR>
__device__ __forceinline__ int wgrad_x_frag_row(const WgradLane& L, int toff) {
    return (BR::HY + L.kh + 1) * BR::HZ + (L.q + 1) + toff;
}
template <class BR>
__device__ __forceinline__ int wgrad_x_step_offset(int s) { return ((s >> 2) * BR::HY + 2 * (s & 3)) * BR::HZ * 64; }

// tap in local axes -> tap of the weight tensor
__device__ __forceinline__ int wgrad_global_tap(const WgradView& gv, int ltap) {
    return (ltap / 9) * gv.ws[0] + ((ltap / 3) % 3) * gv.ws[1] + (ltap % 3) * gv.ws[2];
}
