// Trilinear resize, align_corners=True, NDHWC (ddpm.py:359-361, 367-369).
// HBM-bound gather kernels: one lane owns 8 channels of one voxel (16 B bf16 / 32 B f32).
// A workgroup owns a compact 4 x 8 x 8 tile of the tensor it WRITES, so that the voxels it gathers
// from form a small 3D region that stays in the CU's L1 (a linear thread->voxel map re-fetched every
// gathered voxel ~17x from L2); all loads of a thread are issued before the arithmetic.
// Index arithmetic follows ATen's upsample_trilinear3d exactly (float scale, float source
// index, truncation, clamped second tap) so that tap selection matches the reference.
//
// Host side: resize_plan decides, once per call, everything a launch depends on; tdx_resize_fwd, tdx_resize_bwd and the
// query tdx_resize_plan read that plan and hold no condition of their own.  The forward evaluates only the forward half
// of the plan (no spans) and the adjoint only the adjoint half (no pair windows); the query evaluates both.
#include "tdx_common.h"

struct AxisMap {
    int in, out;
    float scale;
};
__host__ __device__ inline AxisMap make_axis(int in, int out) {
    AxisMap a;
    a.in = in; a.out = out;
    a.scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    return a;
}
// taps of output index o: i0, i1, weight of i1
__host__ __device__ __forceinline__ void axis_taps(const AxisMap& a, int o, int& i0, int& i1, float& w1) {
    const float src = a.scale * (float)o;
    i0 = min((int)src, a.in - 1);
    w1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
    i1 = i0 + ((i0 + 1 < a.in) ? 1 : 0);
}

// tile of the written grid owned by one workgroup: tx x ty x tz voxels (powers of two, <= 4 x 8 x 8),
// shrunk for wide channel counts so that a workgroup makes at most ~8 passes of 256 lanes
struct TileGrid {
    int nx, ny, nz;     // tiles per axis
    int sy, sz;         // log2(ty), log2(tz)
    int tx, ty, tz;
};
#define RS_MAXT 8   // largest tile extent along an axis
#define RS_KMAX 12  // largest number of outputs reading one input along an axis (backward)

__device__ __forceinline__ void tile_origin(const TileGrid& tg, int& b, int& x0, int& y0, int& z0) {
    int t = blockIdx.x;
    z0 = (t % tg.nz) * tg.tz; t /= tg.nz;
    y0 = (t % tg.ny) * tg.ty; t /= tg.ny;
    x0 = (t % tg.nx) * tg.tx;
    b = t / tg.nx;
}
// the map of axis a (0: x, 1: y, 2: z) and the tile's origin along it, for the few threads that fill the LDS tables
__device__ __forceinline__ const AxisMap& tile_axis(int a, const AxisMap& ax, const AxisMap& ay, const AxisMap& az, int x0,
                                                    int y0, int z0, int& origin) {
    origin = a == 0 ? x0 : (a == 1 ? y0 : z0);
    return a == 0 ? ax : (a == 1 ? ay : az);
}
// lane split of a workgroup: lane lc of C / 8 owns 8 channels of slot0, slot0 + per_pass, ...; false for the idle lanes
// past the last whole slot of a pass
__device__ __forceinline__ bool lane_split(int C, int& lc, int& per_pass, int& slot0) {
    const int L = C >> 3;
    per_pass = 256 / L; lc = (int)threadIdx.x % L; slot0 = (int)threadIdx.x / L;
    return (int)threadIdx.x < per_pass * L;
}
// slot -> voxel of the tile, z fastest (the pair kernel's slots are 2 x 2 x 2 blocks: it divides by its half extents)
__device__ __forceinline__ void slot_voxel(const TileGrid& tg, int slot, int& kx, int& ky, int& kz) {
    kz = slot & (tg.tz - 1); ky = (slot >> tg.sz) & (tg.ty - 1); kx = slot >> (tg.sz + tg.sy);
}
template <typename T>
__device__ __forceinline__ void store_acc(const float (&acc)[8], T* p) {
    Vec8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = acc[j];
    o.store(p);
}
// the adjoints' tail: dx = acc (+ add, a second gradient of the resampled tensor -- its use as a U-Net skip), one store
template <typename T>
__device__ __forceinline__ void store_adjoint(float (&acc)[8], const T* add, T* dx, int64_t di) {
    if (add != nullptr) {
        Vec8<T> a;
        a.load(add + di);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += a.v[j];
    }
    store_acc(acc, dx + di);
}

// Per-axis interpolation tables of the tile live in LDS: they are computed once per workgroup by a
// few threads instead of once per lane (the index arithmetic, not the gather, was the bottleneck).
template <typename T>
__global__ void __launch_bounds__(256)
resize_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, AxisMap ax, AxisMap ay, AxisMap az, int C, TileGrid tg) {
    __shared__ int s_i0[3][RS_MAXT], s_i1[3][RS_MAXT];
    __shared__ float s_w[3][RS_MAXT];
    int b, ox0, oy0, oz0;
    tile_origin(tg, b, ox0, oy0, oz0);
    if (threadIdx.x < 3 * RS_MAXT) {
        const int a = threadIdx.x / RS_MAXT, k = threadIdx.x % RS_MAXT;
        int o0, i0, i1;
        const AxisMap& m = tile_axis(a, ax, ay, az, ox0, oy0, oz0, o0);
        const int o = min(o0 + k, m.out - 1);
        float w1;
        axis_taps(m, o, i0, i1, w1);
        s_i0[a][k] = i0; s_i1[a][k] = i1; s_w[a][k] = w1;
    }
    __syncthreads();
    const int nvox = tg.tx * tg.ty * tg.tz;
    int lc, per_pass, slot0, kx, ky, kz;
    if (!lane_split(C, lc, per_pass, slot0)) return;
    for (int slot = slot0; slot < nvox; slot += per_pass) {
        slot_voxel(tg, slot, kx, ky, kz);
        const int ox = ox0 + kx, oy = oy0 + ky, oz = oz0 + kz;
        if (ox >= ax.out || oy >= ay.out || oz >= az.out) continue;
        const float wx = s_w[0][kx], wy = s_w[1][ky], wz = s_w[2][kz];
        const T* xb = x + ((int64_t)b * ax.in * ay.in * az.in) * C + lc * 8;
        const int xs[2] = {s_i0[0][kx], s_i1[0][kx]}, ys[2] = {s_i0[1][ky], s_i1[1][ky]}, zs[2] = {s_i0[2][kz], s_i1[2][kz]};
        const float wxs[2] = {1.0f - wx, wx}, wys[2] = {1.0f - wy, wy}, wzs[2] = {1.0f - wz, wz};
        Raw8<T> t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            t[k].load(xb + (((int64_t)xs[k >> 2] * ay.in + ys[(k >> 1) & 1]) * az.in + zs[k & 1]) * C);
        __builtin_amdgcn_sched_barrier(0);
        float acc[8] = {};
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // x outer, y, z inner
            const float w = wxs[k >> 2] * wys[(k >> 1) & 1] * wzs[k & 1];
            const Vec8<T> v = t[k].get();
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += w * v.v[j];
        }
        store_acc(acc, y + ((((int64_t)b * ax.out + ox) * ay.out + oy) * az.out + oz) * C + lc * 8);
    }
}

// ---- up-sampling, 2 x 2 x 2 outputs per lane ---------------------------------------------------------------------------
// When the grid grows along every axis (the U-Net's up path: 96 x 32 x 24 -> 192 x 64 x 48), the two outputs 2k and 2k + 1
// of an axis read taps inside one window of three inputs [base, base + 2], base = i0(2k) (host-checked per axis with the
// kernel's own float arithmetic, pair_window_ok).  A lane then produces a 2 x 2 x 2 block of outputs for its 8 channels from
// the 3 x 3 x 3 window -- 27 loads for 8 outputs instead of 64 -- interpolating separably (z, then y, then x).  Unused
// window entries carry weight 0 and a clamped address.  Worth 5-9 % at 192 x 64 x 48 x 64 (2.4 -> 2.6 TB/s of stores; a
// plain write-only stream reaches 4.8-6.5 TB/s, profiles/r11_hbm_write_probe.txt): with 216 VGPRs the kernel now waits on
// its three rounds of L2-latency loads at two waves per SIMD instead of on the L1 load rate; longer z runs per tile
// (2 x 8 x 16 ... 2 x 2 x 64) were measured and are no faster.
struct PairTaps {
    int base;
    float w[2][3];  // w[output of the pair][window entry]
};
__host__ __device__ __forceinline__ bool pair_taps(const AxisMap& a, int o_even, PairTaps& p) {
    int i0, i1;
    float w1;
    axis_taps(a, min(o_even, a.out - 1), i0, i1, w1);
    p.base = i0;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int s = 0; s < 3; ++s) p.w[q][s] = 0.f;
        const int o = min(o_even + q, a.out - 1);
        axis_taps(a, o, i0, i1, w1);
        const int d0 = i0 - p.base, d1 = i1 - p.base;
        ok = ok && d0 >= 0 && d0 <= 2 && d1 >= 0 && d1 <= 2;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (s == d0) p.w[q][s] += 1.0f - w1;
            if (s == d1) p.w[q][s] += w1;
        }
    }
    return ok;
}
static bool pair_window_ok(const AxisMap& a) {
    if (a.out < a.in) return false;
    PairTaps p;
    for (int o = 0; o < a.out; o += 2)
        if (!pair_taps(a, o, p)) return false;
    return true;
}

// (256, 3): three workgroups per CU = three waves per SIMD, i.e. at most 168 VGPRs -- the fp16 instantiation came out at 169
// (two waves per SIMD: 185 -> 309 us on the level-0 up-sampling) without the bound
template <typename T>
__global__ void __launch_bounds__(256, 3)
resize_up_pairs_kernel(const T* __restrict__ x, T* __restrict__ y, AxisMap ax, AxisMap ay, AxisMap az, int C, TileGrid tg) {
    __shared__ PairTaps s_p[3][RS_MAXT / 2];
    int b, ox0, oy0, oz0;
    tile_origin(tg, b, ox0, oy0, oz0);  // tile extents are even (host-checked), so pairs never straddle tiles
    if (threadIdx.x < 3 * (RS_MAXT / 2)) {
        const int a = threadIdx.x / (RS_MAXT / 2), k = threadIdx.x % (RS_MAXT / 2);
        int o0;
        const AxisMap& m = tile_axis(a, ax, ay, az, ox0, oy0, oz0, o0);
        PairTaps p;
        pair_taps(m, o0 + 2 * k, p);
        s_p[a][k] = p;
    }
    __syncthreads();
    int lc, per_pass, slot0;
    if (!lane_split(C, lc, per_pass, slot0)) return;
    const int px = tg.tx >> 1, py = tg.ty >> 1, pz = tg.tz >> 1;
    const int nblk = px * py * pz;
    for (int slot = slot0; slot < nblk; slot += per_pass) {
        const int kz = slot % pz, ky = (slot / pz) % py, kx = slot / (pz * py);
        const int ox = ox0 + 2 * kx, oy = oy0 + 2 * ky, oz = oz0 + 2 * kz;
        if (ox >= ax.out || oy >= ay.out || oz >= az.out) continue;
        const PairTaps tx = s_p[0][kx], ty = s_p[1][ky], tz = s_p[2][kz];
        const T* xb = x + ((int64_t)b * ax.in * ay.in * az.in) * C + lc * 8;
        int zi[3], yi[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            zi[s] = min(tz.base + s, az.in - 1);
            yi[s] = min(ty.base + s, ay.in - 1);
        }
        float acc[2][2][2][8];  // [x out][y out][z out][channel]
#pragma unroll
        for (int i = 0; i < 64; ++i) (&acc[0][0][0][0])[i] = 0.f;
#pragma unroll 1  // one x plane of the window at a time: 9 loads in flight, ~170 VGPRs instead of 256
        for (int sx = 0; sx < 3; ++sx) {
            const int xi = min(tx.base + sx, ax.in - 1);
            Raw8<T> t[3][3];
#pragma unroll
            for (int sy = 0; sy < 3; ++sy)
#pragma unroll
                for (int sz = 0; sz < 3; ++sz) t[sy][sz].load(xb + (((int64_t)xi * ay.in + yi[sy]) * az.in + zi[sz]) * C);
            // along z: rows[sy][z out]
            float rz[3][2][8];
#pragma unroll
            for (int sy = 0; sy < 3; ++sy) {
                const Vec8<T> v0 = t[sy][0].get(), v1 = t[sy][1].get(), v2 = t[sy][2].get();
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        rz[sy][q][j] = tz.w[q][0] * v0.v[j] + tz.w[q][1] * v1.v[j] + tz.w[q][2] * v2.v[j];
            }
            // along y, then into the two x outputs
#pragma unroll
            for (int qy = 0; qy < 2; ++qy)
#pragma unroll
                for (int qz = 0; qz < 2; ++qz)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float r = ty.w[qy][0] * rz[0][qz][j] + ty.w[qy][1] * rz[1][qz][j] + ty.w[qy][2] * rz[2][qz][j];
                        acc[0][qy][qz][j] += tx.w[0][sx] * r;
                        acc[1][qy][qz][j] += tx.w[1][sx] * r;
                    }
        }
#pragma unroll
        for (int qx = 0; qx < 2; ++qx)
#pragma unroll
            for (int qy = 0; qy < 2; ++qy)
#pragma unroll
                for (int qz = 0; qz < 2; ++qz) {
                    if (ox + qx >= ax.out || oy + qy >= ay.out || oz + qz >= az.out) continue;
                    store_acc(acc[qx][qy][qz], y + ((((int64_t)b * ax.out + ox + qx) * ay.out + oy + qy) * az.out + oz + qz) * C + lc * 8);
                }
    }
}

// range [lo, hi] of outputs that can read input index i (a superset; weights decide)
__host__ __device__ __forceinline__ void axis_range(const AxisMap& a, int i, int& lo, int& hi) {
    if (a.scale > 0.f) {
        lo = max(0, (int)floorf((float)(i - 1) / a.scale) - 1);
        hi = min(a.out - 1, (int)ceilf((float)(i + 1) / a.scale) + 1);
    } else {
        lo = 0; hi = a.out - 1;  // out == 1 or in == 1: every output reads input 0
    }
}
// weight with which output o reads input i (adjoint of axis_taps); 0 if it does not
__host__ __device__ __forceinline__ float axis_weight(const AxisMap& a, int o, int i) {
    int i0, i1;
    float w1;
    axis_taps(a, o, i0, i1, w1);
    float w = 0.f;
    if (i0 == i) w += 1.0f - w1;
    if (i1 == i) w += w1;
    return w;
}
// first output with a non-zero weight on input i and the number of outputs up to the last one
__host__ __device__ __forceinline__ void axis_span(const AxisMap& a, int i, int& first, int& cnt) {
    int lo, hi;
    axis_range(a, i, lo, hi);
    first = hi + 1;
    int last = lo - 1;
    for (int o = lo; o <= hi; ++o)
        if (axis_weight(a, o, i) != 0.f) {
            first = min(first, o);
            last = o;
        }
    cnt = last - first + 1;
    if (cnt < 0) cnt = 0;
}

// adjoint gather: dx[i] = sum over outputs o of w(o, i) dy[o].  Per axis and tile entry the LDS
// tables hold the first contributing output, their number (<= RS_KMAX, host-checked) and weights.
// K bounds the z candidates at compile time: per (x, y) candidate row the K z-loads go out
// together (clamped addresses, zero weights for the unused ones).
template <typename T, int K>
__global__ void __launch_bounds__(256)
resize_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ add, T* __restrict__ dx, AxisMap ax, AxisMap ay, AxisMap az,
                  int C, TileGrid tg) {
    __shared__ int s_first[3][RS_MAXT], s_cnt[3][RS_MAXT];
    __shared__ float s_w[3][RS_MAXT][RS_KMAX];
    int b, ix0, iy0, iz0;
    tile_origin(tg, b, ix0, iy0, iz0);
    if (threadIdx.x < 3 * RS_MAXT) {
        const int a = threadIdx.x / RS_MAXT, k = threadIdx.x % RS_MAXT;
        int i0, f, c;
        const AxisMap& m = tile_axis(a, ax, ay, az, ix0, iy0, iz0, i0);
        const int i = min(i0 + k, m.in - 1);
        axis_span(m, i, f, c);
        s_first[a][k] = f; s_cnt[a][k] = c;
        for (int j = 0; j < RS_KMAX; ++j) s_w[a][k][j] = j < c ? axis_weight(m, f + j, i) : 0.f;
    }
    __syncthreads();
    const int nvox = tg.tx * tg.ty * tg.tz;
    int lc, per_pass, slot0, kx, ky, kz;
    if (!lane_split(C, lc, per_pass, slot0)) return;
    for (int slot = slot0; slot < nvox; slot += per_pass) {
        slot_voxel(tg, slot, kx, ky, kz);
        const int ix = ix0 + kx, iy = iy0 + ky, iz = iz0 + kz;
        if (ix >= ax.in || iy >= ay.in || iz >= az.in) continue;
        const int fx = s_first[0][kx], cx = s_cnt[0][kx], fy = s_first[1][ky], cy = s_cnt[1][ky], fz = s_first[2][kz];
        float wz[K];
        int oz[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            oz[k] = min(fz + k, az.out - 1);
            wz[k] = s_w[2][kz][k];
        }
        const T* gb = dy + ((int64_t)b * ax.out * ay.out * az.out) * C + lc * 8;
        float acc[8] = {};
        for (int a = 0; a < cx; ++a) {
            const float wx = s_w[0][kx][a];
            for (int bb = 0; bb < cy; ++bb) {
                const float wxy = wx * s_w[1][ky][bb];
                const T* row = gb + (((int64_t)(fx + a) * ay.out + (fy + bb)) * az.out) * C;
                Raw8<T> t[K];
#pragma unroll
                for (int k = 0; k < K; ++k) t[k].load(row + (int64_t)oz[k] * C);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float w = wxy * wz[k];
                    const Vec8<T> v = t[k].get();
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += w * v.v[j];
                }
            }
        }
        store_adjoint(acc, add, dx, ((((int64_t)b * ax.in + ix) * ay.in + iy) * az.in + iz) * C + lc * 8);
    }
}

// General fallback of the adjoint (any resampling factor): one lane per (input voxel, 8 channels),
// candidate outputs scanned over a superset range with the weights recomputed on the fly
template <typename T>
__global__ void __launch_bounds__(256)
resize_bwd_generic_kernel(const T* __restrict__ dy, const T* __restrict__ add, T* __restrict__ dx, AxisMap ax, AxisMap ay,
                          AxisMap az, int C, int64_t total) {
    const int L = C >> 3;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lc = (int)(i % L);
    int64_t v = i / L;
    const int iz = (int)(v % az.in); v /= az.in;
    const int iy = (int)(v % ay.in); v /= ay.in;
    const int ix = (int)(v % ax.in);
    const int b = (int)(v / ax.in);
    int x0, x1, y0, y1, z0, z1;
    axis_range(ax, ix, x0, x1);
    axis_range(ay, iy, y0, y1);
    axis_range(az, iz, z0, z1);
    const T* gb = dy + ((int64_t)b * ax.out * ay.out * az.out) * C + lc * 8;
    float acc[8] = {};
    for (int ox = x0; ox <= x1; ++ox) {
        const float wx = axis_weight(ax, ox, ix);
        if (wx == 0.f) continue;
        for (int oy = y0; oy <= y1; ++oy) {
            const float wxy = wx * axis_weight(ay, oy, iy);
            if (wxy == 0.f) continue;
            const T* row = gb + (((int64_t)ox * ay.out + oy) * az.out) * C;
            for (int oz = z0; oz <= z1; ++oz) {
                const float w = wxy * axis_weight(az, oz, iz);
                if (w == 0.f) continue;
                Vec8<T> t;
                t.load(row + (int64_t)oz * C);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += w * t.v[j];
            }
        }
    }
    store_adjoint(acc, add, dx, ((((int64_t)b * ax.in + ix) * ay.in + iy) * az.in + iz) * C + lc * 8);
}

// ---- host side: one plan per call --------------------------------------------------------------------------------------
static TileGrid make_tiles(int X, int Y, int Z, int C, int64_t samples = 0) {
    // ~8 passes of (256 / L) voxels: 256 voxels up to 64 channels, halved for every doubling beyond
    const int L = C >> 3;
    int vox = 256;
    while (vox > 8 && vox * L > 8 * 256) vox >>= 1;
    // samples > 0 (both callers pass the batch size): small tensors get smaller tiles, down to one pass per workgroup, until
    // ~1024 workgroups exist -- a tile's passes are chains of dependent gathers, and the 48x16x12 / 24x8x6 levels left 576 /
    // 144 / 72 eight-pass workgroups on 256 CUs (100 / 68 / 30 us for 141 / 35 / 8 MB)
    const int one_pass = 256 / L > 8 ? 256 / L : 8;
    while (samples > 0 && vox > one_pass && samples * X * Y * Z / vox < 1024) vox >>= 1;
    TileGrid t;
    t.tz = 8; t.ty = 8; t.tx = 4;
    // shrink x first, then y, then z, down to the voxel budget
    while (t.tx * t.ty * t.tz > vox && t.tx > 1) t.tx >>= 1;
    while (t.tx * t.ty * t.tz > vox && t.ty > 1) t.ty >>= 1;
    while (t.tx * t.ty * t.tz > vox && t.tz > 1) t.tz >>= 1;
    t.sy = 0; while ((1 << t.sy) < t.ty) ++t.sy;
    t.sz = 0; while ((1 << t.sz) < t.tz) ++t.sz;
    t.nx = ceil_div(X, t.tx); t.ny = ceil_div(Y, t.ty); t.nz = ceil_div(Z, t.tz);
    return t;
}
// largest number of outputs that read one input along an axis (exact, same float arithmetic)
static int axis_max_span(const AxisMap& a) {
    int m = 0;
    for (int i = 0; i < a.in; ++i) {
        int f, c;
        axis_span(a, i, f, c);
        m = c > m ? c : m;
    }
    return m;
}
static int dtype_status(int dtype) {
    TDX_DISPATCH_DTYPE(dtype, (void)sizeof(T));
    return TDX_OK;
}

struct ResizePlan {
    int status;  // what tdx_resize_fwd / tdx_resize_bwd return for these arguments; the rest is set when it is TDX_OK
    int B, C;
    AxisMap ax, ay, az;
    int fwd_kernel;      // TDX_RESIZE_PAIRS / TDX_RESIZE_GATHER
    TileGrid fwd_tiles;  // of the output grid
    int bwd_kernel, bwd_k;  // TDX_RESIZE_TILED with K = 2 / 4 / 6 / 12; TDX_RESIZE_GENERIC with K = 0
    TileGrid bwd_tiles;     // of the input grid; zeros for the generic kernel
    int span[3];            // axis_max_span of x, y, z
};
enum { RS_FWD = 1, RS_BWD = 2 };  // the halves of a plan
static ResizePlan resize_plan(int B, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo, int C, int dtype, int halves = RS_FWD | RS_BWD) {
    ResizePlan p = {};
    p.status = !(B > 0 && Xi > 0 && Yi > 0 && Zi > 0 && Xo > 0 && Yo > 0 && Zo > 0 && C > 0) ? TDX_EINVAL
               : (C % 8 || C / 8 > 256)                                                        ? TDX_ESHAPE
                                                                                               : dtype_status(dtype);
    if (p.status != TDX_OK) return p;
    p.B = B; p.C = C;
    p.ax = make_axis(Xi, Xo); p.ay = make_axis(Yi, Yo); p.az = make_axis(Zi, Zo);
    if (halves & RS_FWD) {
        const TileGrid t = p.fwd_tiles = make_tiles(Xo, Yo, Zo, C, B);
        // measured (tools/micro/resize_bench.py, B = 8): 64 channels 281 -> 256 us, 128 channels 65 -> 69 us: narrow rows only
        const bool pairs = C <= 64 && !((t.tx | t.ty | t.tz) & 1) && Xo > Xi && Yo > Yi && Zo > Zi && pair_window_ok(p.ax) &&
                           pair_window_ok(p.ay) && pair_window_ok(p.az);
        p.fwd_kernel = pairs ? TDX_RESIZE_PAIRS : TDX_RESIZE_GATHER;
    }
    if (halves & RS_BWD) {
        const int kx = p.span[0] = axis_max_span(p.ax), ky = p.span[1] = axis_max_span(p.ay), kz = p.span[2] = axis_max_span(p.az);
        p.bwd_kernel = TDX_RESIZE_GENERIC;  // more than ~6x upsampling along an axis: general kernel
        if (kx <= RS_KMAX && ky <= RS_KMAX && kz <= RS_KMAX) {
            p.bwd_kernel = TDX_RESIZE_TILED;
            p.bwd_k = kz <= 2 ? 2 : kz <= 4 ? 4 : kz <= 6 ? 6 : RS_KMAX;
            p.bwd_tiles = make_tiles(Xi, Yi, Zi, C, B);
        }
    }
    return p;
}

static dim3 tile_blocks(int B, const TileGrid& tg) { return dim3((unsigned)((int64_t)B * tg.nx * tg.ny * tg.nz)); }
template <typename T>
static void launch_fwd(const ResizePlan& p, const T* x, T* y, hipStream_t st) {
    auto kernel = p.fwd_kernel == TDX_RESIZE_PAIRS ? resize_up_pairs_kernel<T> : resize_fwd_kernel<T>;
    hipLaunchKernelGGL(kernel, tile_blocks(p.B, p.fwd_tiles), dim3(256), 0, st, x, y, p.ax, p.ay, p.az, p.C, p.fwd_tiles);
}
template <typename T>
static void launch_bwd(const ResizePlan& p, const T* dy, const T* add, T* dx, hipStream_t st) {
    if (p.bwd_kernel == TDX_RESIZE_GENERIC) {
        const int64_t total = (int64_t)p.B * p.ax.in * p.ay.in * p.az.in * (p.C / 8);
        hipLaunchKernelGGL((resize_bwd_generic_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, st, dy, add, dx, p.ax, p.ay, p.az,
                           p.C, total);
        return;
    }
    auto kernel = p.bwd_k == 2 ? resize_bwd_kernel<T, 2> : p.bwd_k == 4 ? resize_bwd_kernel<T, 4>
                : p.bwd_k == 6 ? resize_bwd_kernel<T, 6> : resize_bwd_kernel<T, RS_KMAX>;
    hipLaunchKernelGGL(kernel, tile_blocks(p.B, p.bwd_tiles), dim3(256), 0, st, dy, add, dx, p.ax, p.ay, p.az, p.C, p.bwd_tiles);
}

extern "C" int tdx_resize_fwd(const void* x, void* y, int B, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo, int C,
                              int dtype, void* stream) {
    TDX_CHECK_ARG(x && y);
    const ResizePlan p = resize_plan(B, Xi, Yi, Zi, Xo, Yo, Zo, C, dtype, RS_FWD);
    if (p.status != TDX_OK) return p.status;
    TDX_DISPATCH_DTYPE(dtype, launch_fwd<T>(p, (const T*)x, (T*)y, as_stream(stream)));
    return tdx_launch_status();
}
extern "C" int tdx_resize_bwd(const void* dy, const void* add, void* dx, int B, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo, int C,
                              int dtype, void* stream) {
    TDX_CHECK_ARG(dy && dx);
    const ResizePlan p = resize_plan(B, Xi, Yi, Zi, Xo, Yo, Zo, C, dtype, RS_BWD);
    if (p.status != TDX_OK) return p.status;
    TDX_DISPATCH_DTYPE(dtype, launch_bwd<T>(p, (const T*)dy, (const T*)add, (T*)dx, as_stream(stream)));
    return tdx_launch_status();
}

// the plan query (include/tdx.h): the whole plan as integers, nothing launched
extern "C" int tdx_resize_plan(int B, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo, int C, int dtype, int* plan) {
    TDX_CHECK_ARG(plan);
    const ResizePlan p = resize_plan(B, Xi, Yi, Zi, Xo, Yo, Zo, C, dtype);
    const TileGrid tiles[2] = {p.fwd_tiles, p.bwd_tiles};  // all zeros unless the status is TDX_OK (and the adjoint tiled)
    const int first[2] = {TDX_RESIZE_PLAN_FWD_TX, TDX_RESIZE_PLAN_BWD_TX};
    for (int h = 0; h < 2; ++h) {
        const int v[6] = {tiles[h].tx, tiles[h].ty, tiles[h].tz, tiles[h].nx, tiles[h].ny, tiles[h].nz};
        for (int i = 0; i < 6; ++i) plan[first[h] + i] = v[i];  // TX, TY, TZ, NX, NY, NZ are consecutive (include/tdx.h)
    }
    plan[TDX_RESIZE_PLAN_FWD_KERNEL] = p.fwd_kernel;
    plan[TDX_RESIZE_PLAN_BWD_KERNEL] = p.bwd_kernel;
    plan[TDX_RESIZE_PLAN_BWD_K] = p.bwd_k;
    for (int a = 0; a < 3; ++a) plan[TDX_RESIZE_PLAN_SPAN_X + a] = p.span[a];
    return p.status;
}
