// TF-Net's flow decomposition (tfnet.py:304-337) forward / backward in one pass each: xx (B, T, F, X, Y, Z) fp32 -> the
// three encoder inputs u_bar, u_tilde, u_prime as NDHWC tensors (B, X, Y, Z, Cp), Cp = up8(n F), n = T - L + 1, channel
// c = t' F + f, in the network's dtype (f32 / bf16), channels >= n F written as zeros.
//   u*[t]     = sum_d S[d] xx[t, f, v + d]            3x3x3 spatial filter, zero padding
//   bar[t']   = sum_l w[l] u*[t' + l]                 temporal filter over windows of L steps
//   tilde[t'] = u*[L-1+t'] - bar[t']                  prime[t'] = xx[L-1+t'] - u*[L-1+t']
// The forward's arithmetic is fp32; the one rounding to bf16 is the store.  No fp32 intermediate tensor touches HBM.
//
// A workgroup of 256 threads owns a 4 x 4 x 16 tile of one sample, one voxel per thread (z fastest), and stages planes of
// the tile with its halo of one voxel (6 x 6 x 18 = 648 floats, zeros outside the grid) in LDS.
//   forward : per feature f the T planes of xx are staged; a thread takes its 27 taps per step and keeps u*[t, f] and the
//             centre values in its own LDS column (indexed by runtime t, f: registers cannot be); then it forms its voxel's
//             channel vector eight channels at a time and stores it.
//   backward: g*[t] = sum_{l} w[l] d[t-l] + [t >= L-1] (gt - gp)[t-L+1], d = gb - gt, is elementwise in the incoming
//             gradients, so the tile forms g* on its own halo (one read of the three gradient vectors per halo voxel, scattered
//             into T F planes in LDS).  Then per plane (t, f): xx staged (double buffered, next plane's loads in flight),
//             dS[d] += g*[v] xx[v+d], u* recomputed from the same 27 values, dw[l] += d[t-l] u*, and, when asked for,
//             gxx = [t >= L-1] gp + sum_d S[d] g*[v-d].
//   sums    : f64 throughout: per thread over its T F planes, wave butterfly, the four waves in order, one table column
//             per workgroup, and one wave per entry adds the columns in a fixed order.  No atomics: results are
//             bit-identical from run to run, with or without TDX_DETERMINISTIC.
#include "tdx_common.h"

#define FLD_TX 4
#define FLD_TY 4
#define FLD_TZ 16
#define FLD_THREADS 256
#define FLD_HY 6
#define FLD_HZ 18
#define FLD_HV 648      // halo tile: 6 x 6 x 18
#define FLD_SX 108      // halo strides
#define FLD_SY 18
#define FLD_SLOTS 3     // halo voxels per thread: ceil(648 / 256)
#define FLD_MAX_T 8
#define FLD_MAX_F 8
#define FLD_MAX_PLANES 32   // T F
#define FLD_GRID_Y 65535    // samples along gridDim.y; the rest of B along gridDim.z
#define FLD_MAX_TILES ((1 << 24) - 1)  // gridDim.x: tiles * 256 threads stays below 2^32, a launch's limit per axis
#define FLD_MAX_LDS (124 * 1024)  // >= the backward's (32 * 648 + 32 * 256 + 2 * 648) * 4 = 120896 B

struct FldShape {
    int B, T, L, F, X, Y, Z, n, nF, Cp, ty, tz;
    int64_t V;
};

// the supported shapes and the tile grid; restated by the tests (tests/flow_decompose_cases.py: tile_geometry)
static bool fld_shape(int B, int T, int L, int F, int X, int Y, int Z, FldShape& s, int& tiles) {
    if (B < 1 || T < 1 || T > FLD_MAX_T || L < 1 || L > T || F < 1 || F > FLD_MAX_F || T * F > FLD_MAX_PLANES) return false;
    if (X < 1 || Y < 1 || Z < 1) return false;
    const int64_t V = (int64_t)X * Y * Z;
    if (V >= ((int64_t)1 << 31)) return false;
    s.B = B; s.T = T; s.L = L; s.F = F; s.X = X; s.Y = Y; s.Z = Z;
    s.n = T - L + 1;
    s.nF = s.n * F;
    s.Cp = (s.nF + 7) & ~7;
    s.V = V;
    const int tx = (X + FLD_TX - 1) / FLD_TX;
    s.ty = (Y + FLD_TY - 1) / FLD_TY;
    s.tz = (Z + FLD_TZ - 1) / FLD_TZ;
    const int64_t nt = (int64_t)tx * s.ty * s.tz;  // <= V: every tile holds a voxel
    if (nt > FLD_MAX_TILES) return false;         // only grids thinner than a tile get there: 1 x 1 x Z from Z > 2^28 - 16
    tiles = (int)nt;
    return true;
}

// workspace: [27 + L][B tiles] f64, one column per workgroup
extern "C" size_t tdx_flow_decompose_workspace_bytes(int B, int T, int L, int F, int X, int Y, int Z) {
    FldShape s;
    int tiles;
    if (!fld_shape(B, T, L, F, X, Y, Z, s, tiles)) return 0;
    return (size_t)(27 + L) * (size_t)B * (size_t)tiles * sizeof(double);
}

struct FldTile {
    int x0, y0, z0;        // the tile's origin
    int hoff[FLD_SLOTS];   // voxel index of halo voxel tid + 256 i, -1 outside the grid (or past the halo tile)
    int center;            // the thread's own voxel in the halo tile
    int vox;               // its voxel index, -1 outside the grid
};

__device__ __forceinline__ FldTile fld_tile(const FldShape& s) {
    FldTile t;
    int bid = blockIdx.x;
    const int tz = bid % s.tz;
    bid /= s.tz;
    const int ty = bid % s.ty;
    t.x0 = (bid / s.ty) * FLD_TX;
    t.y0 = ty * FLD_TY;
    t.z0 = tz * FLD_TZ;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < FLD_SLOTS; ++i) {
        const int h = tid + FLD_THREADS * i;
        const int hz = h % FLD_HZ, hy = (h / FLD_HZ) % FLD_HY, hx = h / FLD_SX;
        const int gx = t.x0 - 1 + hx, gy = t.y0 - 1 + hy, gz = t.z0 - 1 + hz;
        const bool in = h < FLD_HV && gx >= 0 && gx < s.X && gy >= 0 && gy < s.Y && gz >= 0 && gz < s.Z;
        t.hoff[i] = in ? (gx * s.Y + gy) * s.Z + gz : -1;
    }
    const int lz = tid & 15, ly = (tid >> 4) & 3, lx = tid >> 6;
    t.center = (lx + 1) * FLD_SX + (ly + 1) * FLD_SY + lz + 1;
    const int gx = t.x0 + lx, gy = t.y0 + ly, gz = t.z0 + lz;
    t.vox = (gx < s.X && gy < s.Y && gz < s.Z) ? (gx * s.Y + gy) * s.Z + gz : -1;
    return t;
}

// the workgroup's sample: B runs along gridDim.y and, past 65535, gridDim.z (the last z layer may hold samples >= B)
__device__ __forceinline__ int fld_sample() { return blockIdx.y + blockIdx.z * gridDim.y; }
static dim3 fld_grid(int tiles, int B) {
    const int gy = B < FLD_GRID_Y ? B : FLD_GRID_Y;
    return dim3(tiles, gy, (B + gy - 1) / gy);
}

// one plane's halo tile: global -> registers -> LDS (zeros outside the grid)
__device__ __forceinline__ void fld_load_plane(float (&r)[FLD_SLOTS], const float* __restrict__ plane, const FldTile& t) {
#pragma unroll
    for (int i = 0; i < FLD_SLOTS; ++i) r[i] = t.hoff[i] >= 0 ? plane[t.hoff[i]] : 0.f;
}
__device__ __forceinline__ void fld_store_plane(const float (&r)[FLD_SLOTS], float* __restrict__ dst) {
#pragma unroll
    for (int i = 0; i < FLD_SLOTS; ++i) {
        const int h = threadIdx.x + FLD_THREADS * i;
        if (h < FLD_HV) dst[h] = r[i];
    }
}

// the 27 values around p (halo-tile pointer of the thread's voxel), k = (dx + 1) 9 + (dy + 1) 3 + dz + 1
__device__ __forceinline__ void fld_taps(float (&xn)[27], const float* __restrict__ p) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) xn[(dx + 1) * 9 + (dy + 1) * 3 + dz + 1] = p[dx * FLD_SX + dy * FLD_SY + dz];
}
__device__ __forceinline__ float fld_dot27(const float (&S)[27], const float (&xn)[27]) {
    float u = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) u = __builtin_fmaf(S[k], xn[k], u);
    return u;
}

template <typename T_>
__global__ void __launch_bounds__(FLD_THREADS)
fld_fwd_kernel(const float* __restrict__ xx, const float* __restrict__ sw, const float* __restrict__ tw, T_* __restrict__ bar,
               T_* __restrict__ tilde, T_* __restrict__ prime, FldShape s) {
    extern __shared__ __attribute__((aligned(16))) float fld_lds[];
    float* const stage = fld_lds;                          // [T][648]
    float* const U = stage + s.T * FLD_HV;                  // [T F][256]: u*, column tid is the thread's own
    float* const XC = U + s.T * s.F * FLD_THREADS;          // [n F][256]: xx[L-1+t'] at the voxel
    const int tid = threadIdx.x;
    const int smp = fld_sample();
    if (smp >= s.B) return;  // the whole workgroup, before any barrier
    const FldTile t = fld_tile(s);
    float S[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) S[k] = sw[k];
    const float* const xb = xx + (int64_t)smp * s.T * s.F * s.V;
    // a feature's T planes travel together (all loads issued before the first is used), the next feature's during the taps
    float r[FLD_MAX_T][FLD_SLOTS];
    auto load = [&](int f) {
#pragma unroll
        for (int tt = 0; tt < FLD_MAX_T; ++tt)
            if (tt < s.T) fld_load_plane(r[tt], xb + ((int64_t)tt * s.F + f) * s.V, t);
    };
    load(0);
    for (int f = 0; f < s.F; ++f) {
        __syncthreads();  // the previous feature's taps are read
#pragma unroll
        for (int tt = 0; tt < FLD_MAX_T; ++tt)
            if (tt < s.T) fld_store_plane(r[tt], stage + tt * FLD_HV);
        __syncthreads();
        if (f + 1 < s.F) load(f + 1);
        for (int tt = 0; tt < s.T; ++tt) {
            float xn[27];
            fld_taps(xn, stage + tt * FLD_HV + t.center);
            U[(tt * s.F + f) * FLD_THREADS + tid] = fld_dot27(S, xn);
            if (tt >= s.L - 1) XC[((tt - s.L + 1) * s.F + f) * FLD_THREADS + tid] = xn[13];
        }
    }
    if (t.vox < 0) return;
    float w[FLD_MAX_T];
#pragma unroll
    for (int l = 0; l < FLD_MAX_T; ++l) w[l] = l < s.L ? tw[l] : 0.f;
    const int64_t o = ((int64_t)smp * s.V + t.vox) * s.Cp;
    for (int c0 = 0; c0 < s.Cp; c0 += 8) {
        Vec8<T_> vb, vt, vp;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            float rb = 0.f, rt = 0.f, rp = 0.f;
            if (c < s.nF) {
                const int tp = c / s.F, f = c - tp * s.F;
                const float* const u = U + (tp * s.F + f) * FLD_THREADS + tid;
                const int step = s.F * FLD_THREADS;
                float a = 0.f;
#pragma unroll
                for (int l = 0; l < FLD_MAX_T; ++l)
                    if (l < s.L) a = __builtin_fmaf(w[l], u[l * step], a);
                const float last = u[(s.L - 1) * step];
                rb = a;
                rt = last - a;
                rp = XC[c * FLD_THREADS + tid] - last;
            }
            vb.v[j] = rb;
            vt.v[j] = rt;
            vp.v[j] = rp;
        }
        vb.store(bar + o + c0);
        vt.store(tilde + o + c0);
        vp.store(prime + o + c0);
    }
}

template <typename T_, bool HAS_GXX>
__global__ void __launch_bounds__(FLD_THREADS)
fld_bwd_kernel(const float* __restrict__ xx, const float* __restrict__ sw, const float* __restrict__ tw, const T_* __restrict__ gb,
               const T_* __restrict__ gt, const T_* __restrict__ gp, float* __restrict__ gxx, double* __restrict__ part, FldShape s) {
    extern __shared__ __attribute__((aligned(16))) float fld_lds[];
    __shared__ double wred[FLD_THREADS / 64][27 + FLD_MAX_T];
    const int Q = s.T * s.F;
    float* const G = fld_lds;                      // [T F][648]: g* on the halo tile
    float* const D = G + Q * FLD_HV;               // [n F][256]: d = gb - gt at the tile's voxels
    float* const XS = D + s.nF * FLD_THREADS;      // [2][648]: the plane of xx in work, the next one
    const int tid = threadIdx.x;
    const int smp = fld_sample();
    if (smp >= s.B) return;  // the whole workgroup, before any barrier
    const FldTile t = fld_tile(s);
    double S[27];  // the plane loop works in f64 (below)
    float w[FLD_MAX_T];
#pragma unroll
    for (int k = 0; k < 27; ++k) S[k] = (double)sw[k];
#pragma unroll
    for (int l = 0; l < FLD_MAX_T; ++l) w[l] = l < s.L ? tw[l] : 0.f;
    const float* const xb = xx + (int64_t)smp * Q * s.V;
    float r[FLD_SLOTS];
    fld_load_plane(r, xb, t);  // plane 0 is on its way while g* is formed

    // ---- g* of every plane on the halo tile; a thread owns the columns of its halo voxels
#pragma unroll
    for (int i = 0; i < FLD_SLOTS; ++i) {
        const int h = tid + FLD_THREADS * i;
        if (h >= FLD_HV) continue;
        for (int q = 0; q < Q; ++q) G[q * FLD_HV + h] = 0.f;
        if (t.hoff[i] < 0) continue;
        const int hz = h % FLD_HZ - 1, hy = (h / FLD_HZ) % FLD_HY - 1, hx = h / FLD_SX - 1;
        const bool inner = hx >= 0 && hx < FLD_TX && hy >= 0 && hy < FLD_TY && hz >= 0 && hz < FLD_TZ;
        const int col = (hx * FLD_TY + hy) * FLD_TZ + hz;  // the thread id of that voxel
        const int64_t o = ((int64_t)smp * s.V + t.hoff[i]) * s.Cp;
        Vec8<T_> a[FLD_MAX_PLANES / 8], b[FLD_MAX_PLANES / 8], c[FLD_MAX_PLANES / 8];  // every chunk's loads before the first use
#pragma unroll
        for (int k = 0; k < FLD_MAX_PLANES / 8; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[k].v[j] = b[k].v[j] = c[k].v[j] = 0.f;
            if (k * 8 < s.Cp) {
                if (gb) a[k].load(gb + o + k * 8);
                if (gt) b[k].load(gt + o + k * 8);
                if (gp) c[k].load(gp + o + k * 8);
            }
        }
#pragma unroll
        for (int k = 0; k < FLD_MAX_PLANES / 8; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ch = k * 8 + j;
                if (ch >= s.nF) continue;
                const int tp = ch / s.F, f = ch - tp * s.F;
                const float d = a[k].v[j] - b[k].v[j];
                float* const g = G + (tp * s.F + f) * FLD_HV + h;
                const int step = s.F * FLD_HV;
#pragma unroll
                for (int l = 0; l < FLD_MAX_T; ++l)
                    if (l < s.L) g[l * step] = __builtin_fmaf(w[l], d, g[l * step]);
                g[(s.L - 1) * step] += b[k].v[j] - c[k].v[j];
                if (inner) D[ch * FLD_THREADS + col] = d;
            }
        }
    }
    fld_store_plane(r, XS);
    __syncthreads();

    // ---- plane by plane.  Products and sums are f64: the three results are compared with fp32 routes at fp32 rounding
    // level, where a chain of 27 fp32 FMAs alone errs by more than the final rounding (tests/test_flow_decompose_gpu.py);
    // the pass has the registers (LDS bounds its occupancy) and f64 FMAs run at half the fp32 rate
    double acc[27], dwa[FLD_MAX_T];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll
    for (int l = 0; l < FLD_MAX_T; ++l) dwa[l] = 0.0;
    const int64_t ob = (int64_t)smp * s.V + t.vox;
    for (int q = 0; q < Q; ++q) {
        const float* const cur = XS + (q & 1) * FLD_HV;
        if (q + 1 < Q) fld_load_plane(r, xb + (int64_t)(q + 1) * s.V, t);
        if (t.vox >= 0) {
            const int tt = q / s.F, f = q - tt * s.F;
            float xn[27];
            fld_taps(xn, cur + t.center);
            const float* const gq = G + q * FLD_HV + t.center;
            const double g = (double)gq[0];
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                const double x = (double)xn[k];
                acc[k] = __builtin_fma(g, x, acc[k]);
                u = __builtin_fma(S[k], x, u);
            }
#pragma unroll
            for (int l = 0; l < FLD_MAX_T; ++l) {
                const int tp = tt - l;
                if (l < s.L && tp >= 0 && tp < s.n) dwa[l] = __builtin_fma((double)D[(tp * s.F + f) * FLD_THREADS + tid], u, dwa[l]);
            }
            if (HAS_GXX) {
                float gn[27];
                fld_taps(gn, gq);
                double v = 0.0;  // sum_d S[d] g*[v - d]: tap k of S meets tap 26 - k of g*
#pragma unroll
                for (int k = 0; k < 27; ++k) v = __builtin_fma(S[k], (double)gn[26 - k], v);
                if (tt >= s.L - 1 && gp) v += (double)ldf(gp + ob * s.Cp + (tt - s.L + 1) * s.F + f);
                gxx[((int64_t)smp * Q + q) * s.V + t.vox] = (float)v;
            }
        }
        if (q + 1 < Q) fld_store_plane(r, XS + ((q + 1) & 1) * FLD_HV);
        __syncthreads();
    }

    // ---- the workgroup's column of the tables
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) wred[wave][k] = v;
    }
#pragma unroll
    for (int l = 0; l < FLD_MAX_T; ++l) {
        if (l < s.L) {  // the same in every lane
            const double v = wave_sum(dwa[l]);
            if (lane == 0) wred[wave][27 + l] = v;
        }
    }
    __syncthreads();
    if (tid < 27 + s.L) {
        double v = wred[0][tid];
#pragma unroll
        for (int i = 1; i < FLD_THREADS / 64; ++i) v += wred[i][tid];
        const int64_t nblk = (int64_t)gridDim.x * s.B;
        part[tid * nblk + (int64_t)smp * gridDim.x + blockIdx.x] = v;
    }
}

// One wave per entry: lane l adds the columns l, l + 64, ... in that order, then the butterfly (fixed order).
__global__ void __launch_bounds__(64)
fld_merge_kernel(const double* __restrict__ part, float* __restrict__ gs, float* __restrict__ gw, int64_t nblk) {
    const int k = blockIdx.x;
    const double* const p = part + k * nblk;
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += 64) a += p[i];
    a = wave_sum(a);
    if (threadIdx.x == 0) {
        if (k < 27) gs[k] = (float)a;
        else gw[k - 27] = (float)a;
    }
}

// the kernels' dynamic LDS can pass the default limit: the attribute is raised to the largest supported shape's
template <auto KERN, typename... Args>
static int fld_launch(dim3 grid, size_t lds, hipStream_t st, Args... args) {
    return tdx_launch_lds_max<KERN>(grid, dim3(FLD_THREADS), FLD_MAX_LDS, lds, st, args...);
}

extern "C" int tdx_flow_decompose_fwd(const float* xx, const float* spatial_w, const float* temporal_w, void* bar, void* tilde,
                                      void* prime, int B, int T, int L, int F, int X, int Y, int Z, int dtype, void* stream) {
    TDX_CHECK_ARG(xx && spatial_w && temporal_w && bar && tilde && prime);
    FldShape s;
    int tiles;
    if (!fld_shape(B, T, L, F, X, Y, Z, s, tiles)) return TDX_ESHAPE;
    if (dtype != TDX_F32 && dtype != TDX_BF16) return TDX_EDTYPE;
    const size_t lds = ((size_t)T * FLD_HV + (size_t)(T * F + s.nF) * FLD_THREADS) * sizeof(float);
    const dim3 grid = fld_grid(tiles, B);
    if (dtype == TDX_F32)
        return fld_launch<fld_fwd_kernel<float>>(grid, lds, as_stream(stream), xx, spatial_w, temporal_w, (float*)bar, (float*)tilde,
                                                 (float*)prime, s);
    return fld_launch<fld_fwd_kernel<bf16>>(grid, lds, as_stream(stream), xx, spatial_w, temporal_w, (bf16*)bar, (bf16*)tilde,
                                            (bf16*)prime, s);
}

extern "C" int tdx_flow_decompose_bwd(const float* xx, const float* spatial_w, const float* temporal_w, const void* gbar,
                                      const void* gtilde, const void* gprime, float* gxx, float* gspatial, float* gtemporal, int B,
                                      int T, int L, int F, int X, int Y, int Z, int dtype, void* workspace, void* stream) {
    TDX_CHECK_ARG(xx && spatial_w && temporal_w && gspatial && gtemporal && workspace);
    FldShape s;
    int tiles;
    if (!fld_shape(B, T, L, F, X, Y, Z, s, tiles)) return TDX_ESHAPE;
    if (dtype != TDX_F32 && dtype != TDX_BF16) return TDX_EDTYPE;
    const size_t lds = ((size_t)T * F * FLD_HV + (size_t)s.nF * FLD_THREADS + 2 * FLD_HV) * sizeof(float);
    const dim3 grid = fld_grid(tiles, B);
    hipStream_t st = as_stream(stream);
    double* part = (double*)workspace;
    int rc = TDX_OK;
    TDX_DISPATCH_BOOL(gxx != nullptr, GX, {
        if (dtype == TDX_F32)
            rc = fld_launch<fld_bwd_kernel<float, GX>>(grid, lds, st, xx, spatial_w, temporal_w, (const float*)gbar, (const float*)gtilde,
                                                       (const float*)gprime, gxx, part, s);
        else
            rc = fld_launch<fld_bwd_kernel<bf16, GX>>(grid, lds, st, xx, spatial_w, temporal_w, (const bf16*)gbar, (const bf16*)gtilde,
                                                      (const bf16*)gprime, gxx, part, s);
    });
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(fld_merge_kernel, dim3(27 + L), dim3(64), 0, st, part, gspatial, gtemporal, (int64_t)tiles * B);
    return tdx_launch_status();
}
