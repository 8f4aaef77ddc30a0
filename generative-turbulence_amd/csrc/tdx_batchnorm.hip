// BatchNorm3d + LeakyReLU (+ add) forward / backward on channels-last activations (rows, C), rows = B X Y Z: the tail
// of tfnet's conv() blocks (Conv3d -> BatchNorm3d -> LeakyReLU(0.1)).
//
// HBM-bound like the GroupNorm passes and built on their streaming skeleton (tdx_gn_stream.h): a thread owns one
// 8-channel vector, so its per-channel coefficients live in registers, and walks rows with a grid stride, four rows per
// trip.  Training-mode BatchNorm over (rows, C) is GroupNorm over ONE sample of `rows` voxels with one channel per group.
//   statistics: per-thread f64 sums of (x - K) and (x - K)^2 with the shift K = x[row 0] of the channel (no E[x^2] - E[x]^2
//               on raw values) -> per-block f64 tables -> one wave per channel adds them in a fixed order
//   apply     : n = (x - mean) rstd gamma + beta;  y = (n > 0 ? n : slope n) + add
//   backward  : reduce pass (P = sum dn, Q = sum dn xhat per channel; per-block tables) -> one wave per channel ->
//               apply pass dx = gamma rstd (dn - P/rows - xhat Q/rows)   [eval mode: dx = gamma rstd dn]
// No atomics anywhere: every merge is a fixed-order sum of per-block tables, so the results are run-to-run reproducible
// with or without TDX_DETERMINISTIC.
#define TDX_NT_LOADS 1  // activations are streamed once per pass
#include "tdx_common.h"
#include "tdx_gn_stream.h"

#define BN_MAX_BLOCKS 1024  // = 16 x 64: the merge kernels hold a lane's 16 partials in registers
#define BN_MAX_C 512

static bool bn_shape_ok(int64_t rows, int C) {
    return C > 0 && C % 8 == 0 && C <= BN_MAX_C && rows > 0 && rows < ((int64_t)1 << 31);
}

// Streaming blocks of a pass over `nb` slabs of V rows each (grid = (blocks, nb)); the launcher's grid rule, restated by
// the tests (tests/tfnet_cases.py: bn_geometry)
static int bn_blocks(int nb, int64_t V, int C) {
    const int rows = GN_THREADS / (C >> 3);
    int64_t want = (2048 + nb - 1) / nb;
    const int64_t most = (V + (int64_t)rows * GN_UNROLL - 1) / ((int64_t)rows * GN_UNROLL);
    if (want > most) want = most;
    if (want > BN_MAX_BLOCKS) want = BN_MAX_BLOCKS;
    return want < 1 ? 1 : (int)want;
}

// workspace: [blocks][C][2] f64 block tables, K[C], pq[C][2]
extern "C" size_t tdx_bn_workspace_bytes(int64_t rows, int C) {
    if (!bn_shape_ok(rows, C)) return 0;
    return (size_t)bn_blocks(1, rows, C) * C * 2 * sizeof(double) + (size_t)C * 3 * sizeof(float) + 64;
}

// s[q][j] of the block's threads -> out[c * 2 + q], summed in f64 over the threads of channel c in thread order
template <typename S>
__device__ __forceinline__ void bn_block_reduce(const S (&s)[2][8], int C, int rows, double* __restrict__ out) {
    __shared__ S red[GN_THREADS][17];
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[tid][j] = s[0][j];
        red[tid][8 + j] = s[1][j];
    }
    __syncthreads();
    const int L = C >> 3;
    for (int o = tid; o < C * 2; o += GN_THREADS) {
        const int c = o >> 1, q = o & 1;
        const int lc = c >> 3, j = c & 7;
        double t = 0.0;
        for (int r = 0; r < rows; ++r) t += (double)red[r * L + lc][q * 8 + j];
        out[o] = t;
    }
}

template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
bn_stats_kernel(const T* __restrict__ x, double* __restrict__ part, float* __restrict__ shift, int64_t rows, int C) {
    const GnLane p = gn_lane(rows, C);
    Vec8<T> k;  // the shift: row 0 of the thread's channels
    k.load(x + p.lc * 8);
    if (blockIdx.x == 0 && p.r == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) shift[p.lc * 8 + j] = k.v[j];
    }
    // f64 accumulators: the pass is HBM-bound at two f64 operations per element, and the differences x - K are exact in f64
    double s[2][8];  // stays zero in a spare thread
#pragma unroll
    for (int j = 0; j < 8; ++j) s[0][j] = s[1][j] = 0.0;
    const T* const in[1] = {x};
    gn_stream<T, 1>(p, in, rows, C, [&](const Vec8<T>(&a)[1], int64_t) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double d = (double)a[0].v[j] - (double)k.v[j];
            s[0][j] += d;
            s[1][j] = __builtin_fma(d, d, s[1][j]);
        }
    });
    bn_block_reduce(s, C, p.rows, part + (size_t)blockIdx.x * C * 2);
}

// One wave per channel: lane l adds the tables of blocks l, l + 64, ... in that order, then the butterfly (fixed order).
__device__ __forceinline__ void bn_wave_merge(const double* __restrict__ part, int nblk, int C, int c, double& a, double& b) {
    const int lane = threadIdx.x & 63;
    double2 t[BN_MAX_BLOCKS / 64];
#pragma unroll
    for (int i = 0; i < BN_MAX_BLOCKS / 64; ++i) {
        const int k = lane + 64 * i;
        t[i] = k < nblk ? *reinterpret_cast<const double2*>(part + ((size_t)k * C + c) * 2) : make_double2(0.0, 0.0);
    }
    a = 0.0;
    b = 0.0;
#pragma unroll
    for (int i = 0; i < BN_MAX_BLOCKS / 64; ++i) {
        a += t[i].x;
        b += t[i].y;
    }
    a = wave_sum(a);
    b = wave_sum(b);
}

// stats[c] = (mean, rstd), var[c] = the biased variance (for the running statistics)
__global__ void __launch_bounds__(256)
bn_stats_merge_kernel(const double* __restrict__ part, const float* __restrict__ shift, float* __restrict__ stats,
                      float* __restrict__ var, int nblk, int C, int64_t rows, float eps) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;  // whole waves leave together
    double s1, s2;
    bn_wave_merge(part, nblk, C, c, s1, s2);
    if ((threadIdx.x & 63) == 0) {
        const double n = (double)rows;
        const double d = s1 / n;
        double v = s2 / n - d * d;
        if (v < 0.0) v = 0.0;
        stats[2 * c] = (float)((double)shift[c] + d);
        stats[2 * c + 1] = (float)(1.0 / sqrt(v + (double)eps));
        if (var) var[c] = (float)v;
    }
}

#define BN_DISPATCH_DTYPE(dtype, ...)      \
    do {                                   \
        if ((dtype) == TDX_F32) {          \
            typedef float T;               \
            __VA_ARGS__;                   \
        } else if ((dtype) == TDX_BF16) {  \
            typedef bf16 T;                \
            __VA_ARGS__;                   \
        } else                             \
            return TDX_EDTYPE;             \
    } while (0)

extern "C" int tdx_bn_stats(const void* x, float* stats, float* var, int64_t rows, int C, float eps, int dtype, void* workspace,
                            void* stream) {
    TDX_CHECK_ARG(x && stats && workspace);
    if (!bn_shape_ok(rows, C) || rows < 2) return TDX_ESHAPE;
    if (dtype != TDX_F32 && dtype != TDX_BF16) return TDX_EDTYPE;
    const int nblk = bn_blocks(1, rows, C);
    double* part = (double*)workspace;
    float* shift = (float*)(part + (size_t)nblk * C * 2);
    hipStream_t st = as_stream(stream);
    BN_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(nblk), dim3(GN_THREADS), 0, st, (const T*)x, part,
                                                shift, rows, C));
    hipLaunchKernelGGL(bn_stats_merge_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, shift, stats, var, nblk, C, rows, eps);
    return tdx_launch_status();
}

// per-thread coefficients of its 8 channels
struct BnCoef {
    float mean[8], rstd[8], gam[8], bet[8];
};
__device__ __forceinline__ void bn_load_coef(BnCoef& k, const float* __restrict__ stats, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int cbase) {
    float4 st[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) st[i] = *reinterpret_cast<const float4*>(stats + (size_t)cbase * 2 + 4 * i);
    const float4 g0 = *reinterpret_cast<const float4*>(gamma + cbase), g1 = *reinterpret_cast<const float4*>(gamma + cbase + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(beta + cbase), b1 = *reinterpret_cast<const float4*>(beta + cbase + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        k.mean[2 * i] = st[i].x; k.rstd[2 * i] = st[i].y;
        k.mean[2 * i + 1] = st[i].z; k.rstd[2 * i + 1] = st[i].w;
    }
    k.gam[0] = g0.x; k.gam[1] = g0.y; k.gam[2] = g0.z; k.gam[3] = g0.w; k.gam[4] = g1.x; k.gam[5] = g1.y; k.gam[6] = g1.z; k.gam[7] = g1.w;
    k.bet[0] = b0.x; k.bet[1] = b0.y; k.bet[2] = b0.z; k.bet[3] = b0.w; k.bet[4] = b1.x; k.bet[5] = b1.y; k.bet[6] = b1.z; k.bet[7] = b1.w;
}

// Slab blockIdx.y holds rows [blockIdx.y V, (blockIdx.y + 1) V) of x and y.  `add` has V rows when it is broadcast over
// the slabs (the launcher then makes one slab per batch sample) and there is one slab when it has all the rows: either
// way its row is the row inside the slab.
template <typename T, bool HAS_ADD>
__global__ void __launch_bounds__(GN_THREADS)
bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                const float* __restrict__ beta, const T* __restrict__ add, T* __restrict__ y, int64_t V, int C, float slope) {
    const GnLane p = gn_lane(V, C);
    BnCoef k;
    bn_load_coef(k, stats, gamma, beta, p.lc * 8);
    const T* const in[1] = {x};
    auto body = [&](const Vec8<T>& a, const Vec8<T>& r, int64_t v) {
        Vec8<T> o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float n = __builtin_fmaf((a.v[j] - k.mean[j]) * k.rstd[j], k.gam[j], k.bet[j]);
            const float t = n > 0.f ? n : slope * n;
            o.v[j] = HAS_ADD ? t + r.v[j] : t;
        }
        o.store(y + p.base + v * C);
    };
    if (HAS_ADD) {
        const T* ap = add + p.lc * 8;
        gn_stream<T, 1, false>(p, in, V, C,
                               [&](int64_t v) { Raw8<T> r; r.load(ap + v * C); return r; },
                               [&](const Vec8<T>(&a)[1], const Raw8<T>& r, int64_t v) { body(a[0], r.get(), v); });
    } else {
        gn_stream<T, 1>(p, in, V, C, [&](const Vec8<T>(&a)[1], int64_t v) { body(a[0], a[0], v); });
    }
}

extern "C" int tdx_bn_apply(const void* x, const float* stats, const float* gamma, const float* beta, const void* add,
                            int64_t add_rows, void* y, int64_t rows, int C, float slope, int dtype, void* stream) {
    TDX_CHECK_ARG(x && stats && gamma && beta && y);
    if (!bn_shape_ok(rows, C)) return TDX_ESHAPE;
    if (add && (add_rows <= 0 || rows % add_rows != 0 || rows / add_rows > 65535)) return TDX_ESHAPE;
    if (dtype != TDX_F32 && dtype != TDX_BF16) return TDX_EDTYPE;
    const int nb = add ? (int)(rows / add_rows) : 1;
    const int64_t V = rows / nb;
    dim3 grid(bn_blocks(nb, V, C), nb);
    TDX_DISPATCH_BOOL(add != nullptr, A, BN_DISPATCH_DTYPE(dtype,
        hipLaunchKernelGGL((bn_apply_kernel<T, A>), grid, dim3(GN_THREADS), 0, as_stream(stream), (const T*)x, stats, gamma, beta,
                           (const T*)add, (T*)y, V, C, slope)));
    return tdx_launch_status();
}

// ------------------------------------------------------------------ backward -------------
template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
bn_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ stats,
                     const float* __restrict__ gamma, const float* __restrict__ beta, double* __restrict__ part, int64_t rows,
                     int C, float slope) {
    const GnLane p = gn_lane(rows, C);
    BnCoef k;
    bn_load_coef(k, stats, gamma, beta, p.lc * 8);
    float s[2][8];  // stays zero in a spare thread
#pragma unroll
    for (int j = 0; j < 8; ++j) s[0][j] = s[1][j] = 0.f;
    const T* const in[2] = {x, dy};
    gn_stream<T, 2>(p, in, rows, C, [&](const Vec8<T>(&a)[2], int64_t) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = (a[0].v[j] - k.mean[j]) * k.rstd[j];
            const float n = __builtin_fmaf(xh, k.gam[j], k.bet[j]);
            const float dn = n > 0.f ? a[1].v[j] : slope * a[1].v[j];
            s[0][j] += dn;
            s[1][j] = __builtin_fmaf(dn, xh, s[1][j]);
        }
    });
    bn_block_reduce(s, C, p.rows, part + (size_t)blockIdx.x * C * 2);
}

// dbeta = P, dgamma = Q; pq[c] = (P, Q) / rows in training mode, (0, 0) in eval mode
__global__ void __launch_bounds__(256)
bn_bwd_merge_kernel(const double* __restrict__ part, float* __restrict__ pq, float* __restrict__ dgamma, float* __restrict__ dbeta,
                    int nblk, int C, int64_t rows, int training) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    double P, Q;
    bn_wave_merge(part, nblk, C, c, P, Q);
    if ((threadIdx.x & 63) == 0) {
        dbeta[c] = (float)P;
        dgamma[c] = (float)Q;
        pq[2 * c] = training ? (float)(P / (double)rows) : 0.f;
        pq[2 * c + 1] = training ? (float)(Q / (double)rows) : 0.f;
    }
}

template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ stats,
                    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ pq,
                    T* __restrict__ dx, int64_t rows, int C, float slope) {
    const GnLane p = gn_lane(rows, C);
    BnCoef k;
    bn_load_coef(k, stats, gamma, beta, p.lc * 8);
    float mp[8], mq[8], gr[8];
    {
        float4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = *reinterpret_cast<const float4*>(pq + (size_t)p.lc * 16 + 4 * i);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mp[2 * i] = t[i].x; mq[2 * i] = t[i].y;
            mp[2 * i + 1] = t[i].z; mq[2 * i + 1] = t[i].w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) gr[j] = k.gam[j] * k.rstd[j];
    }
    const T* const in[2] = {x, dy};
    gn_stream<T, 2>(p, in, rows, C, [&](const Vec8<T>(&a)[2], int64_t v) {
        Vec8<T> o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = (a[0].v[j] - k.mean[j]) * k.rstd[j];
            const float n = __builtin_fmaf(xh, k.gam[j], k.bet[j]);
            const float dn = n > 0.f ? a[1].v[j] : slope * a[1].v[j];
            o.v[j] = gr[j] * (dn - __builtin_fmaf(xh, mq[j], mp[j]));
        }
        o.store(dx + p.base + v * C);
    });
}

extern "C" int tdx_bn_bwd(const void* x, const void* dy, const float* stats, const float* gamma, const float* beta, void* dx,
                          float* dgamma, float* dbeta, int64_t rows, int C, float slope, int training, int dtype,
                          void* workspace, void* stream) {
    TDX_CHECK_ARG(x && dy && stats && gamma && beta && dx && dgamma && dbeta && workspace);
    if (!bn_shape_ok(rows, C) || (training && rows < 2)) return TDX_ESHAPE;
    if (dtype != TDX_F32 && dtype != TDX_BF16) return TDX_EDTYPE;
    const int nblk = bn_blocks(1, rows, C);
    double* part = (double*)workspace;                          // [nblk][C][2]
    float* pq = (float*)(part + (size_t)nblk * C * 2) + C;      // behind K[C]
    hipStream_t st = as_stream(stream);
    BN_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T>), dim3(nblk), dim3(GN_THREADS), 0, st, (const T*)x,
                                                (const T*)dy, stats, gamma, beta, part, rows, C, slope));
    hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, pq, dgamma, dbeta, nblk, C, rows, training);
    BN_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(nblk), dim3(GN_THREADS), 0, st, (const T*)x,
                                                (const T*)dy, stats, gamma, beta, pq, (T*)dx, rows, C, slope));
    return tdx_launch_status();
}
