// Case preparation (turbdiff_amd/data/prepare.py): the reductions behind stats.pickle, mean-flow.h5 and regions.npz.
//   tdx_moments_update : streaming per-column temporal mean and centred sum of squares of a (T, n) f32 chunk, merged into
//                        fp64 running state with Chan's parallel update; one column = one thread, no atomics
//   tdx_field_stats    : per-column min / max / sum / sum of squares of a (rows, C <= 8) f32 matrix and of the row-wise L2
//                        norms over two column ranges; fp64 block partials, then one block folds them in a fixed order
//   tdx_w2n_assign     : nearest centroid of every cell under the 2-Wasserstein distance between diagonal normals
//                        (scripts/homogeneous-regions.py:16-25), centroids in LDS, optional per-block per-cluster sums
//   tdx_w2n_reduce     : folds those block sums in block order into the (k, 7) table of one Lloyd iteration
// Every sum is formed in an order fixed by the shapes alone, so results are bit-reproducible.
#include "tdx_common.h"

#include <climits>

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;

// four consecutive floats at any 4-byte-aligned address: a row of a (T, n) chunk starts 16-byte aligned only if n % 4 == 0
struct __attribute__((packed, aligned(4))) F4U {
    float v[4];
};

// ---------------------------------------------------------------------------------------------- moments
// thread = 4 neighbouring columns (16 B per lane, a wave reads 1 KiB of each row); W = columns this thread owns (4, or the
// n % 4 columns of the tail thread).  Pass 1 sums the T rows in fp64, pass 2 sums the squared deviations from the chunk's
// own mean (the rows are read again, from L2); the merge is Chan et al.'s pairwise update
__global__ void __launch_bounds__(PR_THREADS)
moments_kernel(const float* __restrict__ x, int T, int64_t n, double* __restrict__ mean, double* __restrict__ m2,
               int64_t count) {
    const int64_t c0 = ((int64_t)blockIdx.x * PR_THREADS + threadIdx.x) * 4;
    if (c0 >= n) return;
    const int W = (n - c0 >= 4) ? 4 : (int)(n - c0);
    const float* p = x + c0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    if (W == 4) {
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            const F4U r = *reinterpret_cast<const F4U*>(p + (int64_t)t * n);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += (double)r.v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] /= (double)T;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            const F4U r = *reinterpret_cast<const F4U*>(p + (int64_t)t * n);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)r.v[e] - s[e];
                q[e] = fma(d, d, q[e]);
            }
        }
    } else {
        for (int t = 0; t < T; ++t)
            for (int e = 0; e < W; ++e) s[e] += (double)p[(int64_t)t * n + e];
        for (int e = 0; e < W; ++e) s[e] /= (double)T;
        for (int t = 0; t < T; ++t)
            for (int e = 0; e < W; ++e) {
                const double d = (double)p[(int64_t)t * n + e] - s[e];
                q[e] = fma(d, d, q[e]);
            }
    }
    if (count == 0) {  // empty state: never read
        for (int e = 0; e < W; ++e) {
            mean[c0 + e] = s[e];
            m2[c0 + e] = q[e];
        }
        return;
    }
    const double na = (double)count, nb = (double)T, nt = na + nb;
    for (int e = 0; e < W; ++e) {
        const double ma = mean[c0 + e], delta = s[e] - ma;
        mean[c0 + e] = ma + delta * (nb / nt);
        m2[c0 + e] = (m2[c0 + e] + q[e]) + delta * delta * (na * nb / nt);
    }
}

// ---------------------------------------------------------------------------------------------- field stats
constexpr int FS_MAX_C = 8;
constexpr int FS_MAX_BLOCKS = 1024;

struct Acc {
    float mn, mx;
    double sum, sq;
    __device__ __forceinline__ void init() { mn = INFINITY; mx = -INFINITY; sum = 0.0; sq = 0.0; }
    // squares are formed in fp32, as `field ** 2` on a float32 array is (scripts/dataset-stats.py:30), and summed in fp64
    __device__ __forceinline__ void add(float v) {
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        sum += (double)v;
        const float vv = v * v;  // rounded to fp32 before it is widened: nothing to contract with
        sq += (double)vv;
    }
    __device__ __forceinline__ void merge(const Acc& o) {
        mn = fminf(mn, o.mn);
        mx = fmaxf(mx, o.mx);
        sum += o.sum;
        sq += o.sq;
    }
};

__device__ __forceinline__ Acc wave_merge(Acc a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Acc o;
        o.mn = __shfl_xor(a.mn, off, 64);
        o.mx = __shfl_xor(a.mx, off, 64);
        o.sum = __shfl_xor(a.sum, off, 64);
        o.sq = __shfl_xor(a.sq, off, 64);
        a.merge(o);
    }
    return a;
}

// the block's value of accumulator `a` (xor butterfly in each wave, the wave results in wave order), valid in thread 0
__device__ Acc block_merge(Acc a, Acc* red) {
    a = wave_merge(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    Acc r = red[0];
    for (int w = 1; w < PR_WAVES; ++w) r.merge(red[w]);
    return r;
}

// row-wise L2 norm in fp32, left to right, as np.linalg.norm(x, axis=-1) on float32 rows: every product and sum rounded on
// its own (no contraction into fma; the __f*_rn intrinsics are plain operators here and would contract) and the correctly
// rounded sqrtf (__fsqrt_rn is the 1-ulp hardware instruction in this build)
template <int C>
__device__ __forceinline__ float row_norm(const float (&r)[C], int lo, int hi) {
#pragma clang fp contract(off)
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < C; ++e)
        if (e >= lo && e < hi) {
            const float sq = r[e] * r[e];
            s = (e == lo) ? sq : s + sq;
        }
    return sqrtf(s);
}

struct NormRanges {
    int lo[2], hi[2];  // the two column ranges whose row-wise norms are reduced beside the columns (lo == hi: none)
};

// partials (gridDim.x, C + 2, 4) f64; rows are dealt to threads with a grid stride.  CT == 8 reads a row as two 16-B
// pieces, CT == 1 four rows as one; CT == 0 is every other width (C at run time, one 4-B load per element, columns past
// C idle).  N = columns a thread has accumulators for; the two norms sit behind them
template <int CT>
__global__ void __launch_bounds__(PR_THREADS)
field_stats_kernel(const float* __restrict__ x, int64_t rows, int C, NormRanges nr, double* __restrict__ partials) {
    constexpr int N = CT ? CT : FS_MAX_C;
    __shared__ Acc red[PR_WAVES];
    Acc acc[N + 2];
#pragma unroll
    for (int e = 0; e < N + 2; ++e) acc[e].init();
    const int64_t gid = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * PR_THREADS;
    if constexpr (CT == 1) {
        const int64_t groups = rows / 4;
        for (int64_t g = gid; g < groups; g += stride) {
            const float4 r = reinterpret_cast<const float4*>(x)[g];
            const float v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0].add(v[e]);
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (nr.hi[q] > nr.lo[q]) acc[1 + q].add(fabsf(v[e]));
            }
        }
        if (gid < rows - groups * 4) {
            const float v = x[groups * 4 + gid];
            acc[0].add(v);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (nr.hi[q] > nr.lo[q]) acc[1 + q].add(fabsf(v));
        }
    } else {
        for (int64_t r0 = gid; r0 < rows; r0 += stride) {
            float r[N];
            if constexpr (CT == 8) {
                const float4 a = reinterpret_cast<const float4*>(x + r0 * 8)[0], b = reinterpret_cast<const float4*>(x + r0 * 8)[1];
                r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
                r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e) r[e] = (e < C) ? x[r0 * C + e] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < N; ++e)
                if (CT || e < C) acc[e].add(r[e]);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (nr.hi[q] > nr.lo[q]) acc[N + q].add(row_norm<N>(r, nr.lo[q], nr.hi[q]));
        }
    }
#pragma unroll
    for (int e = 0; e < N + 2; ++e) {
        if (e >= C && e < N) continue;  // an idle column of the generic width: the same for the whole grid
        const Acc b = block_merge(acc[e], red);
        if (threadIdx.x == 0) {
            const int row = (e < N) ? e : C + e - N;
            double* o = partials + ((size_t)blockIdx.x * (C + 2) + row) * 4;
            o[0] = b.mn; o[1] = b.mx; o[2] = b.sum; o[3] = b.sq;
        }
    }
}

// one block: thread t folds partials t, t + 256, ... in that order, then the block merge.  out (C1 = C + 2, 4)
__global__ void __launch_bounds__(PR_THREADS)
field_stats_fold_kernel(const double* __restrict__ partials, int blocks, int C1, double* __restrict__ out) {
    __shared__ Acc red[PR_WAVES];
    for (int e = 0; e < C1; ++e) {
        Acc a;
        a.init();
        for (int b = threadIdx.x; b < blocks; b += PR_THREADS) {
            const double* p = partials + ((size_t)b * C1 + e) * 4;
            Acc o;
            o.mn = (float)p[0]; o.mx = (float)p[1]; o.sum = p[2]; o.sq = p[3];
            a.merge(o);
        }
        const Acc r = block_merge(a, red);
        if (threadIdx.x == 0) {
            out[e * 4 + 0] = r.mn; out[e * 4 + 1] = r.mx; out[e * 4 + 2] = r.sum; out[e * 4 + 3] = r.sq;
        }
    }
}

int field_stats_blocks(int64_t rows, int C) {
    const int64_t per_thread = (C == 1) ? 4 : 1;
    const int64_t b = (rows + PR_THREADS * per_thread - 1) / (PR_THREADS * per_thread);
    return (int)(b < 1 ? 1 : (b > FS_MAX_BLOCKS ? FS_MAX_BLOCKS : b));
}

template <int CT>
int field_stats_launch(const float* x, int64_t rows, int C, NormRanges nr, double* out, double* partials, hipStream_t st) {
    const int blocks = field_stats_blocks(rows, C);
    hipLaunchKernelGGL(field_stats_kernel<CT>, dim3(blocks), dim3(PR_THREADS), 0, st, x, rows, C, nr, partials);
    hipLaunchKernelGGL(field_stats_fold_kernel, dim3(1), dim3(PR_THREADS), 0, st, (const double*)partials, blocks, C + 2, out);
    return tdx_launch_status();
}

// ---------------------------------------------------------------------------------------------- W2 k-means
constexpr int W2_MAX_K = 512;
constexpr int W2_MAX_BLOCKS = 512;
constexpr int W2_ROW = 7;  // per centroid in LDS: mean (3), var (3), sum of var; per cluster in the sums: count, mean (3), var (3)

struct W2Plan {
    int64_t tiles;  // tiles of PR_THREADS cells
    int per_block;  // consecutive tiles of one block
    int blocks;
};

W2Plan w2_plan(int64_t n) {
    W2Plan p;
    p.tiles = (n + PR_THREADS - 1) / PR_THREADS;
    p.per_block = (int)((p.tiles + W2_MAX_BLOCKS - 1) / W2_MAX_BLOCKS);
    p.blocks = (int)((p.tiles + p.per_block - 1) / p.per_block);
    return p;
}

// d = sqrt(max(0, |cm - m|^2 + sum cvar + sum var - 2 sum sqrt(cvar var))): everything fp64 but `sum var`, which the
// reference forms in fp32 (numpy sums the float32 array before promoting it).  Block b owns tiles [b per_block,
// (b + 1) per_block); with SUMS it adds its cells to LDS sums per (cluster, component) -- thread i owns item i, i + 256, ...
// and walks the tile's cells in order -- and writes them to partials (blocks, k, 7)
template <bool SUMS>
__global__ void __launch_bounds__(PR_THREADS)
w2n_assign_kernel(const float* __restrict__ mean, const float* __restrict__ var, int64_t n, const double* __restrict__ cmean,
                  const double* __restrict__ cvar, int k, int per_block, int* __restrict__ idx, double* __restrict__ dist,
                  double* __restrict__ partials) {
    extern __shared__ double lds[];
    double* cen = lds;                                                        // (k, 7)
    double* sums = lds + (size_t)k * W2_ROW;                                  // (k, 7), SUMS only
    float* tile_val = reinterpret_cast<float*>(lds + (size_t)(SUMS ? 2 : 1) * k * W2_ROW);  // (256, 6), SUMS only
    int* tile_idx = reinterpret_cast<int*>(tile_val + PR_THREADS * 6);        // (256), SUMS only
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += PR_THREADS) {
        double* r = cen + (size_t)c * W2_ROW;
        for (int e = 0; e < 3; ++e) {
            r[e] = cmean[(size_t)c * 3 + e];
            r[3 + e] = cvar[(size_t)c * 3 + e];
        }
        r[6] = (r[3] + r[4]) + r[5];
    }
    if (SUMS)
        for (int i = tid; i < k * W2_ROW; i += PR_THREADS) sums[i] = 0.0;
    __syncthreads();

    const int64_t tile0 = (int64_t)blockIdx.x * per_block;
    for (int t = 0; t < per_block; ++t) {
        const int64_t base = (tile0 + t) * PR_THREADS;
        if (base >= n) break;  // block-uniform
        const int64_t cell = base + tid;
        const int live = (int)((n - base < PR_THREADS) ? (n - base) : PR_THREADS);
        if (cell < n) {
            float m[3], v[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                m[e] = mean[cell * 3 + e];
                v[e] = var[cell * 3 + e];
            }
            const double sv = (double)((v[0] + v[1]) + v[2]);  // fp32 additions
            const double md[3] = {(double)m[0], (double)m[1], (double)m[2]}, vd[3] = {(double)v[0], (double)v[1], (double)v[2]};
            double best = INFINITY;
            int arg = 0;
            for (int c = 0; c < k; ++c) {
                const double* r = cen + (size_t)c * W2_ROW;
                const double d0 = r[0] - md[0], d1 = r[1] - md[1], d2 = r[2] - md[2];
                const double nrm = (d0 * d0 + d1 * d1) + d2 * d2;
                const double cross = (sqrt(r[3] * vd[0]) + sqrt(r[4] * vd[1])) + sqrt(r[5] * vd[2]);
                const double dsq = fmax(((nrm + r[6]) + sv) - 2.0 * cross, 0.0);
                if (c == 0 || dsq < best) {  // strict: the lowest index wins a tie, as argmin does
                    best = dsq;
                    arg = c;
                }
            }
            idx[cell] = arg;
            dist[cell] = sqrt(best);
            if (SUMS) {
                tile_idx[tid] = arg;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    tile_val[tid * 6 + e] = m[e];
                    tile_val[tid * 6 + 3 + e] = v[e];
                }
            }
        }
        if (SUMS) {
            __syncthreads();
            for (int i = tid; i < k * W2_ROW; i += PR_THREADS) {
                const int c = i / W2_ROW, j = i - c * W2_ROW;
                double a = sums[i];
                for (int p = 0; p < live; ++p)
                    if (tile_idx[p] == c) a += (j == 0) ? 1.0 : (double)tile_val[p * 6 + j - 1];
                sums[i] = a;
            }
            __syncthreads();
        }
    }
    if (SUMS)
        for (int i = tid; i < k * W2_ROW; i += PR_THREADS) partials[(size_t)blockIdx.x * k * W2_ROW + i] = sums[i];
}

// table[i] = partials[0][i] + partials[1][i] + ... in block order, i over (k, 7)
__global__ void __launch_bounds__(PR_THREADS)
w2n_reduce_kernel(const double* __restrict__ partials, int blocks, int items, double* __restrict__ table) {
    const int i = blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= items) return;
    double a = 0.0;
    for (int b = 0; b < blocks; ++b) a += partials[(size_t)b * items + i];
    table[i] = a;
}

}  // namespace

extern "C" int tdx_moments_update(const float* x, int T, int64_t n, double* mean, double* m2, int64_t count, void* stream) {
    TDX_CHECK_ARG(x && mean && m2 && T > 0 && n > 0 && count >= 0);
    const int64_t threads = (n + 3) / 4;
    const int64_t blocks = (threads + PR_THREADS - 1) / PR_THREADS;
    if (blocks > INT_MAX) return TDX_ESHAPE;
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)blocks), dim3(PR_THREADS), 0, as_stream(stream), x, T, n, mean, m2, count);
    return tdx_launch_status();
}

extern "C" size_t tdx_field_stats_workspace_bytes(int64_t rows, int C) {
    if (rows <= 0 || C < 1 || C > FS_MAX_C) return 0;
    return (size_t)field_stats_blocks(rows, C) * (C + 2) * 4 * sizeof(double);
}

extern "C" int tdx_field_stats(const float* x, int64_t rows, int C, int lo0, int hi0, int lo1, int hi1, double* out,
                               void* workspace, void* stream) {
    TDX_CHECK_ARG(x && out && workspace && rows > 0);
    if (C < 1 || C > FS_MAX_C) return TDX_ESHAPE;
    TDX_CHECK_ARG(lo0 >= 0 && lo0 <= hi0 && hi0 <= C && lo1 >= 0 && lo1 <= hi1 && hi1 <= C);
    const NormRanges nr = {{lo0, lo1}, {hi0, hi1}};
    TDX_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    hipStream_t st = as_stream(stream);
    double* ws = (double*)workspace;
    if (C == 1) return field_stats_launch<1>(x, rows, C, nr, out, ws, st);
    if (C == 8) return field_stats_launch<8>(x, rows, C, nr, out, ws, st);
    return field_stats_launch<0>(x, rows, C, nr, out, ws, st);
}

extern "C" int tdx_w2n_blocks(int64_t n) { return n > 0 ? w2_plan(n).blocks : 0; }

extern "C" int tdx_w2n_assign(const float* mean, const float* var, int64_t n, const double* cmean, const double* cvar, int k,
                              int* idx, double* dist, double* partials, void* stream) {
    TDX_CHECK_ARG(mean && var && cmean && cvar && idx && dist && n > 0 && k > 0);
    if (k > W2_MAX_K) return TDX_ESHAPE;
    const W2Plan p = w2_plan(n);
    hipStream_t st = as_stream(stream);
    // at most 2 * 512 * 7 * 8 + 256 * 7 * 4 = 64512 B of dynamic LDS: under the 64 KiB a kernel gets without an attribute
    if (partials) {
        const size_t lds = (size_t)2 * k * W2_ROW * sizeof(double) + PR_THREADS * 7 * sizeof(float);
        hipLaunchKernelGGL(w2n_assign_kernel<true>, dim3(p.blocks), dim3(PR_THREADS), lds, st, mean, var, n, cmean, cvar, k,
                           p.per_block, idx, dist, partials);
    } else {
        const size_t lds = (size_t)k * W2_ROW * sizeof(double);
        hipLaunchKernelGGL(w2n_assign_kernel<false>, dim3(p.blocks), dim3(PR_THREADS), lds, st, mean, var, n, cmean, cvar, k,
                           p.per_block, idx, dist, partials);
    }
    return tdx_launch_status();
}

extern "C" int tdx_w2n_reduce(const double* partials, int blocks, int k, double* table, void* stream) {
    TDX_CHECK_ARG(partials && table && blocks > 0 && k > 0);
    if (k > W2_MAX_K) return TDX_ESHAPE;
    const int items = k * W2_ROW;
    hipLaunchKernelGGL(w2n_reduce_kernel, dim3(ceil_div(items, PR_THREADS)), dim3(PR_THREADS), 0, as_stream(stream), partials,
                       blocks, items, table);
    return tdx_launch_status();
}
