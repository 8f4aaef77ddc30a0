// Case diagnostics (turbdiff_amd/data/diagnostics.py): the reductions behind autocorrelation.npz,
// gaussian-smoothing-error.txt and the mean-forecast baseline.
//   tdx_lagprod_update         : streaming lagged products of the fluctuating velocity.  Three launches per chunk: the chunk's
//                                fluctuations are staged apart from the ring, a column tile of ring + chunk is put in LDS once and
//                                serves every (frame, lag) pair, then the chunk's last frames are retired into the ring
//   tdx_smooth_residual_update : energy of a bank of temporal FIR filters' outputs, fp64 throughout; a column tile of halo +
//                                chunk and the taps sit in LDS, one column per lane, 8 output frames per lane in registers
//   tdx_sqdev_sum              : sum of the float32 squares of x - mean
// All three end in the same tail: per-block fp64 partials in a workspace, each result folded by one block.  No atomics;
// every sum is formed in an order fixed by the shapes alone, so results are bit-reproducible.
#include "tdx_common.h"

#include <climits>

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_WAVES = DG_THREADS / 64;
constexpr int DG_TILE = 64;          // columns of one LDS tile
constexpr int DG_MAX_BLOCKS = 512;   // two blocks of these LDS sizes fit a CU: one round of the grid
constexpr int DG_LOADS = 8;          // global loads a thread has in flight while a tile is staged

// blocks own runs of consecutive column tiles
struct TilePlan {
    int64_t tiles;
    int per_block;
    int blocks;
};

TilePlan tile_plan(int64_t cols) {
    TilePlan p;
    p.tiles = (cols + DG_TILE - 1) / DG_TILE;
    p.per_block = (int)((p.tiles + DG_MAX_BLOCKS - 1) / DG_MAX_BLOCKS);
    p.blocks = (int)((p.tiles + p.per_block - 1) / p.per_block);
    return p;
}

// the shared tail: acc[i] (+)= the sum over the blocks of partials[b][i].  Item i is folded by one block (grid = items):
// thread t adds partials t, t + 256, ... in that order, then the xor butterfly in each wave and the waves in wave order
__global__ void __launch_bounds__(DG_THREADS)
fold_kernel(const double* __restrict__ partials, int blocks, int items, int accumulate, double* __restrict__ acc) {
    __shared__ double red[DG_WAVES];
    const int i = blockIdx.x;
    double a = 0.0;
    for (int b = threadIdx.x; b < blocks; b += DG_THREADS) a += partials[(size_t)b * items + i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < DG_WAVES; ++w) r += red[w];
        acc[i] = accumulate ? acc[i] + r : r;
    }
}

// ---------------------------------------------------------------------------------------------- lagged products
constexpr int LP_MAX_LAG = DG_THREADS - 1;  // thread = lag
constexpr int LP_MAX_FRAMES = 64;           // frames of one call
constexpr int LP_STRIDE = DG_TILE + 1;      // floats between LDS rows: lanes read neighbouring rows of one column

// stage[t, 3 c + e] = x[t, cells[c], e] - mean[cells[c], e], one float32 subtraction (scripts/autocorrelation.py:43)
__global__ void __launch_bounds__(DG_THREADS)
lagprod_stage_kernel(const float* __restrict__ x, int F, int64_t n, const float* __restrict__ mean, const int* __restrict__ cells,
                     int64_t m, float* __restrict__ stage) {
    const int64_t col = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x, cols = 3 * m;
    if (col >= cols) return;
    const int64_t c = col / 3;
    const int e = (int)(col - 3 * c);
    const int64_t src = (int64_t)cells[c] * 3 + e;
    const float mu = mean[src];
    for (int t = 0; t < F; ++t) stage[(int64_t)t * cols + col] = x[(int64_t)t * n * 3 + src] - mu;
}

// LDS row j of a tile is frame seen - L + j: rows [0, L) come from the ring (slot = frame mod L; frames before the first
// are zero rows and never used), rows [L, L + F) from the stage.  Thread i < L + 1 owns lag i and adds, frame by frame and
// column by column, f[L + t] f[L + t - i] (exact in fp64: two float32 factors) for every frame whose partner exists
__global__ void __launch_bounds__(DG_THREADS)
lagprod_kernel(const float* __restrict__ ring, const float* __restrict__ stage, int F, int64_t cols, int L, int64_t seen,
               int per_block, double* __restrict__ partials) {
    extern __shared__ float lp_tile[];  // (L + F, LP_STRIDE)
    const int tid = threadIdx.x, rows = L + F;
    const int64_t tile0 = (int64_t)blockIdx.x * per_block;
    // frame t of the chunk has a partner at lag tid iff seen + t - tid >= 0
    const int t_first = (seen >= tid) ? 0 : (int)(tid - seen);
    double acc = 0.0;
    for (int k = 0; k < per_block; ++k) {
        const int64_t col0 = (tile0 + k) * DG_TILE;
        if (col0 >= cols) break;  // block-uniform
        __syncthreads();          // the previous tile has been read
        // a wave reads 64 neighbouring columns of one row; DG_LOADS rows per thread are in flight before the first is stored
        const int c = tid & 63;
        const int64_t col = col0 + c;
        for (int jb = tid >> 6; jb < rows; jb += DG_WAVES * DG_LOADS) {
            float v[DG_LOADS];
#pragma unroll
            for (int u = 0; u < DG_LOADS; ++u) {
                const int j = jb + u * DG_WAVES;
                v[u] = 0.0f;
                if (col < cols && j < rows) {
                    if (j >= L) {
                        v[u] = stage[(int64_t)(j - L) * cols + col];
                    } else {
                        const int64_t frame = seen - L + j;
                        if (frame >= 0) v[u] = ring[(frame % L) * cols + col];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < DG_LOADS; ++u) {
                const int j = jb + u * DG_WAVES;
                if (j < rows) lp_tile[j * LP_STRIDE + c] = v[u];
            }
        }
        __syncthreads();
        if (tid <= L) {
            for (int t = t_first; t < F; ++t) {
                const float* a = lp_tile + (L + t) * LP_STRIDE;
                const float* b = lp_tile + (L + t - tid) * LP_STRIDE;
#pragma unroll 8
                for (int c = 0; c < DG_TILE; ++c) acc = fma((double)a[c], (double)b[c], acc);
            }
        }
    }
    if (tid <= L) partials[(size_t)blockIdx.x * (L + 1) + tid] = acc;
}

// rows[(seen + t) mod R] = src[t] for the last min(F, R) frames t of the chunk: the hand-over costs the chunk, not the window
__global__ void __launch_bounds__(DG_THREADS)
retire_kernel(const float* __restrict__ src, int F, int64_t cols, int R, int64_t seen, float* __restrict__ rows) {
    const int64_t col = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
    if (col >= cols) return;
    for (int t = (F > R) ? F - R : 0; t < F; ++t) rows[((seen + t) % R) * cols + col] = src[(int64_t)t * cols + col];
}

size_t lagprod_stage_bytes(int F, int64_t m) { return (((size_t)F * 3 * m * sizeof(float)) + 15) & ~(size_t)15; }

// ---------------------------------------------------------------------------------------------- smoothing residual
constexpr int SR_MAX_W = 32;
constexpr int SR_MAX_H = 50;
constexpr int SR_MAX_FRAMES = 64;
constexpr int SR_MAX_TT = 10;                // most output frames a lane holds in registers
constexpr int SR_WPW = SR_MAX_W / DG_WAVES;  // filters of one wave: w = wave, wave + 4, ...

// steps of one group of TT outputs: K + TT - 1 rows, rounded up to whole turns of the tap registers
__host__ __device__ constexpr int sr_steps(int K, int TT) { return (K + TT - 1 + TT - 1) / TT * TT; }
// LDS rows: the last group starts at the largest multiple of TT below F_out
__host__ __device__ constexpr int sr_rows(int F_out, int K, int TT) { return (F_out + TT - 1) / TT * TT - TT + sr_steps(K, TT); }

// Window row j is frame seen - hh + j: the hh = min(seen, 2 h) frames of the halo (slot = frame mod 2 h), then the chunk.
// Output frame t < F_out of filter w is o = sum_k taps[w, k] x[t + k] in fp64, k ascending; the lane adds o^2, t ascending.
// A lane forms TT outputs at once: step kk reads row tg + kk once and tap kk once (a broadcast), and feeds the TT outputs
// whose window holds that row with taps kk, kk - 1, ... kept in a register file that rotates at compile time.  Taps past
// the end are stored zeros, and the outputs past F_out that a last group forms from the zero rows below the window are
// dropped; the launcher picks the TT that wastes the fewest steps on them.  The arithmetic of an output does not depend on TT
template <int TT>
__global__ void __launch_bounds__(DG_THREADS)
smooth_residual_kernel(const float* __restrict__ halo, const float* __restrict__ x, int F, int64_t n, const double* __restrict__ taps,
                       int W, int h, int64_t seen, int F_out, int per_block, double* __restrict__ partials) {
    extern __shared__ double sr_lds[];
    const int K = 2 * h + 1, H2 = 2 * h, steps = sr_steps(K, TT), trow = steps;  // taps row: K taps, then zeros up to `steps`
    const int rows_lds = sr_rows(F_out, K, TT);
    double* tp = sr_lds;                                             // (W, trow)
    float* tile = reinterpret_cast<float*>(sr_lds + (size_t)W * trow);  // (rows_lds, DG_TILE)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = (int)((seen < H2) ? seen : H2), rows = hh + F;
    for (int i = tid; i < W * trow; i += DG_THREADS) {
        const int w = i / trow, k = i - w * trow;
        tp[i] = (k < K) ? taps[w * K + k] : 0.0;
    }
    double acc[SR_WPW];
#pragma unroll
    for (int q = 0; q < SR_WPW; ++q) acc[q] = 0.0;
    const int64_t tile0 = (int64_t)blockIdx.x * per_block;
    for (int kt = 0; kt < per_block; ++kt) {
        const int64_t col0 = (tile0 + kt) * DG_TILE;
        if (col0 >= n) break;  // block-uniform
        __syncthreads();
        const int64_t col = col0 + lane;
        for (int jb = wave; jb < rows_lds; jb += DG_WAVES * DG_LOADS) {
            float v[DG_LOADS];
#pragma unroll
            for (int u = 0; u < DG_LOADS; ++u) {
                const int j = jb + u * DG_WAVES;
                v[u] = 0.0f;
                if (col < n && j < rows) {
                    if (j >= hh) v[u] = x[(int64_t)(j - hh) * n + col];
                    else v[u] = halo[((seen - hh + j) % H2) * n + col];
                }
            }
#pragma unroll
            for (int u = 0; u < DG_LOADS; ++u) {
                const int j = jb + u * DG_WAVES;
                if (j < rows_lds) tile[j * DG_TILE + lane] = v[u];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SR_WPW; ++q) {
            const int w = wave + q * DG_WAVES;
            if (w >= W) break;  // wave-uniform
            const double* tw = tp + (size_t)w * trow;
            double a = acc[q];
            for (int tg = 0; tg < F_out; tg += TT) {
                double o[TT], tr[TT];
#pragma unroll
                for (int j = 0; j < TT; ++j) o[j] = 0.0, tr[j] = 0.0;
                const float* col = tile + tg * DG_TILE + lane;
                for (int kk0 = 0; kk0 < steps; kk0 += TT) {
#pragma unroll
                    for (int u = 0; u < TT; ++u) {
                        const double xv = (double)col[(kk0 + u) * DG_TILE];
                        tr[u] = tw[kk0 + u];  // tap kk lives in slot kk mod TT until tap kk + TT replaces it
#pragma unroll
                        for (int j = 0; j < TT; ++j) o[j] = fma(tr[(u - j + TT) % TT], xv, o[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < TT; ++j)
                    if (tg + j < F_out) a = fma(o[j], o[j], a);
            }
            acc[q] = a;
        }
    }
#pragma unroll
    for (int q = 0; q < SR_WPW; ++q) {
        const int w = wave + q * DG_WAVES;
        if (w >= W) break;
        const double s = wave_sum(acc[q]);
        if (lane == 0) partials[(size_t)blockIdx.x * W + w] = s;
    }
}

size_t sr_lds_bytes(int W, int K, int F_out, int TT) {
    return (size_t)W * sr_steps(K, TT) * sizeof(double) + (size_t)sr_rows(F_out, K, TT) * DG_TILE * sizeof(float);
}

// steps spent on F_out outputs with groups of TT, each step = TT FMAs and three instructions to fetch a row and a tap
int64_t sr_cost(int F_out, int K, int TT) { return (int64_t)((F_out + TT - 1) / TT) * sr_steps(K, TT) * (TT + 3); }

template <int TT>
int sr_launch(const TilePlan& p, hipStream_t st, const float* halo, const float* x, int F, int64_t n, const double* taps, int W,
              int h, int64_t seen, int F_out, double* partials) {
    // no request exceeds the filter bank at its limits with a full chunk: steps <= K + 2 TT - 2, rows <= F_out + steps
    constexpr int steps_max = 2 * SR_MAX_H + 1 + 2 * SR_MAX_TT - 2;
    constexpr size_t lds_max = (size_t)SR_MAX_W * steps_max * sizeof(double) + (size_t)(SR_MAX_FRAMES + steps_max) * DG_TILE * sizeof(float);
    static_assert(TT <= SR_MAX_TT && lds_max <= 160 * 1024, "LDS of one CU");
    return tdx_launch_lds_max<smooth_residual_kernel<TT>>(dim3(p.blocks), dim3(DG_THREADS), lds_max,
                                                          sr_lds_bytes(W, 2 * h + 1, F_out, TT), st, halo, x, F, n, taps, W, h, seen,
                                                          F_out, p.per_block, partials);
}

// ---------------------------------------------------------------------------------------------- squared deviation
constexpr int SD_MAX_BLOCKS = 1024;

int sqdev_blocks(int64_t cols) {
    const int64_t b = (cols + DG_THREADS - 1) / DG_THREADS;
    return (int)(b < 1 ? 1 : (b > SD_MAX_BLOCKS ? SD_MAX_BLOCKS : b));
}

// thread = column (grid stride), frames in order; difference and square are rounded to fp32 one by one, as
// `(x - mean) ** 2` on float32 arrays is (scripts/mean-forecast-errors.py:42-43), and widened before they are summed
__global__ void __launch_bounds__(DG_THREADS)
sqdev_kernel(const float* __restrict__ x, const float* __restrict__ mean, int T, int64_t cols, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[DG_WAVES];
    double s = 0.0;
    for (int64_t col = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x; col < cols; col += (int64_t)gridDim.x * DG_THREADS) {
        const float mu = mean[col];
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            const float d = x[(int64_t)t * cols + col] - mu;
            const float dd = d * d;
            s += (double)dd;
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < DG_WAVES; ++w) r += red[w];
        partials[blockIdx.x] = r;
    }
}

// ---------------------------------------------------------------------------------------------- fp64 rate probe
constexpr int FP_CHAINS = 8;

// nothing but dependent fp64 FMAs on registers, FP_CHAINS independent chains per lane: the rate the smoothing kernel's
// arithmetic could reach at best (tools/diagnostics_bench.py times it in the same run as the kernel)
__global__ void __launch_bounds__(DG_THREADS)
fma64_probe_kernel(double* __restrict__ out, int iters, double b, double c) {
    double a[FP_CHAINS];
#pragma unroll
    for (int j = 0; j < FP_CHAINS; ++j) a[j] = (double)(threadIdx.x + j);
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < FP_CHAINS; ++j) a[j] = fma(a[j], b, c);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < FP_CHAINS; ++j) s += a[j];
    out[(size_t)blockIdx.x * DG_THREADS + threadIdx.x] = s;
}

}  // namespace

extern "C" int tdx_fma64_probe(double* out, int blocks, int iters, void* stream) {
    TDX_CHECK_ARG(out && blocks >= 1 && iters >= 1);
    static_assert(FP_CHAINS == 8, "include/tdx.h states 8 chains per thread");
    hipLaunchKernelGGL(fma64_probe_kernel, dim3(blocks), dim3(DG_THREADS), 0, as_stream(stream), out, iters, 0.999999, 1e-6);
    return tdx_launch_status();
}

extern "C" size_t tdx_lagprod_workspace_bytes(int F, int64_t m, int L) {
    if (F < 1 || F > LP_MAX_FRAMES || m < 1 || L < 1 || L > LP_MAX_LAG) return 0;
    return lagprod_stage_bytes(F, m) + (size_t)tile_plan(3 * m).blocks * (L + 1) * sizeof(double);
}

extern "C" int tdx_lagprod_update(const float* x, int F, int64_t n, const float* mean, const int* cells, int64_t m, int L,
                                  float* ring, double* acc, int64_t seen, void* workspace, void* stream) {
    TDX_CHECK_ARG(x && mean && cells && ring && acc && workspace && F >= 1 && n >= 1 && m >= 1 && m <= n && L >= 1 && seen >= 0);
    if (F > LP_MAX_FRAMES || L > LP_MAX_LAG) return TDX_ESHAPE;
    TDX_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
    const int64_t cols = 3 * m;
    const int64_t col_blocks = (cols + DG_THREADS - 1) / DG_THREADS;
    if (col_blocks > INT_MAX) return TDX_ESHAPE;
    hipStream_t st = as_stream(stream);
    float* stage = (float*)workspace;
    double* partials = (double*)((char*)workspace + lagprod_stage_bytes(F, m));
    const TilePlan p = tile_plan(cols);
    hipLaunchKernelGGL(lagprod_stage_kernel, dim3((unsigned)col_blocks), dim3(DG_THREADS), 0, st, x, F, n, mean, cells, m, stage);
    const size_t lds = (size_t)(L + F) * LP_STRIDE * sizeof(float);
    constexpr size_t lds_max = (size_t)(LP_MAX_LAG + LP_MAX_FRAMES) * LP_STRIDE * sizeof(float);  // 82 940 B of the CU's 160 KiB
    int rc = tdx_launch_lds_max<lagprod_kernel>(dim3(p.blocks), dim3(DG_THREADS), lds_max, lds, st, (const float*)ring,
                                                (const float*)stage, F, cols, L, seen, p.per_block, partials);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(fold_kernel, dim3(L + 1), dim3(DG_THREADS), 0, st, (const double*)partials, p.blocks, L + 1, 1, acc);
    hipLaunchKernelGGL(retire_kernel, dim3((unsigned)col_blocks), dim3(DG_THREADS), 0, st, (const float*)stage, F, cols, L, seen, ring);
    return tdx_launch_status();
}

extern "C" size_t tdx_smooth_residual_workspace_bytes(int64_t n, int W) {
    if (n < 1 || W < 1 || W > SR_MAX_W) return 0;
    return (size_t)tile_plan(n).blocks * W * sizeof(double);
}

extern "C" int tdx_smooth_residual_update(const float* x, int F, int64_t n, const double* taps, int W, int h, float* halo,
                                          double* acc, int64_t seen, void* workspace, void* stream) {
    TDX_CHECK_ARG(x && taps && halo && acc && workspace && F >= 1 && n >= 1 && W >= 1 && h >= 1 && seen >= 0);
    if (F > SR_MAX_FRAMES || W > SR_MAX_W || h > SR_MAX_H) return TDX_ESHAPE;
    TDX_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    const int64_t col_blocks = (n + DG_THREADS - 1) / DG_THREADS;
    if (col_blocks > INT_MAX) return TDX_ESHAPE;
    hipStream_t st = as_stream(stream);
    const int K = 2 * h + 1, H2 = 2 * h;
    const int64_t before = seen > H2 ? seen - H2 : 0, after = seen + F > H2 ? seen + F - H2 : 0;
    const int F_out = (int)(after - before);
    if (F_out > 0) {
        const TilePlan p = tile_plan(n);
        double* partials = (double*)workspace;
        const int64_t c5 = sr_cost(F_out, K, 5), c8 = sr_cost(F_out, K, 8), c10 = sr_cost(F_out, K, 10);
        int rc;
        if (c10 <= c8 && c10 <= c5) rc = sr_launch<10>(p, st, halo, x, F, n, taps, W, h, seen, F_out, partials);
        else if (c8 <= c5) rc = sr_launch<8>(p, st, halo, x, F, n, taps, W, h, seen, F_out, partials);
        else rc = sr_launch<5>(p, st, halo, x, F, n, taps, W, h, seen, F_out, partials);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(fold_kernel, dim3(W), dim3(DG_THREADS), 0, st, (const double*)partials, p.blocks, W, 1, acc);
    }
    hipLaunchKernelGGL(retire_kernel, dim3((unsigned)col_blocks), dim3(DG_THREADS), 0, st, x, F, n, H2, seen, halo);
    return tdx_launch_status();
}

extern "C" size_t tdx_sqdev_workspace_bytes(int64_t n, int C) {
    if (n < 1 || C < 1 || C > 4) return 0;
    return (size_t)sqdev_blocks(n * C) * sizeof(double);
}

extern "C" int tdx_sqdev_sum(const float* x, const float* mean, int T, int64_t n, int C, int accumulate, double* out,
                             void* workspace, void* stream) {
    TDX_CHECK_ARG(x && mean && out && workspace && T >= 1 && n >= 1);
    if (C < 1 || C > 4) return TDX_ESHAPE;
    TDX_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    hipStream_t st = as_stream(stream);
    const int64_t cols = n * C;
    const int blocks = sqdev_blocks(cols);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(sqdev_kernel, dim3(blocks), dim3(DG_THREADS), 0, st, x, mean, T, cols, partials);
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(DG_THREADS), 0, st, (const double*)partials, blocks, 1, accumulate ? 1 : 0, out);
    return tdx_launch_status();
}
