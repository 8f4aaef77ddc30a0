// 1x1x1 convolution / per-row linear layer on NDHWC activations (vector-ALU version).
//   y[r, :] = bias + [x1 | x2][r, :] @ w  (+ add[r, :])
// 64 rows x 64 cols per 256-thread block, 4x4 register tile per thread, K staged through
// LDS in 32-deep slices (x slice stored k-major so the inner loop reads conflict-free
// float4 rows).  f32 accumulation.  These layers are HBM-bound at the U-Net's channel
// counts (4-174 FLOP/B); the MFMA versions live in tdx_conv1_mfma.hip and tdx_conv1_mfma_f32.hip.  Also here: the family's
// host side -- conv1_route (TDX_CONV1_IMPL=direct forces the kernels of this file), conv1_wgrad_plan, the entry points.
#include "tdx_common.h"
#include "tdx_conv1.h"
#include "tdx_runtime.h"
#include <algorithm>

#define C1_BM 64
#define C1_BN 64
#define C1_BK 32

template <typename T>
__global__ void __launch_bounds__(256)
conv1_fwd_kernel(const T* __restrict__ x1, int C1, const T* __restrict__ x2, int C2, const float* __restrict__ w,
                 int ldw, const float* __restrict__ bias, const T* __restrict__ add, T* __restrict__ y, int64_t rows,
                 int Cout) {
    __shared__ float xs[C1_BK][C1_BM + 4];
    __shared__ float ws[C1_BK][C1_BN + 4];
    const int Cin = C1 + C2;
    const int64_t r0 = (int64_t)blockIdx.x * C1_BM;
    const int n0 = blockIdx.y * C1_BN;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int k0 = 0; k0 < Cin; k0 += C1_BK) {
        // stage x slice: 64 rows x 32 k  (thread: row = tid/4, 8 consecutive k)
        {
            const int rr = tid >> 2, kk = (tid & 3) * 8;
            const int64_t r = r0 + rr;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + kk + j;
                float v = 0.f;
                if (r < rows && k < Cin) v = (k < C1) ? ldf(x1 + r * C1 + k) : ldf(x2 + r * C2 + (k - C1));
                xs[kk + j][rr] = v;
            }
        }
        // stage w slice: 32 k x 64 n
        {
            const int kk = tid >> 3, nn = (tid & 7) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + kk, n = n0 + nn + j;
                ws[kk][nn + j] = (k < Cin && n < Cout) ? w[(size_t)k * ldw + n] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < C1_BK; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&xs[k][ty * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&ws[k][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + ty * 4 + i;
        if (r >= rows) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= Cout) continue;
            float v = acc[i][j];
            if (bias) v += bias[n];
            if (add) v += ldf(add + r * Cout + n);
            stf(y + r * Cout + n, v);
        }
    }
}

Conv1Route conv1_route(int dtype, int C1, int C2, int Cout, int ldw, unsigned w_mod16, bool gn_tail) {
    const bool mfma = tdx_switch(SW_CONV1_IMPL) == 0;  // TDX_CONV1_IMPL=direct: the vector-ALU kernels of this file
    const int nt = (Cout % 64 == 0) ? 2 : 1;  // NT = 4 needs 270 registers on the 16-bit kernel: 1 wave/SIMD, too few loads in flight
    if (!tdx_is_h16(dtype) && (dtype != TDX_F32 || gn_tail)) return {TDX_CONV1_VECTOR, 0, TDX_EDTYPE};
    if (tdx_is_h16(dtype) && mfma && conv1_mfma_supported(C1, C2, Cout)) return {TDX_CONV1_H16, nt, TDX_OK};
    if (gn_tail) return {TDX_CONV1_VECTOR, 0, TDX_ESHAPE};
    if (dtype == TDX_F32 && mfma && conv1_mfma_f32_supported(C1, C2, Cout, ldw, w_mod16)) return {TDX_CONV1_F32, nt, TDX_OK};
    return {TDX_CONV1_VECTOR, 0, TDX_OK};
}

int conv1_vector_fwd_launch(const Conv1Call& c, const Conv1Route& r) {
    if (r.status != TDX_OK || r.family != TDX_CONV1_VECTOR) return TDX_EINVAL;
    dim3 grid(ceil_div(c.rows, C1_BM), ceil_div(c.Cout, C1_BN));
    TDX_DISPATCH_DTYPE(c.fmt, hipLaunchKernelGGL((conv1_fwd_kernel<T>), grid, dim3(256), 0, c.st, (const T*)c.x1, c.C1,
                                                 (const T*)c.x2, c.C2, c.w, c.ldw, c.bias, (const T*)c.add, (T*)c.y, c.rows, c.Cout));
    return tdx_launch_status();
}

static int conv1_fwd_impl(const Conv1Call& c) {
    const Conv1Route r = conv1_route(c.fmt, c.C1, c.C2, c.Cout, c.ldw, (unsigned)((uintptr_t)c.w % 16), c.gn.stats != nullptr);
    if (r.status != TDX_OK) return r.status;
    if (r.family == TDX_CONV1_H16) return conv1_mfma_fwd_launch(c, r);
    return r.family == TDX_CONV1_F32 ? conv1_mfma_f32_fwd_launch(c, r) : conv1_vector_fwd_launch(c, r);
}

extern "C" int tdx_conv1_fwd(const void* x1, int C1, const void* x2, int C2, const float* w, int ldw,
                             const float* bias, const void* add, void* y, int64_t rows, int Cout, int dtype,
                             void* stream) {
    TDX_CHECK_ARG(x1 && w && y && rows > 0 && C1 > 0 && C2 >= 0 && Cout > 0 && ldw >= Cout);
    TDX_CHECK_ARG(C2 == 0 || x2);
    return conv1_fwd_impl({x1, C1, x2, C2, w, ldw, bias, add, y, rows, Cout, dtype, as_stream(stream), {nullptr, nullptr, nullptr, 1, 1}});
}

extern "C" int tdx_conv1_fwd_plan(int C1, int C2, int Cout, int ldw, int w_mod16, int has_add, int gn_tail, int dtype, int* plan) {
    TDX_CHECK_ARG(plan && C1 > 0 && C2 >= 0 && Cout > 0 && ldw >= Cout && (!gn_tail || has_add));
    const Conv1Route r = conv1_route(dtype, C1, C2, Cout, ldw, (unsigned)w_mod16 % 16, gn_tail != 0);
    static const int tile_rows[] = {C1_BM, C1M_ROWS, F1_ROWS};  // by TDX_CONV1_*
    for (int i = 0; i < TDX_CONV1_PLAN_INTS; ++i) plan[i] = 0;
    plan[TDX_CONV1_PLAN_KERNEL] = r.family;
    plan[TDX_CONV1_PLAN_NT] = r.nt;
    plan[TDX_CONV1_PLAN_TILE_ROWS] = tile_rows[r.family];
    return r.status;
}

// y = silu(GroupNorm(h)) + bias + [x1|x2] @ w: the tail of a ResnetBlock with a projected skip in one pass (bf16 / fp16 tensors on
// the matrix-core kernel; TDX_ESHAPE / TDX_EDTYPE otherwise: the caller then runs tdx_conv1_fwd + tdx_gn_apply).
extern "C" int tdx_conv1_fwd_gn(const void* x1, int C1, const void* x2, int C2, const float* w, int ldw, const float* bias,
                                const void* h, const float* stats, const float* gamma, const float* beta, int groups,
                                void* y, int B, int64_t V, int Cout, int dtype, void* stream) {
    TDX_CHECK_ARG(x1 && w && y && h && stats && gamma && beta && B > 0 && V > 0 && C1 > 0 && C2 >= 0 && Cout > 0 && ldw >= Cout);
    TDX_CHECK_ARG((C2 == 0 || x2) && groups > 0 && (Cout % groups) == 0);
    return conv1_fwd_impl({x1, C1, x2, C2, w, ldw, bias, h, y, (int64_t)B * V, Cout, dtype, as_stream(stream), {stats, gamma, beta, groups, V}});
}

// dw[ci][co] = sum_r x[r,ci] dy[r,co]; each block reduces a chunk of rows for one
// 64x64 (ci, co) tile and merges with f32 atomics (dw is zeroed first).
#define C1W_ROWS 4096
template <typename T>
__global__ void __launch_bounds__(256)
conv1_wgrad_kernel(const T* __restrict__ x, int Cin, const T* __restrict__ dy, int Cout, float* __restrict__ dw,
                   int ldw, float* __restrict__ dbias, int64_t rows, int transposed, int64_t rows_per_block,
                   int64_t split_stride) {
    __shared__ float xs[C1_BK][C1_BM + 4];  // [row slice][ci]
    __shared__ float gs[C1_BK][C1_BN + 4];  // [row slice][co]
    const int64_t rbeg = (int64_t)blockIdx.x * rows_per_block;
    const int64_t rend = min(rows, rbeg + rows_per_block);
    dw += (int64_t)blockIdx.x * split_stride;  // TDX_DETERMINISTIC: one zeroed slab per row chunk
    if (dbias) dbias += (int64_t)blockIdx.x * split_stride;
    const int ci0 = blockIdx.y * C1_BM, co0 = blockIdx.z * C1_BN;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    float bsum = 0.f;  // thread tid < 64 sums column co0 + tid when ci tile == 0

    for (int64_t rs = rbeg; rs < rend; rs += C1_BK) {
        {
            const int rr = tid >> 3, cc = (tid & 7) * 8;
            const int64_t r = rs + rr;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ci = ci0 + cc + j, co = co0 + cc + j;
                xs[rr][cc + j] = (r < rend && ci < Cin) ? ldf(x + r * Cin + ci) : 0.f;
                gs[rr][cc + j] = (r < rend && co < Cout) ? ldf(dy + r * Cout + co) : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < C1_BK; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&xs[k][ty * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&gs[k][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
        }
        if (dbias && blockIdx.y == 0 && tid < C1_BN) {
#pragma unroll 8
            for (int k = 0; k < C1_BK; ++k) bsum += gs[k][tid];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ci = ci0 + ty * 4 + i;
        if (ci >= Cin) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + tx * 4 + j;
            if (co < Cout) atomicAdd(&dw[transposed ? (size_t)co * ldw + ci : (size_t)ci * ldw + co], acc[i][j]);
        }
    }
    if (dbias && blockIdx.y == 0 && tid < C1_BN && co0 + tid < Cout) atomicAdd(&dbias[co0 + tid], bsum);
}

void conv1_wgrad_vector_plan(Conv1WgradPlan& p, int64_t rows, int max_split) {
    int64_t rpb = C1W_ROWS;
    if (max_split > 0 && ceil_div(rows, rpb) > max_split) rpb = (ceil_div(rows, max_split) + C1_BK - 1) / C1_BK * C1_BK;
    p.kernel = TDX_CONV1_VECTOR;
    p.mt = p.nt = 0;
    p.nsplit = ceil_div(rows, rpb);
    p.step_rows = C1_BK;
    p.rows_per_split = rpb;
}

int conv1_wgrad_vector_launch(const Conv1WgradCall& c, const Conv1WgradPlan& p) {
    if (p.status != TDX_OK || p.kernel != TDX_CONV1_VECTOR) return TDX_EINVAL;
    dim3 grid(p.nsplit, ceil_div(c.Cin, C1_BM), ceil_div(c.Cout, C1_BN));
    TDX_DISPATCH_DTYPE(c.fmt, hipLaunchKernelGGL((conv1_wgrad_kernel<T>), grid, dim3(256), 0, c.st, (const T*)c.x, c.Cin,
                                                 (const T*)c.dy, c.Cout, c.dw, c.ldw, c.dbias, c.rows, c.transposed ? 1 : 0,
                                                 p.rows_per_split, p.slab_stride));
    return tdx_launch_status();
}

Conv1WgradPlan conv1_wgrad_plan(int dtype, int Cin, int Cout, int64_t rows) {
    Conv1WgradPlan p = {};
    int max_split = 0;  // the kernel's own choice
    int64_t slab = 0;
    if (tdx_deterministic()) {
        slab = ((int64_t)Cin * Cout + Cout + 63) / 64 * 64;  // [nrow][ncol] compact, then the bias gradient
        const int64_t room =
            tdx_scratch_ptr() ? ((int64_t)tdx_scratch_bytes() - TDX_SCRATCH_SLAB_OFFSET) / (int64_t)sizeof(float) / slab : 0;
        max_split = (int)std::min<int64_t>(room, 256);
        if (max_split < 2) max_split = 1, slab = 0;  // fewer than two slabs: one split straight into dw
    }
    // the family the forward of these channels takes (no weight matrix is read: ldw = 0 at address 0 passes the fp32
    // kernel's clauses on it), where the weight-gradient kernel of that family takes them too
    const Conv1Route r = conv1_route(dtype, Cin, 0, Cout, 0, 0, false);
    p.status = r.status;
    if (r.family == TDX_CONV1_H16 && conv1_wgrad_mfma_supported(Cin, Cout)) conv1_wgrad_mfma_plan(p, Cin, Cout, rows, max_split);
    else if (r.family == TDX_CONV1_F32 && conv1_wgrad_mfma_f32_supported(Cin, Cout)) conv1_wgrad_mfma_f32_plan(p, Cin, Cout, rows, max_split);
    else conv1_wgrad_vector_plan(p, rows, max_split);
    p.nslab = slab ? p.nsplit : 0;  // often far fewer than allowed: only those slabs are zeroed and summed
    p.slab_stride = slab;
    return p;
}

static int conv1_bwd_weight_impl(const Conv1WgradCall& c) {
    const Conv1WgradPlan p = conv1_wgrad_plan(c.fmt, c.Cin, c.Cout, c.rows);
    if (p.status != TDX_OK) return p.status;
    const int nrow = c.transposed ? c.Cout : c.Cin, ncol = c.transposed ? c.Cin : c.Cout;
    Conv1WgradCall k = c;  // where the kernel adds: the block itself, or the slabs
    int rc = TDX_OK;
    if (p.nslab > 0) {
        float* slabs = reinterpret_cast<float*>(tdx_scratch_region(TDX_SCRATCH_SLAB_OFFSET, (size_t)p.nslab * p.slab_stride * sizeof(float)));
        if (slabs == nullptr) return TDX_EINVAL;
        k.dw = slabs, k.ldw = ncol, k.dbias = c.dbias ? slabs + (int64_t)nrow * ncol : nullptr;
        rc = tdx_zero_async(slabs, (size_t)p.nslab * p.slab_stride * sizeof(float), c.st);
    } else if (!c.accumulate) {
        // zero the block that is written (ldw may exceed the row length for sub-blocks)
        rc = tdx_zero2d_async(c.dw, (size_t)c.ldw * sizeof(float), (size_t)ncol * sizeof(float), (size_t)nrow, c.st);
        if (rc == TDX_OK && c.dbias) rc = tdx_zero_async(c.dbias, (size_t)c.Cout * sizeof(float), c.st);
    }
    if (rc != TDX_OK) return rc;
    rc = p.kernel == TDX_CONV1_H16   ? conv1_wgrad_mfma_launch(k, p)
         : p.kernel == TDX_CONV1_F32 ? conv1_wgrad_mfma_f32_launch(k, p)
                                     : conv1_wgrad_vector_launch(k, p);
    if (rc != TDX_OK || p.nslab == 0) return rc;
    rc = ordered_sum_launch(k.dw, p.nslab, p.slab_stride, c.dw, nrow, ncol, c.ldw, c.accumulate, c.st);
    if (rc != TDX_OK || !c.dbias) return rc;
    return ordered_sum_launch(k.dbias, p.nslab, p.slab_stride, c.dbias, 1, c.Cout, c.Cout, c.accumulate, c.st);
}

extern "C" int tdx_conv1_bwd_weight_plan(int Cin, int Cout, int64_t rows, int transposed, int dtype, int* plan) {
    TDX_CHECK_ARG(plan && rows > 0 && Cin > 0 && Cout > 0);
    (void)transposed;  // the layout of dw changes the kernel's TR argument and nothing of the plan
    const Conv1WgradPlan p = conv1_wgrad_plan(dtype, Cin, Cout, rows);
    for (int i = 0; i < TDX_CONV1_PLAN_INTS; ++i) plan[i] = 0;
    plan[TDX_CONV1_PLAN_KERNEL] = p.kernel;
    plan[TDX_CONV1_PLAN_NT] = p.nt;
    plan[TDX_CONV1_PLAN_MT] = p.mt;
    plan[TDX_CONV1_PLAN_NSPLIT] = p.nsplit;
    plan[TDX_CONV1_PLAN_NSLAB] = p.nslab;
    plan[TDX_CONV1_PLAN_STEP_ROWS] = p.step_rows;
    plan[TDX_CONV1_PLAN_ROWS_PER_SPLIT] = (int)std::min<int64_t>(p.rows_per_split, INT32_MAX);
    return p.status;
}

extern "C" int tdx_conv1_bwd_weight(const void* x, int Cin, const void* dy, int Cout, float* dw, int ldw,
                                    float* dbias, int64_t rows, int dtype, void* stream) {
    TDX_CHECK_ARG(x && dy && dw && rows > 0 && Cin > 0 && Cout > 0 && ldw >= Cout);
    return conv1_bwd_weight_impl({x, Cin, dy, Cout, dw, ldw, dbias, rows, false, false, dtype, as_stream(stream)});
}

extern "C" int tdx_conv1_bwd_weight_oc(const void* x, int Cin, const void* dy, int Cout, float* dw, int ldw,
                                       float* dbias, int accumulate, int64_t rows, int dtype, void* stream) {
    TDX_CHECK_ARG(x && dy && dw && rows > 0 && Cin > 0 && Cout > 0 && ldw >= Cin);
    return conv1_bwd_weight_impl({x, Cin, dy, Cout, dw, ldw, dbias, rows, true, accumulate != 0, dtype, as_stream(stream)});
}
