// DDPM noise / denoise arithmetic, masked loss, layout transforms and the Philox generator.
// All HBM-bound streaming kernels: 16 B per lane, grid-stride, no LDS needed except for
// the (B,C,V) <-> (B,V,C) transposes which go through an LDS tile so that both sides are
// coalesced.
#include "tdx_common.h"
#include "tdx_runtime.h"  // tdx_deterministic

extern "C" int tdx_version(void) { return 1; }
extern "C" const char* tdx_arch(void) { return "gfx950"; }

// ------------------------------------------------------------------ layout ---------------
// (B, C, V) -> (B, V, C): tile of 64 voxels x C channels (C <= 64 per pass) through LDS.
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) ncv_to_nvc_kernel(const TI* __restrict__ x, TO* __restrict__ y, int C, int64_t V) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * 64;
    const int64_t v0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
    const int nc = min(64, C - c0);
    for (int c = ty; c < nc; c += 4) {
        int64_t v = v0 + tx;
        if (v < V) tile[c][tx] = ldf(x + ((int64_t)b * C + c0 + c) * V + v);
    }
    __syncthreads();
    // write: consecutive threads -> consecutive channels of one voxel
    for (int i = threadIdx.x; i < 64 * nc; i += 256) {
        int vv = i / nc, c = i - vv * nc;
        int64_t v = v0 + vv;
        if (v < V) stf(y + ((int64_t)b * V + v) * C + c0 + c, tile[c][vv]);
    }
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(256) nvc_to_ncv_kernel(const TI* __restrict__ x, TO* __restrict__ y, int C, int64_t V) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * 64;
    const int64_t v0 = (int64_t)blockIdx.x * 64;
    const int nc = min(64, C - c0);
    for (int i = threadIdx.x; i < 64 * nc; i += 256) {
        int vv = i / nc, c = i - vv * nc;
        int64_t v = v0 + vv;
        if (v < V) tile[c][vv] = ldf(x + ((int64_t)b * V + v) * C + c0 + c);
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c = ty; c < nc; c += 4) {
        int64_t v = v0 + tx;
        if (v < V) stf(y + ((int64_t)b * C + c0 + c) * V + v, tile[c][tx]);
    }
}

template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) stf(y + i, ldf(x + i));
}

#define DISPATCH2(di, dto, CALL)                                                   \
    do {                                                                           \
        if ((di) == TDX_F32 && (dto) == TDX_F32) { typedef float TI; typedef float TO; CALL; }      \
        else if ((di) == TDX_F32 && (dto) == TDX_BF16) { typedef float TI; typedef bf16 TO; CALL; } \
        else if ((di) == TDX_BF16 && (dto) == TDX_F32) { typedef bf16 TI; typedef float TO; CALL; } \
        else if ((di) == TDX_BF16 && (dto) == TDX_BF16) { typedef bf16 TI; typedef bf16 TO; CALL; } \
        else if ((di) == TDX_F32 && (dto) == TDX_F16) { typedef float TI; typedef f16 TO; CALL; }   \
        else if ((di) == TDX_F16 && (dto) == TDX_F32) { typedef f16 TI; typedef float TO; CALL; }   \
        else if ((di) == TDX_F16 && (dto) == TDX_F16) { typedef f16 TI; typedef f16 TO; CALL; }     \
        else return TDX_EDTYPE;                                                    \
    } while (0)

extern "C" int tdx_ncv_to_nvc(const void* x, void* y, int B, int C, int64_t V, int di, int dto, void* stream) {
    TDX_CHECK_ARG(x && y && B > 0 && C > 0 && V > 0);
    dim3 grid(ceil_div(V, 64), ceil_div(C, 64), B);
    DISPATCH2(di, dto, hipLaunchKernelGGL((ncv_to_nvc_kernel<TI, TO>), grid, dim3(256), 0, as_stream(stream),
                                           (const TI*)x, (TO*)y, C, V));
    return tdx_launch_status();
}
extern "C" int tdx_nvc_to_ncv(const void* x, void* y, int B, int C, int64_t V, int di, int dto, void* stream) {
    TDX_CHECK_ARG(x && y && B > 0 && C > 0 && V > 0);
    dim3 grid(ceil_div(V, 64), ceil_div(C, 64), B);
    DISPATCH2(di, dto, hipLaunchKernelGGL((nvc_to_ncv_kernel<TI, TO>), grid, dim3(256), 0, as_stream(stream),
                                           (const TI*)x, (TO*)y, C, V));
    return tdx_launch_status();
}
extern "C" int tdx_cast(const void* x, void* y, int64_t n, int di, int dto, void* stream) {
    TDX_CHECK_ARG(x && y && n > 0);
    int grid = (int)min((int64_t)2048, (n + 255) / 256);
    DISPATCH2(di, dto, hipLaunchKernelGGL((cast_kernel<TI, TO>), dim3(grid), dim3(256), 0, as_stream(stream),
                                           (const TI*)x, (TO*)y, n));
    return tdx_launch_status();
}

// ------------------------------------------------------------------ cell mask ------------
__global__ void cell_mask_kernel(const int64_t* __restrict__ idx, int64_t n, uint8_t* __restrict__ mask, int64_t V) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        int64_t j = idx[i];
        if (j >= 0 && j < V) mask[j] = 1;
    }
}
extern "C" int tdx_cell_mask(const int64_t* cell_idx, int64_t n_cells, uint8_t* mask, int64_t V, void* stream) {
    TDX_CHECK_ARG(mask && V > 0 && n_cells >= 0);
    int e = tdx_zero_async(mask, (size_t)V, as_stream(stream));
    if (e != TDX_OK) return e;
    if (n_cells > 0) {
        TDX_CHECK_ARG(cell_idx);
        hipLaunchKernelGGL(cell_mask_kernel, dim3(ceil_div(n_cells, 256)), dim3(256), 0, as_stream(stream), cell_idx,
                           n_cells, mask, V);
    }
    return tdx_launch_status();
}

// ------------------------------------------------------------------ q_sample -------------
// One block row per (b, f) plane so the per-sample coefficients are block-uniform scalars.
// 4 elements per lane (16 B) when V % 4 == 0.
__global__ void __launch_bounds__(256) q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                       const float* __restrict__ sa, const float* __restrict__ sb,
                                                       const int64_t* __restrict__ t, int t_stride,
                                                       const uint8_t* __restrict__ mask, int keep_bcs,
                                                       float* __restrict__ out, int F, int64_t V) {
    const int plane = blockIdx.y;  // b * F + f
    const int b = plane / F;
    const int64_t tt = t[(int64_t)b * t_stride];
    const float a = sa[tt], s = sb[tt];
    const int64_t base = (int64_t)plane * V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if ((V & 3) == 0) {
        const int64_t n4 = V >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x0 + base);
        const float4* z4 = reinterpret_cast<const float4*>(noise + base);
        float4* o4 = reinterpret_cast<float4*>(out + base);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            float4 xv = x4[i], zv = z4[i], r;
            r.x = a * xv.x + s * zv.x; r.y = a * xv.y + s * zv.y;
            r.z = a * xv.z + s * zv.z; r.w = a * xv.w + s * zv.w;
            if (keep_bcs) {
                uchar4 m = reinterpret_cast<const uchar4*>(mask)[i];
                if (!m.x) r.x = xv.x; if (!m.y) r.y = xv.y; if (!m.z) r.z = xv.z; if (!m.w) r.w = xv.w;
            }
            o4[i] = r;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
            float xv = x0[base + i];
            float r = a * xv + s * noise[base + i];
            if (keep_bcs && !mask[i]) r = xv;
            out[base + i] = r;
        }
    }
}

extern "C" int tdx_q_sample(const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac,
                            const int64_t* t, int t_stride, const uint8_t* mask, int keep_bcs, float* out, int B, int F,
                            int64_t V, void* stream) {
    TDX_CHECK_ARG(x0 && noise && sqrt_ac && sqrt_1mac && t && out && B > 0 && F > 0 && V > 0);
    TDX_CHECK_ARG(!keep_bcs || mask);
    dim3 grid((unsigned)min((int64_t)256, (V / 4 + 255) / 256 + 1), B * F);
    hipLaunchKernelGGL(q_sample_kernel, grid, dim3(256), 0, as_stream(stream), x0, noise, sqrt_ac, sqrt_1mac, t,
                       t_stride, mask, keep_bcs, out, F, V);
    return tdx_launch_status();
}

// ------------------------------------------------------------------ masked loss ----------
// pass 1: per-block partial sums in double -> atomicAdd(double) into workspace[0]
// pass 2: scale -> loss.   grad written in pass 1.

// The tail of the loss kernels: N per-thread sums -> wave sums -> block sums through LDS -> thread k adds sum k to acc[k].
// quant != 0 (TDX_DETERMINISTIC) puts the block sums on a grid where f64 additions are exact, hence order-independent
// (see gn_stats_launch).
template <int N>
__device__ __forceinline__ void block_sum_atomic(double* __restrict__ acc, const double (&sums)[N], double quant) {
    __shared__ double part[N][4];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double ws = wave_sum(sums[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = ws;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (quant != 0.0) t = rint(t * quant) / quant;
        atomicAdd(acc + threadIdx.x, t);
    }
}
// one in-domain element of the simple loss, d = eps_hat - noise: the gradient of gscale * term.  Both masked-loss kernels
// and elbo_elem take it from here, so their gradients agree bit for bit.
__device__ __forceinline__ float simple_loss_grad(float d, int l1, float gscale) {
    if (l1) return (d > 0.f) ? gscale : ((d < 0.f) ? -gscale : 0.f);
    return 2.0f * d * gscale;
}
// the same, and adds the element's term to the float sum of the masked-loss kernels
__device__ __forceinline__ float simple_loss_elem(float d, int l1, float gscale, float* sum) {
    if (l1) *sum += fabsf(d);
    else *sum += d * d;
    return simple_loss_grad(d, l1, gscale);
}

__global__ void __launch_bounds__(256)
masked_loss_kernel(const float* __restrict__ e, const float* __restrict__ n, const uint8_t* __restrict__ mask, int l1,
                   double* __restrict__ acc, float* __restrict__ grad, float gscale, int64_t V,
                   const int64_t* __restrict__ n_cells_dev, double samples, double quant) {
    if (n_cells_dev) gscale = (float)(1.0 / (samples * (double)*n_cells_dev));
    const int64_t base = (int64_t)blockIdx.y * V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
        const float d = e[base + i] - n[base + i];
        float g = 0.f;
        if (mask[i] != 0) g = simple_loss_elem(d, l1, gscale, &s);
        if (grad) grad[base + i] = g;
    }
    block_sum_atomic<1>(acc, {(double)s}, quant);
}
// the same pass with 16-B accesses, two independent trips in flight per thread (V % 4 == 0: every sample and feature
// plane starts on a 16-B boundary).  The scalar kernel above walks 36 dependent-free but ROLLED trips of 4-B loads per
// thread at 192 x 64 x 48: 67 us for 170 MB (profiles/r11_batch_scaling.txt); this one streams.
__global__ void __launch_bounds__(256)
masked_loss_vec_kernel(const float* __restrict__ e, const float* __restrict__ n, const uint8_t* __restrict__ mask, int l1,
                       double* __restrict__ acc, float* __restrict__ grad, float gscale, int64_t V,
                       const int64_t* __restrict__ n_cells_dev, double samples, double quant) {
    if (n_cells_dev) gscale = (float)(1.0 / (samples * (double)*n_cells_dev));
    const int64_t base = (int64_t)blockIdx.y * V;
    const int64_t V4 = V >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    float s = 0.f;
    auto one = [&](const float4& a, const float4& b, unsigned m, int64_t i) {
        const float d[4] = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[k] = 0.f;
            if ((m >> (8 * k)) & 0xffu) g[k] = simple_loss_elem(d[k], l1, gscale, &s);
        }
        if (grad) *reinterpret_cast<float4*>(grad + base + 4 * i) = make_float4(g[0], g[1], g[2], g[3]);
    };
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + stride < V4; i += 2 * stride) {
        const float4 a0 = *reinterpret_cast<const float4*>(e + base + 4 * i), b0 = *reinterpret_cast<const float4*>(n + base + 4 * i);
        const float4 a1 = *reinterpret_cast<const float4*>(e + base + 4 * (i + stride)), b1 = *reinterpret_cast<const float4*>(n + base + 4 * (i + stride));
        const unsigned m0 = *reinterpret_cast<const unsigned*>(mask + 4 * i), m1 = *reinterpret_cast<const unsigned*>(mask + 4 * (i + stride));
        one(a0, b0, m0, i);
        one(a1, b1, m1, i + stride);
    }
    for (; i < V4; i += stride)
        one(*reinterpret_cast<const float4*>(e + base + 4 * i), *reinterpret_cast<const float4*>(n + base + 4 * i),
            *reinterpret_cast<const unsigned*>(mask + 4 * i), i);
    block_sum_atomic<1>(acc, {(double)s}, quant);
}
__global__ void masked_loss_finish(const double* acc, float* loss, double inv, const int64_t* n_cells_dev, double samples) {
    if (n_cells_dev) inv = 1.0 / (samples * (double)*n_cells_dev);
    loss[0] = (float)(acc[0] * inv);
}

extern "C" size_t tdx_masked_loss_workspace_bytes(void) { return 16; }
static int masked_loss_launch(const float* eps_hat, const float* noise, const uint8_t* mask, int64_t n_cells,
                              const int64_t* n_cells_dev, int l1, float* loss, float* grad, int B, int F, int64_t V,
                              void* workspace, void* stream) {
    int err = tdx_zero_async(workspace, 16, as_stream(stream));
    if (err != TDX_OK) return err;
    const double samples = (double)B * F;
    const double inv = n_cells_dev ? 0.0 : 1.0 / (samples * (double)n_cells);
    const double quant = tdx_deterministic() ? 1048576.0 : 0.0;  // block partials on a 2^-20 grid: exact up to a total of 2^33
    const bool vec = (V % 4) == 0 && ((uintptr_t)eps_hat % 16) == 0 && ((uintptr_t)noise % 16) == 0 && ((uintptr_t)mask % 4) == 0 &&
                     (grad == nullptr || ((uintptr_t)grad % 16) == 0);
    if (vec) {
        dim3 grid((unsigned)min((int64_t)128, (V / 4 + 511) / 512), B * F);
        hipLaunchKernelGGL(masked_loss_vec_kernel, grid, dim3(256), 0, as_stream(stream), eps_hat, noise, mask, l1,
                           (double*)workspace, grad, (float)inv, V, n_cells_dev, samples, quant);
    } else {
        dim3 grid((unsigned)min((int64_t)64, (V + 255) / 256), B * F);
        hipLaunchKernelGGL(masked_loss_kernel, grid, dim3(256), 0, as_stream(stream), eps_hat, noise, mask, l1,
                           (double*)workspace, grad, (float)inv, V, n_cells_dev, samples, quant);
    }
    hipLaunchKernelGGL(masked_loss_finish, dim3(1), dim3(1), 0, as_stream(stream), (const double*)workspace, loss, inv,
                       n_cells_dev, samples);
    return tdx_launch_status();
}

extern "C" int tdx_masked_loss(const float* eps_hat, const float* noise, const uint8_t* mask, int64_t n_cells, int l1,
                               float* loss, float* grad, int B, int F, int64_t V, void* workspace, void* stream) {
    TDX_CHECK_ARG(eps_hat && noise && mask && loss && workspace && n_cells > 0 && B > 0 && F > 0 && V > 0);
    return masked_loss_launch(eps_hat, noise, mask, n_cells, nullptr, l1, loss, grad, B, F, V, workspace, stream);
}

// the same with the number of in-domain cells read from device memory at run time (int64 scalar): a captured training
// step (hipGraph) serves geometries with different cell counts through one graph
extern "C" int tdx_masked_loss_dyn(const float* eps_hat, const float* noise, const uint8_t* mask,
                                   const int64_t* n_cells_dev, int l1, float* loss, float* grad, int B, int F, int64_t V,
                                   void* workspace, void* stream) {
    TDX_CHECK_ARG(eps_hat && noise && mask && loss && workspace && n_cells_dev && B > 0 && F > 0 && V > 0);
    return masked_loss_launch(eps_hat, noise, mask, 0, n_cells_dev, l1, loss, grad, B, F, V, workspace, stream);
}

// ------------------------------------------------------------------ simple + ELBO loss (learned variances) ---
// The loss of the learned-variance model (ddpm.py:853-870) in one pass over out = [eps_hat | w] (B, 2F, V): the masked
// simple loss on eps_hat plus elbo_weight times the variational bound term -- KL(q(x_{t-1} | x_t, x_0) || p) for samples
// at t > 0, the negative log-likelihood (evaluated at x_t, as the reference does) for samples at t == 0 -- with
// log_var = lb + sigmoid(w) (plv - lb) per element, and its gradient with respect to all 2F planes.  One block row per
// (b, f) plane, so the sample's t and its table entries are block-uniform scalars.
struct ElboCoef {
    double recip, recipm1, c1, c2, lb, plv, dl, epl;  // dl = plv - lb, epl = exp(plv)
    bool first;                                       // t == 0: likelihood term
};
__device__ __forceinline__ ElboCoef elbo_coef(const float* __restrict__ sched, const float* __restrict__ plv, int T, int64_t t) {
    ElboCoef c;
    c.recip = sched[t]; c.recipm1 = sched[T + t]; c.c1 = sched[2 * T + t]; c.c2 = sched[3 * T + t];
    c.lb = sched[4 * T + t]; c.plv = plv[t]; c.dl = c.plv - c.lb; c.epl = exp(c.plv);
    c.first = (t == 0);
    return c;
}
// sigmoid of the variance weight for the reverse step (float; the loss below evaluates its own in double)
__device__ __forceinline__ float lv_sigmoid(float w) { return 1.0f / (1.0f + expf(-w)); }

// one in-domain element: adds its two loss terms to (simple, elbo) and returns the gradients of
// gscale * (simple + elbo_weight * elbo) with respect to eps_hat and w.
// The ELBO term is evaluated in DOUBLE from the float inputs.  Its summands reach |log_var| + (diff^2) exp(-log_var) --
// tens at t == 0, where exp(-log_var) ~ 1e3 -- while their mean is O(1) and the total subtracts it from the simple term:
// in float the per-element roundings of log_var alone (|log_var| 2^-24 ~ 4e-7) left the mean 2e-7 off and the total
// several ulps off where the two terms cancel.  Two double exponentials per element; the pass moves 28 B per element.
// The simple term's gradient is the one masked_loss_kernel writes (simple_loss_grad); its sum is kept in double here.
__device__ __forceinline__ void elbo_elem(const ElboCoef& c, float eps, float w, float noise, float xs, float xt, int l1,
                                          int clip, int detach_mean, float gscale, double escale, double& simple, double& elbo,
                                          float& g_eps, float& g_w) {
    const double dd = (double)eps - (double)noise;
    g_eps = simple_loss_grad(eps - noise, l1, gscale);
    if (l1) simple += fabs(dd);
    else simple += dd * dd;
    const double s = 1.0 / (1.0 + exp(-(double)w));
    const double lv = c.lb + s * c.dl;
    const double raw = c.recip * xt - c.recipm1 * eps;
    const double x0 = clip ? fmin(fmax(raw, -1.0), 1.0) : raw;
    const bool pass = (x0 == raw);  // torch.clamp: the gradient passes for -1 <= x0 <= 1
    // t > 0: true_mean - mean = c1 (x_start - x0), the c2 x_t of both means cancels; t == 0: x_t - mean
    const double diff = c.first ? xt - (c.c1 * x0 + c.c2 * xt) : c.c1 * (xs - x0);
    const double inv = exp(-lv);
    const double q = diff * diff * inv;
    const double a = c.first ? 0.0 : c.epl * inv;                       // exp(plv - log_var)
    const double cst = c.first ? 1.8378770664093453 : -c.plv - 1.0;     // log(2 pi)
    elbo += 0.5 * (lv + cst + a + q);
    g_w = (float)(escale * (0.5 * (1.0 - a - q)) * (c.dl * s * (1.0 - s)));
    // d term / d mean = -diff inv in both branches; d mean / d eps_hat = -c1 recipm1 where the clip left x0 alone
    if (!detach_mean && pass) g_eps = (float)((double)g_eps + escale * (diff * inv * (c.c1 * c.recipm1)));
}

template <bool VEC>
__global__ void __launch_bounds__(256)
elbo_loss_kernel(const float* __restrict__ out, const float* __restrict__ noise, const float* __restrict__ x_start,
                 const float* __restrict__ x_t, const uint8_t* __restrict__ mask, const int64_t* __restrict__ t,
                 const float* __restrict__ sched, const float* __restrict__ plv, int T, int l1, int clip, int detach_mean,
                 double elbo_weight, double* __restrict__ acc, float* __restrict__ grad, double inv_n, int F, int64_t V,
                 const int64_t* __restrict__ n_cells_dev, double samples, double quant) {
    if (n_cells_dev) inv_n = 1.0 / (samples * (double)*n_cells_dev);
    const float gscale = (float)inv_n;  // as masked_loss_kernel
    const double escale = elbo_weight * inv_n;
    const int plane = blockIdx.y, b = plane / F, f = plane - b * F;
    const ElboCoef c = elbo_coef(sched, plv, T, t[b]);
    const int64_t base = (int64_t)plane * V;                      // noise, x_start, x_t
    const int64_t ebase = ((int64_t)b * 2 * F + f) * V, wbase = ebase + (int64_t)F * V;  // out, grad
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double ssum = 0.0, esum = 0.0;
    if (VEC) {
        const int64_t V4 = V >> 2;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V4; i += stride) {
            const float4 e4 = *reinterpret_cast<const float4*>(out + ebase + 4 * i);
            const float4 w4 = *reinterpret_cast<const float4*>(out + wbase + 4 * i);
            const float4 n4 = *reinterpret_cast<const float4*>(noise + base + 4 * i);
            const float4 s4 = *reinterpret_cast<const float4*>(x_start + base + 4 * i);
            const float4 x4 = *reinterpret_cast<const float4*>(x_t + base + 4 * i);
            const unsigned m = *reinterpret_cast<const unsigned*>(mask + 4 * i);
            const float e[4] = {e4.x, e4.y, e4.z, e4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w}, n[4] = {n4.x, n4.y, n4.z, n4.w};
            const float xs[4] = {s4.x, s4.y, s4.z, s4.w}, xt[4] = {x4.x, x4.y, x4.z, x4.w};
            float ge[4] = {0.f, 0.f, 0.f, 0.f}, gw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((m >> (8 * k)) & 0xffu)
                    elbo_elem(c, e[k], w[k], n[k], xs[k], xt[k], l1, clip, detach_mean, gscale, escale, ssum, esum, ge[k], gw[k]);
            if (grad) {
                *reinterpret_cast<float4*>(grad + ebase + 4 * i) = make_float4(ge[0], ge[1], ge[2], ge[3]);
                *reinterpret_cast<float4*>(grad + wbase + 4 * i) = make_float4(gw[0], gw[1], gw[2], gw[3]);
            }
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
            float ge = 0.f, gw = 0.f;
            if (mask[i])
                elbo_elem(c, out[ebase + i], out[wbase + i], noise[base + i], x_start[base + i], x_t[base + i], l1, clip,
                          detach_mean, gscale, escale, ssum, esum, ge, gw);
            if (grad) { grad[ebase + i] = ge; grad[wbase + i] = gw; }
        }
    }
    block_sum_atomic<2>(acc, {ssum, esum}, quant);
}
// loss = {total, simple, elbo}: both terms are means over the same B F n_cells elements
__global__ void elbo_loss_finish(const double* acc, float* loss, double inv, const int64_t* n_cells_dev, double samples,
                                 double elbo_weight) {
    if (n_cells_dev) inv = 1.0 / (samples * (double)*n_cells_dev);
    const double simple = acc[0] * inv, elbo = acc[1] * inv;
    loss[0] = (float)(simple + elbo_weight * elbo);
    loss[1] = (float)simple;
    loss[2] = (float)elbo;
}

extern "C" size_t tdx_elbo_loss_workspace_bytes(void) { return 16; }
static int elbo_loss_launch(const float* out, const float* noise, const float* x_start, const float* x_t, const uint8_t* mask,
                            int64_t n_cells, const int64_t* n_cells_dev, const int64_t* t, const float* sched,
                            const float* plv, int T, int l1, int clip, int detach_mean, double elbo_weight, float* loss,
                            float* grad, int B, int F, int64_t V, void* workspace, void* stream) {
    int err = tdx_zero_async(workspace, 16, as_stream(stream));
    if (err != TDX_OK) return err;
    const double samples = (double)B * F;
    const double inv = n_cells_dev ? 0.0 : 1.0 / (samples * (double)n_cells);
    const double quant = tdx_deterministic() ? 1048576.0 : 0.0;  // block partials on a 2^-20 grid, as masked_loss_launch
    const bool vec = (V % 4) == 0 && (((uintptr_t)out | (uintptr_t)noise | (uintptr_t)x_start | (uintptr_t)x_t | (uintptr_t)grad) % 16) == 0 &&
                     ((uintptr_t)mask % 4) == 0;
    if (vec) {
        dim3 grid((unsigned)min((int64_t)128, (V / 4 + 255) / 256), B * F);
        hipLaunchKernelGGL(elbo_loss_kernel<true>, grid, dim3(256), 0, as_stream(stream), out, noise, x_start, x_t, mask, t,
                           sched, plv, T, l1, clip, detach_mean, elbo_weight, (double*)workspace, grad, inv, F, V,
                           n_cells_dev, samples, quant);
    } else {
        dim3 grid((unsigned)min((int64_t)64, (V + 255) / 256), B * F);
        hipLaunchKernelGGL(elbo_loss_kernel<false>, grid, dim3(256), 0, as_stream(stream), out, noise, x_start, x_t, mask, t,
                           sched, plv, T, l1, clip, detach_mean, elbo_weight, (double*)workspace, grad, inv, F, V,
                           n_cells_dev, samples, quant);
    }
    hipLaunchKernelGGL(elbo_loss_finish, dim3(1), dim3(1), 0, as_stream(stream), (const double*)workspace, loss, inv,
                       n_cells_dev, samples, elbo_weight);
    return tdx_launch_status();
}

extern "C" int tdx_elbo_loss(const float* out, const float* noise, const float* x_start, const float* x_t,
                             const uint8_t* mask, int64_t n_cells, const int64_t* t, const float* sched,
                             const float* posterior_log_var, int T, int l1, int clip, int detach_mean, double elbo_weight,
                             float* loss, float* grad, int B, int F, int64_t V, void* workspace, void* stream) {
    TDX_CHECK_ARG(out && noise && x_start && x_t && mask && t && sched && posterior_log_var && loss && workspace);
    TDX_CHECK_ARG(n_cells > 0 && T > 0 && B > 0 && F > 0 && V > 0);
    return elbo_loss_launch(out, noise, x_start, x_t, mask, n_cells, nullptr, t, sched, posterior_log_var, T, l1, clip,
                            detach_mean, elbo_weight, loss, grad, B, F, V, workspace, stream);
}
// n_cells read from device memory when the kernels run, as tdx_masked_loss_dyn: the captured training step
extern "C" int tdx_elbo_loss_dyn(const float* out, const float* noise, const float* x_start, const float* x_t,
                                 const uint8_t* mask, const int64_t* n_cells_dev, const int64_t* t, const float* sched,
                                 const float* posterior_log_var, int T, int l1, int clip, int detach_mean,
                                 double elbo_weight, float* loss, float* grad, int B, int F, int64_t V, void* workspace,
                                 void* stream) {
    TDX_CHECK_ARG(out && noise && x_start && x_t && mask && t && sched && posterior_log_var && loss && workspace);
    TDX_CHECK_ARG(n_cells_dev && T > 0 && B > 0 && F > 0 && V > 0);
    return elbo_loss_launch(out, noise, x_start, x_t, mask, 0, n_cells_dev, t, sched, posterior_log_var, T, l1, clip,
                            detach_mean, elbo_weight, loss, grad, B, F, V, workspace, stream);
}

// ------------------------------------------------------------------ Philox N(0,1) --------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// four N(0,1) draws of counter `ctr` in Philox stream `sid`: (0,1] uniforms from 32 bits each, two Box-Muller pairs
__device__ __forceinline__ void philox_normal4(uint64_t ctr, uint64_t sid, uint64_t seed, float (&r)[4]) {
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)sid, (uint32_t)(sid >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float u1 = ((float)c[2 * k] + 1.0f) * 2.3283064365386963e-10f;
        float u2 = (float)c[2 * k + 1] * 2.3283064365386963e-10f;
        float rad = sqrtf(-2.0f * __logf(u1));
        float sn, cs;
        __sincosf(6.283185307179586f * u2, &sn, &cs);
        r[2 * k] = rad * cs; r[2 * k + 1] = rad * sn;
    }
}

// n draws of stream `sid` from counter `off` on, four per counter, by the lanes of one grid row
__device__ __forceinline__ void philox_fill(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t sid, uint64_t off) {
    const int64_t n4 = (n + 3) >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float r[4];
        philox_normal4(off + (uint64_t)i, sid, seed, r);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * i + k < n) out[4 * i + k] = r[k];
    }
}
__global__ void __launch_bounds__(256) randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t sid,
                                                    const uint64_t* __restrict__ offp) {
    philox_fill(out, n, seed, sid, *offp);
}
__global__ void advance_offset(uint64_t* offp, uint64_t by) { *offp += by; }

__global__ void __launch_bounds__(256) randn_batched_kernel(float* __restrict__ out, int64_t n, uint64_t seed,
                                                            const uint64_t* __restrict__ sids,
                                                            const uint64_t* __restrict__ offp) {
    philox_fill(out + (int64_t)blockIdx.y * n, n, seed, sids[blockIdx.y], *offp);
}

extern "C" int tdx_randn_batched(float* out, int B, int64_t n, uint64_t seed, const uint64_t* stream_ids,
                                 uint64_t* offset_dev, void* stream) {
    TDX_CHECK_ARG(out && stream_ids && offset_dev && n > 0 && B > 0);
    const int64_t n4 = (n + 3) >> 2;
    dim3 grid((unsigned)min((int64_t)512, (n4 + 255) / 256), B);
    hipLaunchKernelGGL(randn_batched_kernel, grid, dim3(256), 0, as_stream(stream), out, n, seed, stream_ids, offset_dev);
    hipLaunchKernelGGL(advance_offset, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, (uint64_t)n4);
    return tdx_launch_status();
}

// ------------------------------------------------------------------ reverse step: five rules over two skeletons ----
// One launch takes the state from one timestep of its sequence to the one before.  A RULE says which tables a step reads
// and what it does to one element:
//   Coef          the step's coefficients (block-uniform scalars); `last` = the step that writes the mean and fixes the BC cells
//   valid(i)      is i a column of the tables?  A finished trajectory has none: the skeletons then write nothing
//   load(i)       column i
//   draws_z(c)    does the interior consume z at this step?
//   update(...)   one element; w, z, z2 and xb arrive as 0 where the step does not use them
//   eps_planes    1: eps is (B, F, V); 2: it is the decoder's [eps_hat | w], 2F planes per sample -- the LAYOUT
//   reads_w       w feeds the update (needs eps_planes == 2).  A rule with eps_planes == 2 and reads_w == false steps over the
//                 w half without loading it
// The two SKELETONS own everything else -- indexing, the mask, which operands are read, where the noise comes from -- so the
// tensor-noise and the in-kernel-noise entry of a rule agree bit for bit by construction of `update`: the DDIM and the
// learned-variance rule spell every multiply-add as an fmaf because, left to the compiler, the contraction of a * b + c * d
// came out differently in the scalar and in the 4-wide loop (1 ulp apart).

// ddpm.py:745-752 + 797-811: x0h from eps, the posterior mean, sigma = exp(log_betas[t] / 2) for the interior, BC cells
// re-noised at level t under noise_bcs.  sched = the 7 tables of include/tdx.h.  The two kernels this rule replaced wrote
// plain a * b - c * d and a * b + c * d; the fmafs below are the contractions the compiler chose for them (read off their
// ISA: the mean fuses c2 x_t, NOT c1 x0h as LvRule does), and tests/golden/reverse_step_bits.json pins the bits.  Left
// unspelled, the scalar skeleton contracted sa xb + sb z2 the other way round and came out 1 ulp off.  Fast exp for sigma.
struct AncestralRule {
    const float* sched;
    int T;
    static constexpr int eps_planes = 1;
    static constexpr bool reads_w = false;
    struct Coef {
        float recip, recipm1, c1, c2, sigma, sa, sb;
        bool last;
    };
    __device__ __forceinline__ bool valid(int64_t t) const { return t >= 0 && t < T; }
    __device__ __forceinline__ Coef load(int64_t t) const {
        Coef c;
        c.recip = sched[t]; c.recipm1 = sched[T + t]; c.c1 = sched[2 * T + t]; c.c2 = sched[3 * T + t];
        c.sigma = __expf(sched[4 * T + t] * 0.5f);
        c.sa = sched[5 * T + t]; c.sb = sched[6 * T + t];
        c.last = (t == 0);
        return c;
    }
    static __device__ __forceinline__ bool draws_z(const Coef& c) { return !c.last; }
    static __device__ __forceinline__ float update(const Coef& c, float xt, float eps, float, float z, float z2, float xb,
                                                   bool inside, int noise_bcs, int clip) {
        float x0h = fmaf(c.recip, xt, -(c.recipm1 * eps));
        if (!noise_bcs && !inside) x0h = xt;
        if (clip) x0h = fminf(fmaxf(x0h, -1.0f), 1.0f);
        float r = fmaf(c.c2, xt, c.c1 * x0h);
        if (c.last) {
            if (!inside) r = xb;
        } else if (inside) {
            r = fmaf(c.sigma, z, r);
        } else if (noise_bcs) {
            r = fmaf(c.sa, xb, c.sb * z2);
        }
        return r;
    }
};

// The ancestral step of the model that also predicts its variance (ddpm.py:732-741): the noise inside the domain is
// scaled per element by sigma = exp(log_var / 2), log_var = lb + sigmoid(w) (plv - lb), lb = log_betas[t], plv =
// posterior_log_var[t], instead of by exp(lb / 2).
struct LvRule {
    const float *sched, *plv;
    int T;
    static constexpr int eps_planes = 2;
    static constexpr bool reads_w = true;
    struct Coef {
        float recip, recipm1, c1, c2, lb, dl, sa, sb;  // dl = plv - lb
        bool last;
    };
    __device__ __forceinline__ bool valid(int64_t t) const { return t >= 0 && t < T; }
    __device__ __forceinline__ Coef load(int64_t t) const {
        Coef c;
        c.recip = sched[t]; c.recipm1 = sched[T + t]; c.c1 = sched[2 * T + t]; c.c2 = sched[3 * T + t];
        c.lb = sched[4 * T + t]; c.dl = plv[t] - c.lb;
        c.sa = sched[5 * T + t]; c.sb = sched[6 * T + t];
        c.last = (t == 0);
        return c;
    }
    static __device__ __forceinline__ bool draws_z(const Coef& c) { return !c.last; }
    static __device__ __forceinline__ float update(const Coef& c, float xt, float eps, float w, float z, float z2, float xb,
                                                   bool inside, int noise_bcs, int clip) {
        float x0 = fmaf(c.recip, xt, -(c.recipm1 * eps));
        if (!noise_bcs && !inside) x0 = xt;
        if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        float r = fmaf(c.c1, x0, c.c2 * xt);
        if (c.last) {
            if (!inside) r = xb;
        } else if (inside) {
            const float sigma = expf(0.5f * fmaf(lv_sigmoid(w), c.dl, c.lb));
            r = fmaf(sigma, z, r);
        } else if (noise_bcs) {
            r = fmaf(c.sa, xb, c.sb * z2);
        }
        return r;
    }
};

// Generalized DDIM update (Song et al. 2021, eq. 12) from tau_k to tau_{k-1}; tab = 6 rows of S floats (schedules.
// DDIM_PACKED_ORDER), column k.  x0 is formed as model_predictions forms it (BC cells keep x_t without noise_bcs, then the
// clip); where that changed it, eps is re-derived from it (predict_noise_from_start) so that x0 and the direction term
// describe the same point.  BC cells under noise_bcs are re-noised at the level of the state PRODUCED, tau_{k-1} (sp =
// sqrt(abar), sbp = sqrt(1 - abar) there): the ancestral loop re-noises them at level t for x_{t-1}, one level off, an
// offset a subsequence cannot keep.  Step k = 0 writes the mean and fixes the BC cells.  z is consumed only where
// sigma != 0 (eta = 0: the interior does not depend on the noise at all, not even through the sign of a zero); the Philox
// rounds for it are then skipped, the offset still advances as if they had been drawn.
struct DdimRule {
    const float* tab;
    int S;
    static constexpr int eps_planes = 1;
    static constexpr bool reads_w = false;
    struct Coef {
        float recip, recipm1, sp, dir, sigma, sbp;
        bool last;
    };
    __device__ __forceinline__ bool valid(int64_t k) const { return k >= 0 && k < S; }
    __device__ __forceinline__ Coef load(int64_t k) const {
        Coef c;
        c.recip = tab[k]; c.recipm1 = tab[S + k]; c.sp = tab[2 * S + k];
        c.dir = tab[3 * S + k]; c.sigma = tab[4 * S + k]; c.sbp = tab[5 * S + k];
        c.last = (k == 0);
        return c;
    }
    static __device__ __forceinline__ bool draws_z(const Coef& c) { return !c.last && c.sigma != 0.0f; }
    static __device__ __forceinline__ float update(const Coef& c, float xt, float eps, float, float z, float z2, float xb,
                                                   bool inside, int noise_bcs, int clip) {
        const float raw = fmaf(c.recip, xt, -(c.recipm1 * eps));
        float x0 = raw;
        if (!noise_bcs && !inside) x0 = xt;
        if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        const float e = (x0 == raw) ? eps : fmaf(c.recip, xt, -x0) / c.recipm1;
        float r = fmaf(c.sp, x0, c.dir * e);
        if (c.last) {
            if (!inside) r = xb;
        } else if (inside) {
            if (c.sigma != 0.0f) r = fmaf(c.sigma, z, r);
        } else if (noise_bcs) {
            r = fmaf(c.sp, xb, c.sbp * z2);
        }
        return r;
    }
};

// LvRule's step over an increasing subsequence tau[0..S-1] of the training timesteps, from tau[k] to tau[k-1]: the ancestral
// step of the SHORTER chain whose cumulative products are a = abar[tau[k]] (Nichol & Dhariwal 2021, the SpacedDiffusion
// construction).  tab = 8 rows of S floats (schedules.RESPACED_PACKED_ORDER), column k: the respaced beta' = 1 - a / p and
// beta~' = beta' (1 - p) / (1 - a) take the places of beta_t and the posterior variance.  The element is LvRule's own
// function, not a restatement: a table that holds the training chain's columns gives the training chain's bits.  BC cells
// under noise_bcs are re-noised at the level of the state PRODUCED (sa = sqrt(p), sb = sqrt(1 - p)), as DdimRule does.
struct LvRespacedRule {
    const float* tab;
    int S;
    static constexpr int eps_planes = 2;
    static constexpr bool reads_w = true;
    using Coef = LvRule::Coef;
    __device__ __forceinline__ bool valid(int64_t k) const { return k >= 0 && k < S; }
    __device__ __forceinline__ Coef load(int64_t k) const {
        Coef c;
        c.recip = tab[k]; c.recipm1 = tab[S + k]; c.c1 = tab[2 * S + k]; c.c2 = tab[3 * S + k];
        c.lb = tab[4 * S + k]; c.dl = tab[5 * S + k] - c.lb;
        c.sa = tab[6 * S + k]; c.sb = tab[7 * S + k];
        c.last = (k == 0);
        return c;
    }
    static __device__ __forceinline__ bool draws_z(const Coef& c) { return LvRule::draws_z(c); }
    static __device__ __forceinline__ float update(const Coef& c, float xt, float eps, float w, float z, float z2, float xb,
                                                   bool inside, int noise_bcs, int clip) {
        return LvRule::update(c, xt, eps, w, z, z2, xb, inside, noise_bcs, clip);
    }
};

// DdimRule on the eps_hat half of a learned-variance model's output: the same table, coefficients and update, eps_hat read
// at the 2F stride, w never loaded (the DDIM variance is the table's sigma).
struct DdimLvRule : DdimRule {
    static constexpr int eps_planes = 2;
};

// Skeleton 1: z and z2 are tensors.  One block row per (b, f) plane, one element per lane and trip.  A NULL noise tensor
// reads as "no noise" rather than being dereferenced (the host cannot see the step index); x_bcs, z, z2 and w are read
// only where the step uses them.
template <typename Rule>
__global__ void __launch_bounds__(256)
reverse_step_kernel(Rule rule, const float* __restrict__ x_t, const float* __restrict__ eps, const float* __restrict__ z,
                    const float* __restrict__ z2, const float* __restrict__ x_bcs, const uint8_t* __restrict__ mask,
                    const int64_t* __restrict__ ip, int noise_bcs, int clip, float* __restrict__ out, int F, int64_t V) {
    const int64_t idx = *ip;
    if (!rule.valid(idx)) return;  // a finished trajectory: no column to read
    const typename Rule::Coef c = rule.load(idx);
    const bool use_z = Rule::draws_z(c) && z, use_z2 = !c.last && noise_bcs && z2, use_xb = c.last || noise_bcs;
    const int plane = blockIdx.y;
    const int64_t base = (int64_t)plane * V;
    int64_t ebase = base, wbase = 0;
    if (Rule::eps_planes == 2) {  // sample b: F planes of eps_hat, then F of w
        const int b = plane / F, f = plane - b * F;
        ebase = ((int64_t)b * 2 * F + f) * V;
        wbase = ebase + (int64_t)F * V;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
        const bool inside = mask[i] != 0;
        const bool noisy = use_z && inside;
        const float zz = noisy ? z[base + i] : 0.f, ww = (Rule::reads_w && noisy) ? eps[wbase + i] : 0.f;
        const float zb = (use_z2 && !inside) ? z2[base + i] : 0.f;
        const float xb = (use_xb && !inside) ? x_bcs[base + i] : 0.f;
        out[base + i] = Rule::update(c, x_t[base + i], eps[ebase + i], ww, zz, zb, xb, inside, noise_bcs, clip);
    }
}

// Skeleton 2: z and z2 are generated where they are consumed.  One block row per sample, four elements per lane and trip:
// lane i of sample b draws the four normals randn_batched_kernel would have written to z[b][4i..4i+3] (counter off + i)
// and to z2 (counter off + n4 + i, n4 = F V / 4 over the F planes of the STATE), so a run is bit-identical to
// tdx_randn_batched(z); [tdx_randn_batched(z2);] <the rule's tensor-noise entry>.  Saves two 4-byte writes and two reads
// per value; the Philox rounds are a few microseconds of VALU per launch, and are skipped for a quad that has no use for them.
template <typename Rule>
__global__ void __launch_bounds__(256)
reverse_step_rng_kernel(Rule rule, const float* __restrict__ x_t, const float* __restrict__ eps,
                        const float* __restrict__ x_bcs, const uint8_t* __restrict__ mask, const int64_t* __restrict__ ip,
                        int noise_bcs, int clip, float* __restrict__ out, int64_t V, int64_t n4, uint64_t seed,
                        const uint64_t* __restrict__ sids, const uint64_t* __restrict__ offp) {
    const int64_t idx = *ip;
    if (!rule.valid(idx)) return;  // a finished trajectory: no column to read
    const uint64_t off = *offp, sid = sids[blockIdx.y];
    const typename Rule::Coef c = rule.load(idx);
    const bool use_z = Rule::draws_z(c), use_z2 = !c.last && noise_bcs, use_xb = c.last || noise_bcs;
    const int64_t base4 = (int64_t)blockIdx.y * n4;
    const int64_t v4 = V >> 2;
    const float4* xt4 = reinterpret_cast<const float4*>(x_t) + base4;
    const float4* e4 = reinterpret_cast<const float4*>(eps) + Rule::eps_planes * base4;
    const float4* w4 = e4 + n4;  // eps_planes == 2: sample b holds F planes of eps_hat, then F of w
    const float4* xb4 = reinterpret_cast<const float4*>(x_bcs) + base4;
    const uchar4* m4 = reinterpret_cast<const uchar4*>(mask);
    float4* o4 = reinterpret_cast<float4*>(out) + base4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 xv = xt4[i], ev = e4[i];
        const uchar4 mv = m4[i % v4];
        const bool in[4] = {mv.x != 0, mv.y != 0, mv.z != 0, mv.w != 0};
        const bool any_in = in[0] | in[1] | in[2] | in[3], any_out = !(in[0] & in[1] & in[2] & in[3]);
        const float xt[4] = {xv.x, xv.y, xv.z, xv.w}, ee[4] = {ev.x, ev.y, ev.z, ev.w};
        float xb[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
        if (use_xb && any_out) {
            const float4 bv = xb4[i];
            xb[0] = bv.x; xb[1] = bv.y; xb[2] = bv.z; xb[3] = bv.w;
        }
        if (use_z && any_in) {
            if (Rule::reads_w) {
                const float4 wv = w4[i];
                w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
            }
            philox_normal4(off + (uint64_t)i, sid, seed, z);
        }
        if (use_z2 && any_out) philox_normal4(off + (uint64_t)n4 + (uint64_t)i, sid, seed, z2);
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = Rule::update(c, xt[k], ee[k], w[k], z[k], z2[k], xb[k], in[k], noise_bcs, clip);
        o4[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
}
// Skeleton 2 for DdimRule, written out as it stood before the skeletons: reverse_step_rng_kernel<DdimRule> averaged 56.6 us
// at 8 x 4 x 192 x 64 x 48 against 55.6 / 56.2 us for this form, 0.15 us over what the comparison allows
// (profiles/r19_reverse_step_rules.txt, item 6).  Same loop without the w plane; coefficients and update are the rule's.
__global__ void __launch_bounds__(256)
ddim_step_rng_kernel(const float* __restrict__ x_t, const float* __restrict__ eps, const float* __restrict__ x_bcs,
                     const uint8_t* __restrict__ mask, const float* __restrict__ tab, int S,
                     const int64_t* __restrict__ kp, int noise_bcs, int clip, float* __restrict__ out, int64_t V,
                     int64_t n4, uint64_t seed, const uint64_t* __restrict__ sids, const uint64_t* __restrict__ offp) {
    const int64_t k = *kp;
    const DdimRule rule{tab, S};
    if (!rule.valid(k)) return;  // a finished trajectory: no column to read
    const uint64_t off = *offp, sid = sids[blockIdx.y];
    const DdimRule::Coef c = rule.load(k);
    const bool use_z = DdimRule::draws_z(c), use_z2 = !c.last && noise_bcs;
    const int64_t base4 = (int64_t)blockIdx.y * n4;
    const int64_t v4 = V >> 2;
    const float4* xt4 = reinterpret_cast<const float4*>(x_t) + base4;
    const float4* e4 = reinterpret_cast<const float4*>(eps) + base4;
    const float4* xb4 = reinterpret_cast<const float4*>(x_bcs) + base4;
    const uchar4* m4 = reinterpret_cast<const uchar4*>(mask);
    float4* o4 = reinterpret_cast<float4*>(out) + base4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 xv = xt4[i], ev = e4[i];
        const uchar4 mv = m4[i % v4];
        const bool in[4] = {mv.x != 0, mv.y != 0, mv.z != 0, mv.w != 0};
        const bool any_in = in[0] | in[1] | in[2] | in[3], any_out = !(in[0] & in[1] & in[2] & in[3]);
        const float xt[4] = {xv.x, xv.y, xv.z, xv.w}, ee[4] = {ev.x, ev.y, ev.z, ev.w};
        float xb[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f};
        if (any_out && (c.last || noise_bcs)) {
            const float4 bv = xb4[i];
            xb[0] = bv.x; xb[1] = bv.y; xb[2] = bv.z; xb[3] = bv.w;
        }
        if (use_z && any_in) philox_normal4(off + (uint64_t)i, sid, seed, z);
        if (use_z2 && any_out) philox_normal4(off + (uint64_t)n4 + (uint64_t)i, sid, seed, z2);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = DdimRule::update(c, xt[j], ee[j], 0.f, z[j], z2[j], xb[j], in[j], noise_bcs, clip);
        o4[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
}
// offset += by; t -= 1: the two scalar updates that close a reverse step, in one launch
__global__ void advance_step(uint64_t* offp, uint64_t by, int64_t* tp) { *offp += by; *tp -= 1; }
// offset += by; k -= 1; t = tau[k] while a step is left: the scalar updates that close a DDIM step, in one launch
__global__ void advance_ddim_step(uint64_t* offp, uint64_t by, int64_t* kp, const int64_t* __restrict__ tau, int S,
                                  int64_t* tp) {
    *offp += by;
    const int64_t k = *kp - 1;
    *kp = k;
    if (k >= 0 && k < S) *tp = tau[k];
}

// the launch of each skeleton: the checks every rule shares, and the grid.  `idx` is the rule's device-side step index.
template <typename Rule>
static int reverse_step_launch(const Rule& rule, const float* x_t, const float* eps, const float* z, const float* z2,
                               const float* x_bcs, const uint8_t* mask, const int64_t* idx, int noise_bcs, int clip,
                               float* out, int B, int F, int64_t V, void* stream) {
    TDX_CHECK_ARG(x_t && eps && x_bcs && mask && idx && out && B > 0 && F > 0 && V > 0);
    dim3 grid((unsigned)min((int64_t)128, (V + 255) / 256), B * F);
    hipLaunchKernelGGL((reverse_step_kernel<Rule>), grid, dim3(256), 0, as_stream(stream), rule, x_t, eps, z, z2, x_bcs, mask,
                       idx, noise_bcs, clip, out, F, V);
    return tdx_launch_status();
}
// ... then `advance(by)` launches the rule's scalar updates, by = the counters the step has consumed
template <typename Rule, typename Advance>
static int reverse_step_rng_launch(const Rule& rule, const float* x_t, const float* eps, const float* x_bcs,
                                   const uint8_t* mask, const int64_t* idx, int noise_bcs, int clip, float* out, int B, int F,
                                   int64_t V, uint64_t seed, const uint64_t* stream_ids, const uint64_t* offset_dev,
                                   void* stream, Advance advance) {
    TDX_CHECK_ARG(x_t && eps && x_bcs && mask && idx && out && stream_ids && offset_dev);
    TDX_CHECK_ARG(B > 0 && F > 0 && V > 0 && (V & 3) == 0);
    TDX_CHECK_ARG(((uintptr_t)x_t | (uintptr_t)eps | (uintptr_t)x_bcs | (uintptr_t)out) % 16 == 0 && (uintptr_t)mask % 4 == 0);
    const int64_t n4 = (int64_t)F * V / 4;
    dim3 grid((unsigned)min((int64_t)256, (n4 + 255) / 256), B);
    if constexpr (std::is_same_v<Rule, DdimRule>)  // written out, see ddim_step_rng_kernel
        hipLaunchKernelGGL(ddim_step_rng_kernel, grid, dim3(256), 0, as_stream(stream), x_t, eps, x_bcs, mask, rule.tab, rule.S,
                           idx, noise_bcs, clip, out, V, n4, seed, stream_ids, offset_dev);
    else
        hipLaunchKernelGGL((reverse_step_rng_kernel<Rule>), grid, dim3(256), 0, as_stream(stream), rule, x_t, eps, x_bcs, mask,
                           idx, noise_bcs, clip, out, V, n4, seed, stream_ids, offset_dev);
    advance((uint64_t)(noise_bcs ? 2 * n4 : n4));
    return tdx_launch_status();
}

extern "C" int tdx_p_sample_step(const float* x_t, const float* eps, const float* z, const float* z2,
                                 const float* x_bcs, const uint8_t* mask, const float* sched, int T, const int64_t* t,
                                 int noise_bcs, int clip, float* out, int B, int F, int64_t V, void* stream) {
    TDX_CHECK_ARG(sched && T > 0);
    return reverse_step_launch(AncestralRule{sched, T}, x_t, eps, z, z2, x_bcs, mask, t, noise_bcs, clip, out, B, F, V, stream);
}
extern "C" int tdx_p_sample_step_rng(const float* x_t, const float* eps, const float* x_bcs, const uint8_t* mask,
                                     const float* sched, int T, int64_t* t, int noise_bcs, int clip, float* out, int B,
                                     int F, int64_t V, uint64_t seed, const uint64_t* stream_ids, uint64_t* offset_dev,
                                     void* stream) {
    TDX_CHECK_ARG(sched && T > 0);
    return reverse_step_rng_launch(AncestralRule{sched, T}, x_t, eps, x_bcs, mask, t, noise_bcs, clip, out, B, F, V, seed,
                                   stream_ids, offset_dev, stream, [&](uint64_t by) {
        hipLaunchKernelGGL(advance_step, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, by, t);
    });
}

extern "C" int tdx_p_sample_step_lv(const float* x_t, const float* model_out, const float* z, const float* z2,
                                    const float* x_bcs, const uint8_t* mask, const float* sched,
                                    const float* posterior_log_var, int T, const int64_t* t, int noise_bcs, int clip,
                                    float* out, int B, int F, int64_t V, void* stream) {
    TDX_CHECK_ARG(sched && posterior_log_var && T > 0);
    return reverse_step_launch(LvRule{sched, posterior_log_var, T}, x_t, model_out, z, z2, x_bcs, mask, t, noise_bcs, clip,
                               out, B, F, V, stream);
}
extern "C" int tdx_p_sample_step_lv_rng(const float* x_t, const float* model_out, const float* x_bcs, const uint8_t* mask,
                                        const float* sched, const float* posterior_log_var, int T, int64_t* t,
                                        int noise_bcs, int clip, float* out, int B, int F, int64_t V, uint64_t seed,
                                        const uint64_t* stream_ids, uint64_t* offset_dev, void* stream) {
    TDX_CHECK_ARG(sched && posterior_log_var && T > 0);
    return reverse_step_rng_launch(LvRule{sched, posterior_log_var, T}, x_t, model_out, x_bcs, mask, t, noise_bcs, clip, out,
                                   B, F, V, seed, stream_ids, offset_dev, stream, [&](uint64_t by) {
        hipLaunchKernelGGL(advance_step, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, by, t);
    });
}

extern "C" int tdx_ddim_step(const float* x_t, const float* eps, const float* z, const float* z2, const float* x_bcs,
                             const uint8_t* mask, const float* tab, int S, const int64_t* k, const int64_t* tau,
                             const int64_t* t, int noise_bcs, int clip, float* out, int B, int F, int64_t V,
                             void* stream) {
    TDX_CHECK_ARG(tab && S > 0 && tau && t);
    return reverse_step_launch(DdimRule{tab, S}, x_t, eps, z, z2, x_bcs, mask, k, noise_bcs, clip, out, B, F, V, stream);
}
extern "C" int tdx_ddim_step_rng(const float* x_t, const float* eps, const float* x_bcs, const uint8_t* mask,
                                 const float* tab, int S, int64_t* k, const int64_t* tau, int64_t* t, int noise_bcs,
                                 int clip, float* out, int B, int F, int64_t V, uint64_t seed,
                                 const uint64_t* stream_ids, uint64_t* offset_dev, void* stream) {
    TDX_CHECK_ARG(tab && S > 0 && tau && t);
    return reverse_step_rng_launch(DdimRule{tab, S}, x_t, eps, x_bcs, mask, k, noise_bcs, clip, out, B, F, V, seed, stream_ids,
                                   offset_dev, stream, [&](uint64_t by) {
        hipLaunchKernelGGL(advance_ddim_step, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, by, k, tau, S, t);
    });
}

extern "C" int tdx_p_sample_step_lv_respaced(const float* x_t, const float* model_out, const float* z, const float* z2,
                                             const float* x_bcs, const uint8_t* mask, const float* tab, int S,
                                             const int64_t* k, const int64_t* tau, const int64_t* t, int noise_bcs, int clip,
                                             float* out, int B, int F, int64_t V, void* stream) {
    TDX_CHECK_ARG(tab && S > 0 && tau && t);
    return reverse_step_launch(LvRespacedRule{tab, S}, x_t, model_out, z, z2, x_bcs, mask, k, noise_bcs, clip, out, B, F, V,
                               stream);
}
extern "C" int tdx_p_sample_step_lv_respaced_rng(const float* x_t, const float* model_out, const float* x_bcs,
                                                 const uint8_t* mask, const float* tab, int S, int64_t* k, const int64_t* tau,
                                                 int64_t* t, int noise_bcs, int clip, float* out, int B, int F, int64_t V,
                                                 uint64_t seed, const uint64_t* stream_ids, uint64_t* offset_dev,
                                                 void* stream) {
    TDX_CHECK_ARG(tab && S > 0 && tau && t);
    return reverse_step_rng_launch(LvRespacedRule{tab, S}, x_t, model_out, x_bcs, mask, k, noise_bcs, clip, out, B, F, V, seed,
                                   stream_ids, offset_dev, stream, [&](uint64_t by) {
        hipLaunchKernelGGL(advance_ddim_step, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, by, k, tau, S, t);
    });
}

extern "C" int tdx_ddim_step_lv(const float* x_t, const float* model_out, const float* z, const float* z2, const float* x_bcs,
                                const uint8_t* mask, const float* tab, int S, const int64_t* k, const int64_t* tau,
                                const int64_t* t, int noise_bcs, int clip, float* out, int B, int F, int64_t V, void* stream) {
    TDX_CHECK_ARG(tab && S > 0 && tau && t);
    return reverse_step_launch(DdimLvRule{{tab, S}}, x_t, model_out, z, z2, x_bcs, mask, k, noise_bcs, clip, out, B, F, V,
                               stream);
}
extern "C" int tdx_ddim_step_lv_rng(const float* x_t, const float* model_out, const float* x_bcs, const uint8_t* mask,
                                    const float* tab, int S, int64_t* k, const int64_t* tau, int64_t* t, int noise_bcs,
                                    int clip, float* out, int B, int F, int64_t V, uint64_t seed, const uint64_t* stream_ids,
                                    uint64_t* offset_dev, void* stream) {
    TDX_CHECK_ARG(tab && S > 0 && tau && t);
    return reverse_step_rng_launch(DdimLvRule{{tab, S}}, x_t, model_out, x_bcs, mask, k, noise_bcs, clip, out, B, F, V, seed,
                                   stream_ids, offset_dev, stream, [&](uint64_t by) {
        hipLaunchKernelGGL(advance_ddim_step, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, by, k, tau, S, t);
    });
}

extern "C" int tdx_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, uint64_t* offset_dev, void* stream) {
    TDX_CHECK_ARG(out && offset_dev && n > 0);
    const int64_t n4 = (n + 3) >> 2;
    int grid = (int)min((int64_t)2048, (n4 + 255) / 256);
    hipLaunchKernelGGL(randn_kernel, dim3(grid), dim3(256), 0, as_stream(stream), out, n, seed, stream_id, offset_dev);
    hipLaunchKernelGGL(advance_offset, dim3(1), dim3(1), 0, as_stream(stream), offset_dev, (uint64_t)n4);
    return tdx_launch_status();
}


// ------------------------------------------------------------------ host signal ----------
// One lane stores gen * TDX_SIGNAL_STRIDE + k into a word of HOST memory (pinned, device-mapped) with a system-scope release:
// everything enqueued before it on the stream -- the staging kernels of a gradient bucket inside a captured backward pass --
// has completed and is visible.  This runtime refuses event-record nodes inside a captured graph
// (hipEventRecordWithFlags(..., hipEventRecordExternal) -> hipErrorInvalidValue; torch: "External events are disallowed in
// rocm", tools/micro/external_event_probe.py), so a graph-external stream cannot wait on a point INSIDE a graph; the host
// can: it polls this word and launches the bucket's all-reduce on its communication stream while the rest of the graph runs.
__global__ void signal_host_kernel(uint32_t* __restrict__ flag, const uint32_t* __restrict__ gen, uint32_t k) {
    __hip_atomic_store(flag, gen[0] * (uint32_t)TDX_SIGNAL_STRIDE + k, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
extern "C" int tdx_signal_host(uint32_t* host_flag, const uint32_t* gen_dev, uint32_t k, void* stream) {
    TDX_CHECK_ARG(host_flag && gen_dev && k < (uint32_t)TDX_SIGNAL_STRIDE);
    hipLaunchKernelGGL(signal_host_kernel, dim3(1), dim3(1), 0, as_stream(stream), host_flag, gen_dev, k);
    return tdx_launch_status();
}
