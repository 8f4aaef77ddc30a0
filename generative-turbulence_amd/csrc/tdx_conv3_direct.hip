// 3x3x3 convolution on NDHWC activations: weight packing and unpacking, and the vector-ALU implicit-GEMM kernels (any
// dtype, exact f32 accumulation -- the f32 parity path and the cross-check for the MFMA kernels) with the halo fold of
// their data gradient.  The entry points and the choice between these kernels and the MFMA families: tdx_conv3_entry.hip.
//
// Geometry shared by all implementations: an "output grid" (Xo,Yo,Zo) is produced from an
// "input grid" (Xi,Yi,Zi); output voxel o reads input voxel o + off + e for the 27 taps
// e in {-1,0,1}^3, either clamped to the grid (replicate padding, forward: off = 0, grids
// equal) or treated as zero outside (data gradient: the adjoint is evaluated on the padded
// grid Xi+2 with off = -1 and the halo is folded back onto the boundary afterwards).
#include "tdx_common.h"
#include "tdx_conv3.h"
#include <stdlib.h>

// ------------------------------------------------------------------ weight packing -------
// element index of operand (tap, k, n) for a conv with K input / N output channels
__host__ __device__ __forceinline__ int64_t wp_index(int kc, int tap, int k, int n, int K, int N) {
    return kc ? ((((int64_t)(k / kc) * 27 + tap) * N + n) * kc + (k % kc)) : (((int64_t)tap * K + k) * N + n);
}

// w (Cout, Cin, 27) f32 -> wf: forward operand (K = Cin, N = Cout);
//                           wb: data-gradient operand (K = Cout, N = Cin, taps flipped)
template <typename T>
__global__ void conv3_pack_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wb, int Cin,
                                  int Cout, int lf, int lb) {
    const int64_t n = (int64_t)Cout * Cin * 27;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 27);
        const int64_t r = i / 27;
        const int ci = (int)(r % Cin), co = (int)(r / Cin);
        const float v = w[i];
        if (wf) stf(wf + wp_index(lf, tap, ci, co, Cin, Cout), v);
        if (wb) stf(wb + wp_index(lb, 26 - tap, co, ci, Cout, Cin), v);
    }
}
// Tiled pack for the case that both operands use the MFMA layout: a workgroup owns a 16 (co) x 16 (ci) tile, reads
// its 16 runs of 16*27 contiguous floats, and writes, per tap, one 512-B run of wf ([ci/16][tap][co][16 ci]) and one
// of wb ([co/16][26-tap][ci][16 co]); per tap 16 rows x 2 halves of 8 packed values (one 16-B store each): 32 threads
// per tap, 8 taps per pass.  FMT = PACK_SPLIT: fp32 tensors' split-precision operands, a hi and a lo image (hi = bf16(v),
// lo = bf16(v - hi)) 27 Cin Cout elements apart; PACK_F16: the bf16 layout with IEEE half elements.
#define PACK_BF16 0
#define PACK_SPLIT 1
#define PACK_F16 2
template <int FMT>
__device__ __forceinline__ void conv3_pack_tile(const float* __restrict__ w, bf16* __restrict__ wf, bf16* __restrict__ wb,
                                                int Cin, int Cout, int ci0, int co0, float (*t)[16 * 27 + 1]) {
    constexpr bool SPLIT = FMT == PACK_SPLIT;
    typedef H16<FMT == PACK_F16> H;
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)Cout * Cin * 27;
    for (int i = tid; i < 16 * 432; i += 256) {
        const int co = i / 432, r = i - co * 432;
        t[co][r] = w[((int64_t)(co0 + co) * Cin + ci0) * 27 + r];
    }
    __syncthreads();
    const int row = (tid >> 1) & 15, half = tid & 1, tsub = tid >> 5;
    auto put = [&](bf16* dst, int64_t j, const float* v) {
        unsigned h[4], l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            h[q] = H::pack2(v[2 * q], v[2 * q + 1]);
            if (SPLIT)
                l[q] = pack_bf16x2(v[2 * q] - __uint_as_float(h[q] << 16), v[2 * q + 1] - __uint_as_float(h[q] & 0xffff0000u));
        }
        *reinterpret_cast<uint4*>(dst + j) = make_uint4(h[0], h[1], h[2], h[3]);
        if (SPLIT) *reinterpret_cast<uint4*>(dst + n + j) = make_uint4(l[0], l[1], l[2], l[3]);
    };
    for (int tap = tsub; tap < 27; tap += 8) {
        float v[8];
        if (wf) {  // row = co, k = ci
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = t[row][(half * 8 + q) * 27 + tap];
            // bf16: [ci/16][tap][co][16 ci]; split images: [ci/8][tap][co][8 ci] (8-channel slices are what their kernels stage)
            put(wf, SPLIT ? (((int64_t)((ci0 >> 3) + half) * 27 + tap) * Cout + co0 + row) << 3
                          : ((((int64_t)(ci0 >> 4) * 27 + tap) * Cout + co0 + row) << 4) + half * 8, v);
        }
        if (wb) {  // row = ci, k = co
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = t[half * 8 + q][row * 27 + tap];
            put(wb, SPLIT ? (((int64_t)((co0 >> 3) + half) * 27 + (26 - tap)) * Cin + ci0 + row) << 3
                          : ((((int64_t)(co0 >> 4) * 27 + (26 - tap)) * Cin + ci0 + row) << 4) + half * 8, v);
        }
    }
}

template <int FMT>
__global__ void __launch_bounds__(256)
conv3_pack_tiled_kernel(const float* __restrict__ w, bf16* __restrict__ wf, bf16* __restrict__ wb, int Cin, int Cout) {
    __shared__ float t[16][16 * 27 + 1];  // [co][ci*27 + tap]
    conv3_pack_tile<FMT>(w, wf, wb, Cin, Cout, blockIdx.x * 16, blockIdx.y * 16, t);
}

// the same over several weights in one launch (tdx_conv3_pack_weights): block -> (job, tile)
#define PACK_MAX_JOBS 32
struct PackTable {
    const float* w[PACK_MAX_JOBS];
    bf16* wf[PACK_MAX_JOBS];
    bf16* wb[PACK_MAX_JOBS];
    int Cin[PACK_MAX_JOBS], Cout[PACK_MAX_JOBS];
    int first[PACK_MAX_JOBS + 1];  // first block of job i
    int n;
};
template <int FMT>
__global__ void __launch_bounds__(256)
conv3_pack_tiled_many_kernel(PackTable tab) {
    __shared__ float t[16][16 * 27 + 1];
    int j = 0;
    while (j + 1 < tab.n && (int)blockIdx.x >= tab.first[j + 1]) ++j;
    const int tile = blockIdx.x - tab.first[j], ncx = tab.Cin[j] / 16;
    conv3_pack_tile<FMT>(tab.w[j], tab.wf[j], tab.wb[j], tab.Cin[j], tab.Cout[j], (tile % ncx) * 16, (tile / ncx) * 16, t);
}

// split-precision operands (tdx_conv3_mfma_split.hip): hi = bf16(v), lo = bf16(v - hi), two images [2][K/8][27][N][8] bf16
// in a buffer of the fp32 operand's size
__global__ void conv3_pack_split_kernel(const float* __restrict__ w, bf16* __restrict__ wf, bf16* __restrict__ wb, int Cin,
                                        int Cout) {
    const int64_t n = (int64_t)Cout * Cin * 27;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 27);
        const int64_t r = i / 27;
        const int ci = (int)(r % Cin), co = (int)(r / Cin);
        const float v = w[i];
        const bf16 hi = __float2bfloat16(v);
        const bf16 lo = __float2bfloat16(v - __bfloat162float(hi));
        if (wf) {
            const int64_t j = wp_index(8, tap, ci, co, Cin, Cout);
            wf[j] = hi;
            wf[n + j] = lo;
        }
        if (wb) {
            const int64_t j = wp_index(8, 26 - tap, co, ci, Cout, Cin);
            wb[j] = hi;
            wb[n + j] = lo;
        }
    }
}

extern "C" int tdx_conv3_pack_weight(const float* w, void* wf, void* wb, int Cin, int Cout, int dtype, void* stream) {
    TDX_CHECK_ARG(w && (wf || wb) && Cin > 0 && Cout > 0);
    const int64_t n = (int64_t)Cout * Cin * 27;
    if (dtype == TDX_F32_SPLIT) {
        // per operand: the split images where the split kernel can run (a function of (K, N) only, like every
        // layout decision here), else the plain fp32 operand
        void* sf = (wf && conv3_mfma_split_supported(Cin, 0, Cout)) ? wf : nullptr;
        void* sb = (wb && conv3_mfma_split_supported(Cout, 0, Cin)) ? wb : nullptr;
        if (sf && sb) {
            hipLaunchKernelGGL(conv3_pack_tiled_kernel<PACK_SPLIT>, dim3(Cin / 16, Cout / 16), dim3(256), 0, as_stream(stream), w,
                               (bf16*)sf, (bf16*)sb, Cin, Cout);
        } else if (sf || sb) {
            int grid = (int)min((int64_t)1024, (n + 255) / 256);
            hipLaunchKernelGGL(conv3_pack_split_kernel, dim3(grid), dim3(256), 0, as_stream(stream), w, (bf16*)sf, (bf16*)sb,
                               Cin, Cout);
        }
        void* pf = sf ? nullptr : wf;
        void* pb = sb ? nullptr : wb;
        if (pf || pb) return tdx_conv3_pack_weight(w, pf, pb, Cin, Cout, TDX_F32, stream);
        return tdx_launch_status();
    }
    const int lf = conv3_layout_kc(dtype, Cin, Cout), lb = conv3_layout_kc(dtype, Cout, Cin);
    if (tdx_is_h16(dtype) && (lf || !wf) && (lb || !wb) && (Cin % 16) == 0 && (Cout % 16) == 0) {
        if (dtype == TDX_F16)
            hipLaunchKernelGGL(conv3_pack_tiled_kernel<PACK_F16>, dim3(Cin / 16, Cout / 16), dim3(256), 0, as_stream(stream), w,
                               (bf16*)wf, (bf16*)wb, Cin, Cout);
        else
            hipLaunchKernelGGL(conv3_pack_tiled_kernel<PACK_BF16>, dim3(Cin / 16, Cout / 16), dim3(256), 0, as_stream(stream), w,
                               (bf16*)wf, (bf16*)wb, Cin, Cout);
        return tdx_launch_status();
    }
    int grid = (int)min((int64_t)1024, (n + 255) / 256);
    TDX_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv3_pack_kernel<T>), dim3(grid), dim3(256), 0, as_stream(stream),
                                                  w, (T*)wf, (T*)wb, Cin, Cout, lf, lb));
    return tdx_launch_status();
}

// Several weights in one call: the jobs whose both operands take the tiled kernel (the MFMA layouts, Cin % 16 ==
// Cout % 16 == 0 -- every 3x3x3 conv of the U-Net but the first) go out in launches of up to PACK_MAX_JOBS, the rest
// one by one through tdx_conv3_pack_weight.
extern "C" int tdx_conv3_pack_weights(const TdxPackJob* jobs, int n, int dtype, void* stream) {
    TDX_CHECK_ARG(jobs && n > 0);
    PackTable tab;
    tab.n = 0;
    tab.first[0] = 0;
    const bool split = dtype == TDX_F32_SPLIT;
    auto flush = [&]() -> int {
        if (tab.n == 0) return TDX_OK;
        if (split)
            hipLaunchKernelGGL(conv3_pack_tiled_many_kernel<PACK_SPLIT>, dim3(tab.first[tab.n]), dim3(256), 0, as_stream(stream), tab);
        else if (dtype == TDX_F16)
            hipLaunchKernelGGL(conv3_pack_tiled_many_kernel<PACK_F16>, dim3(tab.first[tab.n]), dim3(256), 0, as_stream(stream), tab);
        else
            hipLaunchKernelGGL(conv3_pack_tiled_many_kernel<PACK_BF16>, dim3(tab.first[tab.n]), dim3(256), 0, as_stream(stream), tab);
        tab.n = 0;
        return tdx_launch_status();
    };
    for (int i = 0; i < n; ++i) {
        const TdxPackJob& j = jobs[i];
        TDX_CHECK_ARG(j.w && j.wf && j.wb && j.Cin > 0 && j.Cout > 0);
        bool tiled = (j.Cin % 16) == 0 && (j.Cout % 16) == 0;
        if (split)
            tiled = tiled && conv3_mfma_split_supported(j.Cin, 0, j.Cout) && conv3_mfma_split_supported(j.Cout, 0, j.Cin);
        else
            tiled = tiled && tdx_is_h16(dtype) && conv3_layout_kc(dtype, j.Cin, j.Cout) && conv3_layout_kc(dtype, j.Cout, j.Cin);
        if (!tiled) {
            int rc = tdx_conv3_pack_weight(j.w, j.wf, j.wb, j.Cin, j.Cout, dtype, stream);
            if (rc != TDX_OK) return rc;
            continue;
        }
        const int k = tab.n++;
        tab.w[k] = j.w; tab.wf[k] = (bf16*)j.wf; tab.wb[k] = (bf16*)j.wb; tab.Cin[k] = j.Cin; tab.Cout[k] = j.Cout;
        tab.first[k + 1] = tab.first[k] + (j.Cin / 16) * (j.Cout / 16);
        if (tab.n == PACK_MAX_JOBS) {
            int rc = flush();
            if (rc != TDX_OK) return rc;
        }
    }
    return flush();
}

// Transposed copies of several fp32 matrices in one launch (the 1x1 conv weights (Cout, Cin) -> the [Cin][Cout]
// operand of tdx_conv1_fwd): dst[c][r] = src[r][c].
struct TransposeTable {
    const float* src[PACK_MAX_JOBS];
    float* dst[PACK_MAX_JOBS];
    int rows[PACK_MAX_JOBS], cols[PACK_MAX_JOBS];
    int first[PACK_MAX_JOBS + 1];
    int n;
};
__global__ void __launch_bounds__(256)
transpose_many_kernel(TransposeTable tab) {
    __shared__ float t[32][33];
    int j = 0;
    while (j + 1 < tab.n && (int)blockIdx.x >= tab.first[j + 1]) ++j;
    const int R = tab.rows[j], C = tab.cols[j];
    const int tile = blockIdx.x - tab.first[j], ntc = (C + 31) / 32;
    const int r0 = (tile / ntc) * 32, c0 = (tile % ntc) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < C) t[i][tx] = tab.src[j][(int64_t)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < C && r0 + tx < R) tab.dst[j][(int64_t)(c0 + i) * R + r0 + tx] = t[tx][i];
}
extern "C" int tdx_transpose_many(const TdxTransposeJob* jobs, int n, void* stream) {
    TDX_CHECK_ARG(jobs && n > 0);
    for (int lo = 0; lo < n; lo += PACK_MAX_JOBS) {
        TransposeTable tab;
        tab.n = min(PACK_MAX_JOBS, n - lo);
        tab.first[0] = 0;
        for (int k = 0; k < tab.n; ++k) {
            const TdxTransposeJob& j = jobs[lo + k];
            TDX_CHECK_ARG(j.src && j.dst && j.rows > 0 && j.cols > 0);
            tab.src[k] = j.src; tab.dst[k] = j.dst; tab.rows[k] = j.rows; tab.cols[k] = j.cols;
            tab.first[k + 1] = tab.first[k] + ceil_div(j.rows, 32) * ceil_div(j.cols, 32);
        }
        hipLaunchKernelGGL(transpose_many_kernel, dim3(tab.first[tab.n]), dim3(256), 0, as_stream(stream), tab);
        int rc = tdx_launch_status();
        if (rc != TDX_OK) return rc;
    }
    return TDX_OK;
}

// dwp [27][Cin][Cout] f32 -> dw (Cout, Cin, 27) f32, through a 16 (ci) x 16 (co) LDS tile so that
// both sides move 64-B+ runs; the accumulators are cleared behind the read (the workspace is left
// all-zero, see TDX_WS_CLEAN), and block (0, *) also moves the bias-gradient accumulator.
__global__ void __launch_bounds__(256)
conv3_unpack_wgrad_kernel(float* __restrict__ dwp, float* __restrict__ dw, float* __restrict__ dbw,
                          float* __restrict__ dbias, int Cin, int Cout, const float* __restrict__ slabs, int nslab) {
    __shared__ float t[16][16 * 27 + 1];  // [co][ci*27 + tap]
    const int ci0 = blockIdx.x * 16, co0 = blockIdx.y * 16;
    const int tid = threadIdx.x;
    const int ci = tid >> 4, co = tid & 15;
    const bool ok = ci0 + ci < Cin && co0 + co < Cout;
    // all 27 loads first (the clearing stores below may alias them as far as the compiler knows: interleaved, every
    // tap would wait for a full memory round trip)
    float v[27];
    const int64_t stride = (int64_t)27 * Cin * Cout, tstride = (int64_t)Cin * Cout;
    const int64_t idx0 = (int64_t)(ci0 + ci) * Cout + co0 + co;
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) v[tap] = 0.f;
    if (ok) {
        if (nslab > 0) {  // the K-splits stored their partial tiles into slabs: add them up
            for (int k = 0; k < nslab; ++k)
#pragma unroll
                for (int tap = 0; tap < 27; ++tap) v[tap] += slabs[k * stride + tap * tstride + idx0];
        } else {
#pragma unroll
            for (int tap = 0; tap < 27; ++tap) v[tap] = dwp[tap * tstride + idx0];
#pragma unroll
            for (int tap = 0; tap < 27; ++tap) dwp[tap * tstride + idx0] = 0.f;
        }
    }
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) t[co][ci * 27 + tap] = v[tap];
    __syncthreads();
    const int nci = min(16, Cin - ci0);
    for (int i = tid; i < 16 * nci * 27; i += 256) {
        const int c = i / (nci * 27), r = i - c * (nci * 27);
        if (co0 + c < Cout) dw[((int64_t)(co0 + c) * Cin + ci0) * 27 + r] = t[c][r];
    }
    if (blockIdx.x == 0 && tid < 16 && co0 + tid < Cout) {
        const float b = dbw[co0 + tid];
        dbw[co0 + tid] = 0.f;
        if (dbias) dbias[co0 + tid] = b;
    }
}

// The same unpack for launches that stored MANY per-split slabs (round 4: the fine levels' weight gradients split K over
// 32-512 workgroups; their fp32 atomic merge was 56 MB per launch at the chip's 1.3 TB/s of atomic adds = 30-43 us of
// every launch, and summed in arrival order).  Workgroup = (8 ci x 32 co) of ONE tap: a thread adds its element over the
// slabs in slab order (128-B runs per slab row, eight loads in flight) and writes dw in the parameter layout -- plain
// stores in the weight-gradient kernel, a fixed summation order here: the weight gradient is bit-reproducible.
__global__ void __launch_bounds__(256)
conv3_unpack_sum_kernel(float* __restrict__ dw, float* __restrict__ dbw, float* __restrict__ dbias, int Cin, int Cout,
                        const float* __restrict__ slabs, int nslab) {
    const int tap = blockIdx.z, ci = blockIdx.x * 8 + (threadIdx.x >> 5), co = blockIdx.y * 32 + (threadIdx.x & 31);
    const int64_t stride = (int64_t)27 * Cin * Cout;
    if (ci < Cin && co < Cout) {
        const float* p = slabs + ((int64_t)tap * Cin + ci) * Cout + co;
        float v = 0.f;
        int k = 0;
        for (; k + 8 <= nslab; k += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = p[(int64_t)(k + u) * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) v += t[u];
        }
        for (; k < nslab; ++k) v += p[(int64_t)k * stride];
        dw[((int64_t)co * Cin + ci) * 27 + tap] = v;
    }
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x < 32 && co < Cout) {
        const float b = dbw[co];
        dbw[co] = 0.f;
        if (dbias) dbias[co] = b;
    }
}

int conv3_unpack_wgrad_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p, float* dw, float* dbw, float* dbias) {
    const int Cin = c.C1 + c.C2, Cout = c.Cout;
    const int nslab = p.nslab;
    if (p.sum_unpack)
        hipLaunchKernelGGL(conv3_unpack_sum_kernel, dim3(ceil_div(Cin, 8), ceil_div(Cout, 32), 27), dim3(256), 0, c.st, dw, dbw,
                           dbias, Cin, Cout, c.slabs, nslab);
    else
        hipLaunchKernelGGL(conv3_unpack_wgrad_kernel, dim3(ceil_div(Cin, 16), ceil_div(Cout, 16)), dim3(256), 0, c.st, c.dwp, dw,
                           dbw, dbias, Cin, Cout, c.slabs, nslab);
    return tdx_launch_status();
}

// ------------------------------------------------------------------ direct implicit GEMM -
#define D3_BM 64
#define D3_BN 64
#define D3_BK 32

template <typename T, bool ZERO_PAD>
__global__ void __launch_bounds__(256)
conv3_direct_kernel(const T* __restrict__ x1, int C1, const T* __restrict__ x2, int C2, const T* __restrict__ wp,
                    const float* __restrict__ bias, T* __restrict__ y, Conv3Geom g, int Cout, int mfma_layout) {
    __shared__ float xs[D3_BK][D3_BM + 4];
    __shared__ float ws[D3_BK][D3_BN + 4];
    const int Cin = C1 + C2;
    const int64_t nvox_out = (int64_t)g.B * g.Xo * g.Yo * g.Zo;
    const int64_t m0 = (int64_t)blockIdx.x * D3_BM;
    const int n0 = blockIdx.y * D3_BN;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;

    // staging role: voxel row rr, 8-channel group kk
    const int rr = tid >> 2, kk = (tid & 3) * 8;
    const int64_t mv = m0 + rr;
    const bool row_ok = mv < nvox_out;
    int ob = 0, ox = 0, oy = 0, oz = 0;
    if (row_ok) {
        int64_t v = mv;
        oz = (int)(v % g.Zo); v /= g.Zo;
        oy = (int)(v % g.Yo); v /= g.Yo;
        ox = (int)(v % g.Xo); ob = (int)(v / g.Xo);
    }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int tap = 0; tap < 27; ++tap) {
        const int ex = tap / 9 - 1, ey = (tap / 3) % 3 - 1, ez = tap % 3 - 1;
        int sx = ox + g.off + ex, sy = oy + g.off + ey, sz = oz + g.off + ez;
        bool src_ok = row_ok;
        if (ZERO_PAD) {
            src_ok = src_ok && sx >= 0 && sx < g.Xi && sy >= 0 && sy < g.Yi && sz >= 0 && sz < g.Zi;
        } else {
            sx = min(max(sx, 0), g.Xi - 1); sy = min(max(sy, 0), g.Yi - 1); sz = min(max(sz, 0), g.Zi - 1);
        }
        const int64_t sv = (((int64_t)ob * g.Xi + sx) * g.Yi + sy) * g.Zi + sz;
        for (int k0 = 0; k0 < Cin; k0 += D3_BK) {
            {
                const int k = k0 + kk;
                Vec8<T> a;
#pragma unroll
                for (int j = 0; j < 8; ++j) a.v[j] = 0.f;
                if (src_ok && k < Cin) {
                    if (k < C1) a.load(x1 + sv * C1 + k);
                    else a.load(x2 + sv * C2 + (k - C1));
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) xs[kk + j][rr] = a.v[j];
            }
            {
                const int kq = tid >> 3, nn = (tid & 7) * 8;
                const int k = k0 + kq;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int n = n0 + nn + j;
                    ws[kq][nn + j] = (k < Cin && n < Cout) ? ldf(wp + wp_index(mfma_layout, tap, k, n, Cin, Cout)) : 0.f;
                }
            }
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < D3_BK; ++k) {
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
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + ty * 4 + i;
        if (m >= nvox_out) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= Cout) continue;
            float v = acc[i][j];
            if (bias) v += bias[n];
            stf(y + m * Cout + n, v);
        }
    }
}

int conv3_direct_launch(const Conv3Call& c) {
    if ((c.C1 % 8) || (c.C2 % 8)) return TDX_ESHAPE;
    // data gradient: the adjoint on the padded grid, dpad[p'] = sum_e wb[e] dy_zero[p' - 1 + e]
    const Conv3Geom g = c.zero_pad ? Conv3Geom{c.B, c.X, c.Y, c.Z, c.X + 2, c.Y + 2, c.Z + 2, -1} : c.geom();
    const int64_t nvox = (int64_t)g.B * g.Xo * g.Yo * g.Zo;
    dim3 grid(ceil_div(nvox, D3_BM), ceil_div(c.N, D3_BN));
    const int ml = conv3_layout_kc(c.fmt, c.C1 + c.C2, c.N);
    TDX_DISPATCH_DTYPE(c.fmt, {
        if (c.zero_pad)
            hipLaunchKernelGGL((conv3_direct_kernel<T, true>), grid, dim3(256), 0, c.st, (const T*)c.x1, c.C1, (const T*)c.x2,
                               c.C2, (const T*)c.wp, c.bias, (T*)c.y, g, c.N, ml);
        else
            hipLaunchKernelGGL((conv3_direct_kernel<T, false>), grid, dim3(256), 0, c.st, (const T*)c.x1, c.C1,
                               (const T*)c.x2, c.C2, (const T*)c.wp, c.bias, (T*)c.y, g, c.N, ml);
    });
    return tdx_launch_status();
}

// ------------------------------------------------------------------ halo fold ------------
// dx[b,u,:] (+)= sum over padded positions p with clamp(p) == u of dpad[b,p,:]
// dpad grid is (X+2, Y+2, Z+2) with p' = p + 1.  Channels are split over dx1 | dx2.
__device__ __forceinline__ void fold_range(int u, int n, int& lo, int& hi) {
    lo = (u == 0) ? 0 : u + 1;
    hi = (u == n - 1) ? n + 1 : u + 1;
}
template <typename T>
__global__ void __launch_bounds__(256)
conv3_fold_kernel(const T* __restrict__ dpad, T* __restrict__ dx1, int C1, T* __restrict__ dx2, int C2,
                  const T* __restrict__ add1, const T* __restrict__ add2,
                  int B, int X, int Y, int Z, int64_t total) {
    const int C = C1 + C2;
    const int L = C >> 3;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lc = (int)(i % L);
    int64_t v = i / L;
    const int64_t vox = v;
    const int uz = (int)(v % Z); v /= Z;
    const int uy = (int)(v % Y); v /= Y;
    const int ux = (int)(v % X);
    const int b = (int)(v / X);
    int x0, x1, y0, y1, z0, z1;
    fold_range(ux, X, x0, x1);
    fold_range(uy, Y, y0, y1);
    fold_range(uz, Z, z0, z1);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const int Xp = X + 2, Yp = Y + 2, Zp = Z + 2;
    for (int px = x0; px <= x1; ++px)
        for (int py = y0; py <= y1; ++py)
            for (int pz = z0; pz <= z1; ++pz) {
                Vec8<T> t;
                t.load(dpad + ((((int64_t)b * Xp + px) * Yp + py) * Zp + pz) * C + lc * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += t.v[j];
            }
    const int c = lc * 8;
    T* dst = (c < C1) ? dx1 + vox * C1 + c : dx2 + vox * C2 + (c - C1);
    Vec8<T> o;
    const T* asrc = (c < C1) ? (add1 ? add1 + vox * C1 + c : nullptr) : (add2 ? add2 + vox * C2 + (c - C1) : nullptr);
    if (asrc) {
        o.load(asrc);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] += acc[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = acc[j];
    }
    o.store(dst);
}

int conv3_fold_launch(const Conv3Call& c) {
    const int64_t total = (int64_t)c.B * c.X * c.Y * c.Z * (c.N / 8);
    TDX_DISPATCH_DTYPE(c.fmt, hipLaunchKernelGGL((conv3_fold_kernel<T>), dim3(ceil_div(total, 256)), dim3(256), 0, c.st,
                                                  (const T*)c.y, (T*)c.d1, c.D1, (T*)c.d2, c.N - c.D1, (const T*)c.a1,
                                                  (const T*)c.a2, c.B, c.X, c.Y, c.Z, total));
    return tdx_launch_status();
}

// ------------------------------------------------------------------ direct weight grad ---
// dwp[tap][ci][co] += sum over a chunk of voxels of x[clamp(v+tap), ci] * dy[v, co]
#define D3W_VOX 8192
template <typename T>
__global__ void __launch_bounds__(256)
conv3_wgrad_direct_kernel(const T* __restrict__ x1, int C1, const T* __restrict__ x2, int C2,
                          const T* __restrict__ dy, float* __restrict__ dwp, float* __restrict__ dbias, int B, int X,
                          int Y, int Z, int Cout, int n_ci_tiles, int64_t vpb, int64_t slab_stride) {
    // vpb: voxels per block (D3W_VOX).  slab_stride != 0 (TDX_DETERMINISTIC): voxel chunk k STORES its partial sums into
    // slab k (every element of a slab has exactly one writer); the unpack kernel adds the slabs in order
    __shared__ float xs[D3_BK][D3_BM + 4];  // [voxel slice][ci]
    __shared__ float gs[D3_BK][D3_BN + 4];  // [voxel slice][co]
    const int Cin = C1 + C2;
    const int64_t nvox = (int64_t)B * X * Y * Z;
    const int64_t vbeg = (int64_t)blockIdx.x * vpb;
    const int64_t vend = min(nvox, vbeg + vpb);
    dwp += (int64_t)blockIdx.x * slab_stride;
    const int tap = blockIdx.y;
    const int ci0 = (blockIdx.z % n_ci_tiles) * D3_BM, co0 = (blockIdx.z / n_ci_tiles) * D3_BN;
    const int ex = tap / 9 - 1, ey = (tap / 3) % 3 - 1, ez = tap % 3 - 1;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int rr = tid >> 3, cc = (tid & 7) * 8;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    float bsum = 0.f;
    const bool do_bias = dbias && tap == 13 && ci0 == 0;

    for (int64_t vs = vbeg; vs < vend; vs += D3_BK) {
        const int64_t v = vs + rr;
        Vec8<T> a, gq;
#pragma unroll
        for (int j = 0; j < 8; ++j) a.v[j] = gq.v[j] = 0.f;
        if (v < vend) {
            int64_t t = v;
            const int oz = (int)(t % Z); t /= Z;
            const int oy = (int)(t % Y); t /= Y;
            const int ox = (int)(t % X);
            const int ob = (int)(t / X);
            const int sx = min(max(ox + ex, 0), X - 1), sy = min(max(oy + ey, 0), Y - 1),
                      sz = min(max(oz + ez, 0), Z - 1);
            const int64_t sv = (((int64_t)ob * X + sx) * Y + sy) * Z + sz;
            const int ci = ci0 + cc, co = co0 + cc;
            if (ci < Cin) {
                if (ci < C1) a.load(x1 + sv * C1 + ci);
                else a.load(x2 + sv * C2 + (ci - C1));
            }
            if (co < Cout) gq.load(dy + v * Cout + co);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { xs[rr][cc + j] = a.v[j]; gs[rr][cc + j] = gq.v[j]; }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < D3_BK; ++k) {
            const float4 av4 = *reinterpret_cast<const float4*>(&xs[k][ty * 4]);
            const float4 bv4 = *reinterpret_cast<const float4*>(&gs[k][tx * 4]);
            const float av[4] = {av4.x, av4.y, av4.z, av4.w}, bv[4] = {bv4.x, bv4.y, bv4.z, bv4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
        }
        if (do_bias && tid < D3_BN) {
#pragma unroll 8
            for (int k = 0; k < D3_BK; ++k) bsum += gs[k][tid];
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
            if (co >= Cout) continue;
            if (slab_stride) dwp[((int64_t)tap * Cin + ci) * Cout + co] = acc[i][j];
            else atomicAdd(&dwp[((int64_t)tap * Cin + ci) * Cout + co], acc[i][j]);
        }
    }
    if (do_bias && tid < D3_BN && co0 + tid < Cout) atomicAdd(&dbias[co0 + tid], bsum);
}

// voxels per block: D3W_VOX, or with max_slabs > 0 what leaves at most max_slabs voxel chunks, one slab each
static int64_t d3w_vpb(int64_t nvox, int max_slabs) {
    return max_slabs > 0 ? (ceil_div(nvox, max_slabs) + D3_BK - 1) / D3_BK * D3_BK : D3W_VOX;
}
bool conv3_wgrad_direct_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs) {
    const int64_t nvox = (int64_t)c.B * c.X * c.Y * c.Z;
    p.kernel = TDX_WGRAD_DIRECT; p.nt = 0; p.depth = 0; p.nbricks = 0;
    p.nsplit = ceil_div(nvox, d3w_vpb(nvox, max_slabs));
    p.nslab = max_slabs > 0 ? p.nsplit : 0;
    p.max_slabs = max_slabs;
    return true;
}

int conv3_wgrad_direct_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p, int dtype) {
    const int64_t nvox = (int64_t)c.B * c.X * c.Y * c.Z;
    const int Cin = c.C1 + c.C2, nci = ceil_div(Cin, D3_BM), nco = ceil_div(c.Cout, D3_BN);
    const int64_t vpb = d3w_vpb(nvox, p.max_slabs);
    int64_t slab_stride;
    float* out = conv3_wgrad_out(c, p, slab_stride);
    dim3 grid(ceil_div(nvox, vpb), 27, nci * nco);
    TDX_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((conv3_wgrad_direct_kernel<T>), grid, dim3(256), 0, c.st, (const T*)c.x1, c.C1,
                                                  (const T*)c.x2, c.C2, (const T*)c.dy, out, c.dbias, c.B, c.X, c.Y, c.Z, c.Cout,
                                                  nci, vpb, slab_stride));
    return tdx_launch_status();
}
