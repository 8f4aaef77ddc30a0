// What the forward / data-gradient kernels of the 3x3x3 convolution share behind their K loops: the swizzle of the LDS
// output tile, the data gradient's store, the fused GroupNorm moments, and the whole epilogue of the two fp32-tensor brick
// kernels (tdx_conv3_mfma_f32.hip, tdx_conv3_mfma_split_kernel.h).  The 16-bit brick kernel (tdx_conv3_mfma.hip) uses the
// pieces; the ring kernel (tdx_conv3_ring.hip) the tile address: it keeps its own moments (registers across the bricks of a
// sample) and has the dx store written out in place (behind the call its bf16 instantiations compiled to split stores).
//
// The data gradient runs on the ORIGINAL grid (Conv3Call::geom(): equal grids, off = 0; its halo-shell term is
// tdx_conv3_shell.hip), so an output voxel of a zero-padded launch IS the voxel of dx it belongs to: no in-grid test, no
// workspace behind it.  A zero-padded launch therefore needs d1 (the launchers check).
#pragma once
#include "tdx_common.h"
#include "tdx_conv3.h"
#include "tdx_conv3_brick.h"
#include "tdx_mfma.h"

// ---- LDS output tile: rows of BN channels, 16-B chunk c of row v at c ^ swizzle(v)
// 16-bit rows of 64 B (BN = 32) or 128 B (BN = 64)
template <int BN>
__device__ __forceinline__ int conv3_tile_addr16(int v, int c) {
    if (BN == 64) return v * 128 + ((c ^ (v & 7)) << 4);
    return v * 64 + ((c ^ ((v >> 1) & 3)) << 4);
}
// fp32 rows of BN floats
template <int BN>
__device__ __forceinline__ int conv3_tile_addr32(int v, int c) {
    return v * (BN * 4) + ((c ^ (v & (BN / 4 - 1))) << 4);
}

// ---- data gradient: one 16-B chunk (result channels [n, n + 8) or [n, n + 4)) of voxel u, counted over the batch.  The N
// result channels are split over the two inputs of a concatenated conv, d1 (channels [0, D1)) | d2, each plus its addend
// a1 | a2 where given (the gradient that arrives over the block's residual path).
template <typename HT>
__device__ __forceinline__ void conv3_store_dx(uint4 val, int64_t u, int n, int N, bf16* d1, int D1, bf16* d2,
                                               const bf16* a1, const bf16* a2) {
    const bool lo = n < D1;
    bf16* dst = lo ? d1 + u * D1 + n : d2 + u * (N - D1) + (n - D1);
    const bf16* asrc = lo ? (a1 ? a1 + u * D1 + n : nullptr) : (a2 ? a2 + u * (N - D1) + (n - D1) : nullptr);
    if (asrc) {
        Vec8<HT> va, vb;
        va.load(reinterpret_cast<const HT*>(&val));
        vb.load(reinterpret_cast<const HT*>(asrc));
#pragma unroll
        for (int e = 0; e < 8; ++e) va.v[e] += vb.v[e];
        va.store(reinterpret_cast<HT*>(dst));
    } else {
        *reinterpret_cast<uint4*>(dst) = val;
    }
}
__device__ __forceinline__ void conv3_store_dx(float4 val, int64_t u, int n, int N, float* __restrict__ d1, int D1,
                                               float* __restrict__ d2, const float* __restrict__ a1, const float* __restrict__ a2) {
    const bool lo = n < D1;
    float* dst = lo ? d1 + u * D1 + n : d2 + u * (N - D1) + (n - D1);
    const float* asrc = lo ? (a1 ? a1 + u * D1 + n : nullptr) : (a2 ? a2 + u * (N - D1) + (n - D1) : nullptr);
    if (asrc) {
        const float4 av = *reinterpret_cast<const float4*>(asrc);
        val.x += av.x; val.y += av.y; val.z += av.z; val.w += av.w;
    }
    *reinterpret_cast<float4*>(dst) = val;
}

// ---- fused GroupNorm statistics of the forward (tdx_conv3_fwd_gn): per-channel sum and sum of squares of the stored
// (rounded) tile, so that the read pass over y is saved.  A thread of the store loop owns E channels (one 16-B chunk):
// accumulate per thread, reduce over the workgroup through LDS, merge across workgroups with one f64 atomic per channel
// and moment.
template <typename H>
__device__ __forceinline__ void conv3_moments_add(const uint4& val, float (&s1)[8], float (&s2)[8]) {
    const unsigned wds[4] = {val.x, val.y, val.z, val.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float lo = H::lo(wds[e]), hi = H::hi(wds[e]);
        s1[2 * e] += lo; s2[2 * e] += lo * lo;
        s1[2 * e + 1] += hi; s2[2 * e + 1] += hi * hi;
    }
}
__device__ __forceinline__ void conv3_moments_add(const float4& val, float (&s1)[4], float (&s2)[4]) {
    s1[0] += val.x; s2[0] += val.x * val.x; s1[1] += val.y; s2[1] += val.y * val.y;
    s1[2] += val.z; s2[2] += val.z * val.z; s1[3] += val.w; s2[3] += val.w * val.w;
}
// 256 threads; thread tid holds chunk tid % (BN / E).  red: [256 E / BN][BN][2] floats of LDS (behind the output tile).
// 32 replicas of the [B][Cout][2] table, picked by workgroup: all workgroups of a sample would otherwise hammer the same
// 2 Cout addresses
template <int BN, int E>
__device__ __forceinline__ void conv3_moments_merge(const float (&s1)[E], const float (&s2)[E], float* red,
                                                    double* __restrict__ gn_acc, int B, int b, int Cout, int n0) {
    constexpr int CHUNKS = BN / E, NP = 256 / CHUNKS;  // NP: threads per chunk column
    const int tid = threadIdx.x;
    const int cidx = tid % CHUNKS, part = tid / CHUNKS;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        red[(part * BN + cidx * E + e) * 2] = s1[e];
        red[(part * BN + cidx * E + e) * 2 + 1] = s2[e];
    }
    __syncthreads();
    if (tid < BN * 2) {
        float t = 0.f;
#pragma unroll 8
        for (int pp = 0; pp < NP; ++pp) t += red[pp * BN * 2 + tid];
        const int rep = blockIdx.x & (TDX_GN_REPLICAS - 1);
        atomicAdd(&gn_acc[(((size_t)rep * B + b) * Cout + n0) * 2 + tid], (double)t);
    }
}

// ---- the epilogue of the fp32-tensor brick kernels.  acc: D[row = channel][col = voxel] of the transposed MFMA; lane
// (r, hh) of wave w holds, for M tile mt, the voxel Brick<SHAPE>::lane_voxel(w, mt, r) and channels nt*32 + 8 j + 4 hh +
// (0..3) in accumulator registers 4 j .. 4 j + 3: bias added, 16-B writes into the LDS tile [NVOX voxels][BN] fp32 (smem
// is free: the caller's K loop is done), then whole voxel rows to y, or to dx (ZERO_PAD).
template <int NT, bool ZERO_PAD, int SHAPE, bool PERM>
__device__ __forceinline__ void conv3_epilogue_f32(const f32x16 (&acc)[NT][Brick<SHAPE>::MT], unsigned char* smem,
                                                   const BrickView& g, const int (&o)[3], int b, int n0,
                                                   const float* __restrict__ bias, float* __restrict__ y, int Cout,
                                                   double* __restrict__ gn_acc, float* __restrict__ d1, int D1,
                                                   float* __restrict__ d2, const float* __restrict__ a1,
                                                   const float* __restrict__ a2) {
    using BR = Brick<SHAPE>;
    constexpr int MT = BR::MT, BN = NT * 32;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    __syncthreads();
    unsigned char* sO = smem;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = nt * 32 + 8 * j + 4 * hh;
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bias) bv = *reinterpret_cast<const float4*>(bias + n0 + ch);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                int lx, ly, lz;
                BR::lane_voxel(wave, mt, r, lx, ly, lz);
                const int v = BR::tile_index(lx, ly, lz);
                *reinterpret_cast<float4*>(sO + conv3_tile_addr32<BN>(v, ch >> 2)) =
                    make_float4(acc[nt][mt][4 * j] + bv.x, acc[nt][mt][4 * j + 1] + bv.y, acc[nt][mt][4 * j + 2] + bv.z,
                                acc[nt][mt][4 * j + 3] + bv.w);
            }
        }
    __syncthreads();
    constexpr int CHUNKS = BN / 4;  // 16-B chunks per voxel row
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};  // GroupNorm moments of this thread's 4 channels
#pragma unroll
    for (int i = 0; i < CHUNKS * (BR::NVOX / 256); ++i) {
        const int p = tid + i * 256;
        const int v = p / CHUNKS, cidx = p % CHUNKS;
        int lx, ly, lz, vox;
        BR::tile_voxel(v, lx, ly, lz);
        if (brick_out_voxel<PERM>(g, o, lx, ly, lz, vox)) {
            const int64_t ov = (int64_t)b * g.Eo[0] * g.Eo[1] * g.Eo[2] + vox;
            const float4 val = *reinterpret_cast<const float4*>(sO + conv3_tile_addr32<BN>(v, cidx));
            if (ZERO_PAD) {
                conv3_store_dx(val, ov, n0 + cidx * 4, Cout, d1, D1, d2, a1, a2);
            } else {
                *reinterpret_cast<float4*>(y + ov * Cout + n0 + cidx * 4) = val;
                if (gn_acc != nullptr) conv3_moments_add(val, s1, s2);
            }
        }
    }
    if (!ZERO_PAD && gn_acc != nullptr)
        conv3_moments_merge<BN, 4>(s1, s2, reinterpret_cast<float*>(smem + BR::NVOX * BN * 4), gn_acc, g.B, b, Cout, n0);
}
