// fp32 MFMA implicit-GEMM 3x3x3 convolution (forward and, zero-padded, the main term of the data
// gradient) for the fp32 parity mode.  gfx950, v_mfma_f32_32x32x2_f32 (256 FLOP/clk/CU: the same peak as
// the packed-FMA vector ALU, but fed from an LDS halo brick with 27-fold reuse instead of a tile that is
// re-fetched for every tap).
//
// Same structure as the bf16 kernel (tdx_conv3_mfma.hip), in its plainest form: a workgroup owns a
// 4 x 8 x 8 brick of output voxels and BN = 32 * NT output channels; K = 27 taps x input channels is
// walked in 8-channel slices.  Per slice the halo'd brick (6 x 10 x 10 voxels x 8 ch) and the slice's
// weights of all 27 taps go to LDS as two half-planes of 16-B entries (4 fp32 channels each; the brick's z
// stride is padded 10 -> 12 so that fragment reads are conflict-free with affine addresses); the next
// slice's global loads are in flight during the MFMAs of the current one.  A lane reads one 16-B entry
// per operand and tap and feeds its four floats to four MFMAs (lanes 0-31 carry k = 0, lanes 32-63
// k = 1 of each 32x32x2 step: channel 4*(lane >> 5) + j for the j-th MFMA, on both operands).
// The MFMA is issued transposed (weights as A), so a lane owns one voxel and 4 consecutive channels per
// accumulator quad: 16-B writes into an LDS output tile, then full-row coalesced stores (conv3_epilogue_f32,
// tdx_conv3_epilogue.h).
// Products and sums are IEEE fp32 (no reduced-precision operands): the 1e-4 parity gate holds as with
// the vector-ALU kernels; only the summation order differs.
#include "tdx_common.h"
#include "tdx_conv3.h"
#include "tdx_conv3_epilogue.h"

#define F3_KC 8

bool conv3_mfma_f32_supported(int C1, int C2, int Cout) {
    return C1 > 0 && (C1 % F3_KC) == 0 && (C2 % F3_KC) == 0 && (Cout % 32) == 0;
}

template <int NT, bool ZERO_PAD, int SHAPE, bool PERM>
__global__ void __launch_bounds__(256, 2)
conv3_mfma_f32_kernel(const float* __restrict__ x1, int C1, const float* __restrict__ x2, int C2,
                      const float* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y, BrickRegions R,
                      int Cout, double* __restrict__ gn_acc, float* __restrict__ d1, int D1, float* __restrict__ d2,
                      const float* __restrict__ a1, const float* __restrict__ a2) {
    using BR = Brick<SHAPE>;
    constexpr int MT = BR::MT;
    constexpr int BN = NT * 32;
    constexpr int HY = BR::HY, HZ = BR::HZ, SZ = BR::SZ;
    constexpr int NHALO = BR::NHALO;
    constexpr int APLANE = BR::ENTRIES * 16 + 64;
    constexpr int BRICK_BYTES = 2 * APLANE;
    constexpr int B_PLANE = 27 * BN * 16 + 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;
    unsigned char* sB = smem + BRICK_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;

    int b, o[3];
    const BrickView& g = brick_decode<SHAPE>(R, xcd_contiguous((int)blockIdx.x, (int)gridDim.x), b, o);
    const int n0 = blockIdx.y * BN;
    const int Cin = C1 + C2;

    // staging plan of the halo brick: 2 * NHALO 16-B pieces (voxel, half = channel group of 4)
    constexpr int A_PIECES = NHALO * 2;
    constexpr int A_PER_THREAD = (A_PIECES + 255) / 256;
    constexpr int B_PIECES = 27 * BN * 2;
    constexpr int B_PER_THREAD = (B_PIECES + 255) / 256;
    int a_src[A_PER_THREAD], a_dst[A_PER_THREAD];
#pragma unroll
    for (int i = 0; i < A_PER_THREAD; ++i) {
        const int p = tid + i * 256;
        a_dst[i] = -1;
        a_src[i] = -1;
        if (p < A_PIECES) {
            const int hv = ((p >> 3) << 2) + (p & 3), half = (p >> 2) & 1;
            const int hx = hv / (HY * HZ), rem = hv - hx * (HY * HZ);
            const int hy = rem / HZ, hz = rem - hy * HZ;
            a_dst[i] = half * APLANE + ((hx * HY + hy) * SZ + hz) * 16;
            const int src = brick_halo_source<ZERO_PAD, PERM>(g, o, hx, hy, hz);
            if (src >= 0) a_src[i] = src * 2 + half;
        }
    }
    const int64_t batch_vox = (int64_t)b * g.Ei[0] * g.Ei[1] * g.Ei[2];

    // weight staging role: (row = b_row0 + 128 i, half); packed layout [K/8][27][Cout][8]
    const int b_half = (tid >> 2) & 1;
    const int b_row0 = ((tid >> 3) << 2) + (tid & 3);
    const int b_goff = ((b_row0 / BN) * Cout + (b_row0 % BN)) * F3_KC + b_half * 4;
    const int b_dst = b_half * B_PLANE + b_row0 * 16;

    float4 areg[A_PER_THREAD], breg[B_PER_THREAD];
    auto load_slice = [&](int c) {
        const int k0 = c * F3_KC;
        const float* xs;
        int Cs, kk;
        if (k0 < C1) { xs = x1; Cs = C1; kk = k0; } else { xs = x2; Cs = C2; kk = k0 - C1; }
        xs += batch_vox * Cs + kk;
#pragma unroll
        for (int i = 0; i < A_PER_THREAD; ++i) {
            areg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a_src[i] >= 0)
                areg[i] = *reinterpret_cast<const float4*>(xs + (int64_t)(a_src[i] >> 1) * Cs + (a_src[i] & 1) * 4);
        }
        const float* wc = wp + (int64_t)c * 27 * Cout * F3_KC + (int64_t)n0 * F3_KC + b_goff;
#pragma unroll
        for (int i = 0; i < B_PER_THREAD; ++i) {
            breg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b_row0 + 128 * i < 27 * BN)
                breg[i] = *reinterpret_cast<const float4*>(wc + (int64_t)i * (128 / BN) * Cout * F3_KC);
        }
    };
    auto store_slice = [&]() {
#pragma unroll
        for (int i = 0; i < A_PER_THREAD; ++i)
            if (a_dst[i] >= 0) *reinterpret_cast<float4*>(sA + a_dst[i]) = areg[i];
#pragma unroll
        for (int i = 0; i < B_PER_THREAD; ++i)
            if (b_row0 + 128 * i < 27 * BN) *reinterpret_cast<float4*>(sB + b_dst + i * 2048) = breg[i];
    };

    // this lane's voxel of M tile mt (Brick<THIN>::lane_voxel)
    int a_h[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int lx, ly, lz;
        BR::lane_voxel(wave, mt, r, lx, ly, lz);
        a_h[mt] = ((lx + 1) * HY + (ly + 1)) * SZ + (lz + 1);
    }
    int tap_row[27];  // weight-image row of every local tap (immediates when the axes are not permuted)
#pragma unroll
    for (int t = 0; t < 27; ++t) tap_row[t] = (PERM ? brick_tap(g, t / 9 - 1, (t / 3) % 3 - 1, t % 3 - 1) : t) * (BN * 16);
    int b_off[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_off[nt] = hh * B_PLANE + (nt * 32 + r) * 16;

    f32x16 acc[NT][MT];  // D[row = channel][col = voxel]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][mt][i] = 0.f;

    const int nchunks = Cin / F3_KC;
    load_slice(0);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();
        store_slice();
        __syncthreads();
        if (c + 1 < nchunks) load_slice(c + 1);
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            const int ex = tap / 9 - 1, ey = (tap / 3) % 3 - 1, ez = tap % 3 - 1;
            const int toff = (ex * HY + ey) * SZ + ez;
            float4 xf[MT], wf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xf[mt] = *reinterpret_cast<const float4*>(sA + hh * APLANE + (a_h[mt] + toff) * 16);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wf[nt] = *reinterpret_cast<const float4*>(sB + tap_row[tap] + b_off[nt]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[nt].x, xf[mt].x, acc[nt][mt], 0, 0, 0);
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[nt].y, xf[mt].y, acc[nt][mt], 0, 0, 0);
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[nt].z, xf[mt].z, acc[nt][mt], 0, 0, 0);
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[nt].w, xf[mt].w, acc[nt][mt], 0, 0, 0);
                }
        }
    }

    conv3_epilogue_f32<NT, ZERO_PAD, SHAPE, PERM>(acc, smem, g, o, b, n0, bias, y, Cout, gn_acc, d1, D1, d2, a1, a2);
}

template <int NT, bool ZP, int SHAPE, bool PERM>
static int f32_go(const Conv3Call& c, const BrickRegions& reg) {
    constexpr int BN = NT * 32;
    size_t lds = (size_t)2 * (Brick<SHAPE>::ENTRIES * 16 + 64) + (size_t)2 * (27 * BN * 16 + 64);
    const size_t tile = (size_t)Brick<SHAPE>::NVOX * BN * 4 + 8192;  // epilogue: output tile + moment reduction
    if (tile > lds) lds = tile;
    if (!brick_closed(reg)) return TDX_EINVAL;
    return tdx_launch_lds<conv3_mfma_f32_kernel<NT, ZP, SHAPE, PERM>>(
        dim3((unsigned)reg.start[reg.n], c.N / BN), dim3(256), lds, c.st, (const float*)c.x1, c.C1, (const float*)c.x2, c.C2,
        (const float*)c.wp, c.bias, (float*)c.y, reg, c.N, c.gn_acc, (float*)c.d1, c.D1, (float*)c.d2, (const float*)c.a1,
        (const float*)c.a2);
}

int conv3_mfma_f32_launch(const Conv3Call& c) {
    if (c.fmt != TDX_F32 || (c.zero_pad && c.d1 == nullptr)) return TDX_EINVAL;
    const Conv3Geom g = c.geom();
    if ((int64_t)g.Xi * g.Yi * g.Zi * 2 >= (1ll << 31) || (int64_t)g.Xo * g.Yo * g.Zo >= (1ll << 31)) return TDX_ESHAPE;
    // 4 x 8 x 8 bricks only (8 x 8 x 8 bricks with four M tiles per wave, which pay in the split kernel, measured 25-35 %
    // SLOWER here: this kernel is MFMA-bound with two workgroups per CU already)
    BrickRegions main, thin;
    brick_plan(g, c.zero_pad, conv3_thin_slabs() != 0, main, thin);
    int rc = TDX_OK;
    TDX_DISPATCH_BOOL(c.N % 64 == 0, WIDE, TDX_DISPATCH_BOOL(c.zero_pad, ZP, TDX_DISPATCH_BOOL(main.v[0].perm[0] != 0, PM,
        rc = f32_go<WIDE ? 2 : 1, ZP, BRICK_MAIN, PM>(c, main))));
    if (rc != TDX_OK || thin.n == 0) return rc;
    // remainder slabs of the data gradient on big grids: 2 x 16 x 8 bricks
    TDX_DISPATCH_BOOL(c.N % 64 == 0, WIDE, rc = f32_go<WIDE ? 2 : 1, true, BRICK_THIN, true>(c, thin));
    return rc;
}
