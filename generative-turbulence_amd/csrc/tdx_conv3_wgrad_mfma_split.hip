// Split-precision ("bf16x2") MFMA weight gradient of the replicate-padded 3x3x3 convolution for fp32 tensors
// (gfx950, opt-in with TDX_CONV_SPLIT; see tdx_conv3_mfma_split.hip for the arithmetic):
//
//   dW[tap][ci][co] = sum_v x[clamp(v + tap)][ci] * dy[v][co]
//                  ~= sum_v  xh * dyh + xl * dyh + xh * dyl        (bf16 hi / lo terms, fp32 accumulation)
//
// The structure is that of the bf16 kernel (tdx_conv3_wgrad_mfma.hip): a TN GEMM per tap over the voxels of
// 4 x 8 x 8 bricks, both operands voxel-major, fragments by transposed LDS reads (ds_read_b64_tr_b16) of
// 64-B rows; a workgroup owns a 32 (ci) x 32 (co) tile of all 27 taps, wave w the taps w, w + 4, ...
// (7 x 16 accumulator registers).  Differences: the operands are loaded as fp32 and split into a hi and a lo
// bf16 image while they are written to LDS (x: 2 x 38 KB, dy: 2 x 16 KB -> one workgroup per CU), each
// (tap, K-step) issues three MFMAs, the output tile is 32 channels wide (NT = 1: the second register set of
// the double-buffered fragments takes the room of the second accumulator tile), and the bias gradient is
// summed from the fp32 staging registers, i.e. exactly.
#include "tdx_conv3_wgrad.h"
#include <stdlib.h>

typedef WgradBrick<4> WS;                            // 4 x 8 x 8 bricks; an image (hi or lo) has 64-B rows of 32 bf16 channels
#define WS_NSTEPS (WS::NVOX / 16)                    // K-steps of 16 voxels
#define WS_TAPS 7

bool conv3_wgrad_mfma_split_supported(int C1, int C2, int Cout) {
    const bool c1_ok = (C1 % 32) == 0 || (C2 == 0 && (C1 % 8) == 0);
    return C1 > 0 && c1_ok && (C2 % 32) == 0 && (Cout % 32) == 0;
}

__global__ void __launch_bounds__(256, 1)
conv3_wgrad_mfma_split_kernel(const float* __restrict__ x1, int C1, const float* __restrict__ x2, int C2,
                              const float* __restrict__ dy, float* __restrict__ dwp, float* __restrict__ dbias, WgradView gv,
                              int Cout, int nsplit, int n_ci_tiles, int64_t slab_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sXh = smem;
    unsigned char* sXl = smem + WS::XBYTES;
    unsigned char* sGh = smem + 2 * WS::XBYTES;
    unsigned char* sGl = sGh + WS::GPLANE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cin = C1 + C2;
    const int tile = blockIdx.x / nsplit, split = blockIdx.x - tile * nsplit;
    const int ci0 = (tile % n_ci_tiles) * 32;
    const int co0 = (tile / n_ci_tiles) * 32;
    const float* xs;
    int Cs, cbase;
    if (ci0 < C1) { xs = x1; Cs = C1; cbase = ci0; } else { xs = x2; Cs = C2; cbase = ci0 - C1; }

    const int nbricks = gv.B * gv.nb[0] * gv.nb[1] * gv.nb[2];

    const WgradLane L = wgrad_lane(lane);  // fragment lane geometry
    const int q = L.q, kh = L.kh, col_off = L.col_off;

    f32x16 acc[WS_TAPS];
#pragma unroll
    for (int t = 0; t < WS_TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    const bool do_bias = dbias != nullptr && ci0 == 0;
    float bs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bs[e] = 0.f;

    int a_off[WS_TAPS];  // byte offset inside an x image of this lane's fragment at step 0, per tap
#pragma unroll
    for (int t = 0; t < WS_TAPS; ++t) {
        a_off[t] = wgrad_x_frag_row<WS>(L, WS::tap_offset(min(wave + 4 * t, 26))) * 64 + col_off;
    }

    constexpr int XP = (WS::NHALO * 4 + 255) / 256;  // pieces of 8 fp32 channels per thread (10)
    constexpr int GP = (WS::NVOX * 4) / 256;          // 4
    float4 xreg[XP][2], greg[GP][2];

    auto load_brick = [&](int brick) {
        int bx, by, bz;
        const int b = wgrad_brick_coords(gv, brick, bx, by, bz);
        const int ox0 = bx * WS::BX, oy0 = by * WS::BY, oz0 = bz * WS::BZ;
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int pc = tid + i * 256;
            xreg[i][0] = xreg[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pc < WS::NHALO * 4 && cbase + (pc & 3) * 8 < Cs) {
                const int q4 = pc & 3;
                int hx, hy, hz;
                WS::halo_coords(pc >> 2, hx, hy, hz);
                const int64_t vox = WS::halo_source(gv, b, bx, by, bz, hx, hy, hz);
                const float4* src = reinterpret_cast<const float4*>(xs + vox * Cs + cbase + q4 * 8);
                xreg[i][0] = src[0];
                xreg[i][1] = src[1];
            }
        }
#pragma unroll
        for (int i = 0; i < GP; ++i) {
            const int pc = tid + i * 256;
            const int v = pc >> 2, q8 = pc & 3;
            const int vx = ox0 + (v >> 6), vy = oy0 + ((v >> 3) & 7), vz = oz0 + (v & 7);
            greg[i][0] = greg[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (vx < gv.E[0] && vy < gv.E[1] && vz < gv.E[2]) {
                const int64_t vox = wgrad_voxel(gv, b, vx, vy, vz);
                const float4* src = reinterpret_cast<const float4*>(dy + vox * Cout + co0 + q8 * 8);
                greg[i][0] = src[0];
                greg[i][1] = src[1];
            }
        }
    };
    auto store_brick = [&]() {
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int pc = tid + i * 256;
            if (pc < WS::NHALO * 4) {
                uint4 hi, lo;
                split8(xreg[i][0], xreg[i][1], hi, lo);
                *reinterpret_cast<uint4*>(sXh + pc * 16) = hi;
                *reinterpret_cast<uint4*>(sXl + pc * 16) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < GP; ++i) {
            const int pc = tid + i * 256;
            uint4 hi, lo;
            split8(greg[i][0], greg[i][1], hi, lo);
            *reinterpret_cast<uint4*>(sGh + pc * 16) = hi;
            *reinterpret_cast<uint4*>(sGl + pc * 16) = lo;
            if (do_bias) {
                bs[0] += greg[i][0].x; bs[1] += greg[i][0].y; bs[2] += greg[i][0].z; bs[3] += greg[i][0].w;
                bs[4] += greg[i][1].x; bs[5] += greg[i][1].y; bs[6] += greg[i][1].z; bs[7] += greg[i][1].w;
            }
        }
    };

    auto step_off = [&](int s) { return wgrad_x_step_offset<WS>(s); };
    auto read_a = [&](int soff, int t, bf16x8& h, bf16x8& l) {
        const int o = a_off[t] + soff;
        h = tr_frag(sXh + o, sXh + o + 4 * 64);
        l = tr_frag(sXl + o, sXl + o + 4 * 64);
    };
    auto read_b = [&](int s, bf16x8& h, bf16x8& l) {
        const int o = (16 * s + 8 * kh + q) * 64 + col_off;
        h = tr_frag(sGh + o, sGh + o + 4 * 64);
        l = tr_frag(sGl + o, sGl + o + 4 * 64);
    };

    int brick = split;
    if (brick < nbricks) load_brick(brick);
    for (; brick < nbricks; brick += nsplit) {
        __syncthreads();
        store_brick();
        __syncthreads();
        if (brick + nsplit < nbricks) load_brick(brick + nsplit);  // in flight during the MFMA phase

        bf16x8 A0h[WS_TAPS], A0l[WS_TAPS], A1h[WS_TAPS], A1l[WS_TAPS], B0h, B0l, B1h, B1l;
#pragma unroll
        for (int t = 0; t < WS_TAPS; ++t) read_a(0, t, A0h[t], A0l[t]);
        read_b(0, B0h, B0l);
#pragma unroll 1
        for (int s2 = 0; s2 < WS_NSTEPS / 2; ++s2) {
            const int so = 2 * s2 + 1, sn = min(2 * s2 + 2, WS_NSTEPS - 1);
            const int off_o = step_off(so), off_n = step_off(sn);
            // term-major MFMA order: one wave per SIMD, so an MFMA that accumulates onto the result of the MFMA
            // right before it stalls ~12 cycles (tools/micro/mfma_peak: 1785 vs 2437 TFLOP/s); the three terms of a
            // tap are issued 7 MFMAs apart.  The next step's fragments are fetched during the first term.
#pragma unroll
            for (int t = 0; t < WS_TAPS; ++t) {  // even step: compute set 0, fetch set 1
                read_a(off_o, t, A1h[t], A1l[t]);
                if (t == 0) read_b(so, B1h, B1l);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0h[t], B0h, acc[t], 0, 0, 0);
                if (t == 0) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
                else __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
#pragma unroll
            for (int t = 0; t < WS_TAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0l[t], B0h, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < WS_TAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0h[t], B0l, acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * WS_TAPS, 0);
#pragma unroll
            for (int t = 0; t < WS_TAPS; ++t) {  // odd step: compute set 1, fetch set 0
                read_a(off_n, t, A0h[t], A0l[t]);
                if (t == 0) read_b(sn, B0h, B0l);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1h[t], B1h, acc[t], 0, 0, 0);
                if (t == 0) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
                else __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
#pragma unroll
            for (int t = 0; t < WS_TAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1l[t], B1h, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < WS_TAPS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1h[t], B1l, acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * WS_TAPS, 0);
        }
    }

    // ---- merge: D[row = ci][col = co]; lane holds col (lane & 31), rows (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const int r = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int t = 0; t < WS_TAPS; ++t) {
        const int ltap = wave + 4 * t;
        if (ltap < 27) {
            const int tap = wgrad_global_tap(gv, ltap);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ci = ci0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (ci >= Cin) continue;
                float* dst = &dwp[((int64_t)tap * Cin + ci) * Cout + co0 + r];
                if (slab_stride) dst[(int64_t)split * slab_stride] = acc[t][i];
                else atomicAdd(dst, acc[t][i]);
            }
        }
    }
    if (do_bias) {
        // threads with equal tid % 4 hold partial sums of the same 8 channels
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);  // [256][8]
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bs[e];
        __syncthreads();
        if (tid < 32) {
            const int q8 = tid >> 3, e = tid & 7;
            float t = 0.f;
            for (int k = q8; k < 256; k += 4) t += red[k * 8 + e];
            atomicAdd(&dbias[co0 + tid], t);
        }
    }
}

// The single-role kernel takes every supported call (grids that give every workgroup several bricks go to the producer /
// consumer form, which is asked first: conv3_wgrad_plan)
bool conv3_wgrad_mfma_split_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs) {
    if (!conv3_wgrad_mfma_split_supported(c.C1, c.C2, c.Cout)) return false;
    const int Cout = c.Cout;
    const int Cin = c.C1 + c.C2;
    WgradView g;
    const int order = conv3_wgrad_view_order(c, WS::BX, WS::BY, WS::BZ);
    const int nbricks = conv3_wgrad_view(g, c, WS::BX, WS::BY, WS::BZ, order);
    const int n_ci = (Cin + 31) / 32, n_co = Cout / 32;
    const int ntiles = n_ci * n_co;
    int nsplit = (256 + ntiles - 1) / ntiles;  // one workgroup per CU: one resident wave of workgroups
    if (nsplit > nbricks) nsplit = nbricks;
    if (nsplit < 1) nsplit = 1;
    p.kernel = TDX_WGRAD_SPLIT; p.nt = 1; p.depth = WS::BX; p.nbricks = nbricks; p.order = order;
    conv3_wgrad_plan_merge(p, nsplit, max_slabs);  // may lower nsplit (TDX_DETERMINISTIC)
    return true;
}

int conv3_wgrad_mfma_split_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p) {
    const int Cout = c.Cout;
    const int Cin = c.C1 + c.C2;
    WgradView g;
    conv3_wgrad_view(g, c, WS::BX, WS::BY, WS::BZ, p.order);
    const int n_ci = (Cin + 31) / 32, n_co = Cout / 32;
    const int ntiles = n_ci * n_co;
    const int nsplit = p.nsplit;
    int64_t slab_stride;
    float* out = conv3_wgrad_out(c, p, slab_stride);
    const size_t lds = (size_t)2 * WS::XBYTES + 2 * WS::GPLANE;
    dim3 grid((unsigned)(ntiles * nsplit));
    auto kern = conv3_wgrad_mfma_split_kernel;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, c.st, (const float*)c.x1, c.C1, (const float*)c.x2, c.C2, (const float*)c.dy, out,
                       c.dbias, g, Cout, nsplit, n_ci, slab_stride);
    return tdx_launch_status();
}
