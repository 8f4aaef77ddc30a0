// Split-precision ("bf16x2") MFMA weight gradient of the replicate-padded 3x3x3 convolution for fp32 tensors, producer /
// consumer form (gfx950): 8 computing + 4 loader waves per workgroup, one workgroup per CU.
//
//   dW[tap][ci][co] = sum_v x[clamp(v + tap)][ci] * dy[v][co]  ~=  sum_v  xh * dyh + xl * dyh + xh * dyl
//
// The single-role kernel (tdx_conv3_wgrad_mfma_split.hip) lets one wave per SIMD load, split, store and multiply in turn:
// its matrix pipe is busy 52 % of the cycles, and with the re-staging removed 73 % (profiles/r12_split_staging_ablation.txt,
// section 5).  This kernel is tdx_conv3_wgrad_ring.hip's 32-wide form with split operands:
//   * a workgroup owns a 32 (ci) x 32 (co) tile of all 27 taps and walks 2 x 8 x 8 bricks (half the single-role kernel's:
//     hi + lo images of the halo'd x brick and of the dy brick are 67 KB, so that TWO sets fit the LDS);
//   * the 4 LOADER waves stage brick i + 1 into the other set while brick i is multiplied: global -> registers -> hi / lo
//     (bf16(v), bf16(v - hi)) -> LDS, zero rows for voxels beyond a ragged grid and channels beyond a half-filled ci tile
//     written from registers (no zero source needed); ONE barrier per brick;
//   * the 8 COMPUTING waves own 4 / 4 / 4 / 3 / 3 / 3 / 3 / 3 taps (7 x 3 MFMAs per SIMD and K step of 16 voxels); the three
//     terms of a tap are issued back to back on its accumulator (the SIMD's other computing wave fills the dependent-issue
//     stall), then the tap's x fragments are re-read for the next step; wave 7's spare slot multiplies ones with dy_hi and
//     dy_lo: the bias gradient.
// Same contract as the single-role kernel; conv3_wgrad_split_ring_plan says when a call is a case for it (enough bricks per workgroup).
#include "tdx_conv3_wgrad.h"
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

typedef WgradBrick<2> SR;                              // 2 x 8 x 8 bricks: 128 voxels, 400 halo'd; 64-B rows (32 bf16 channels)
#define SR_NSTEPS (SR::NVOX / 16)                      // 8 K steps of 16 voxels
#define SR_SET (2 * SR::XBYTES + 2 * SR::GPLANE)       // hi and lo image of the x brick and of the dy brick: 67 584 B
#define SR_CW 8                                        // computing waves
#define SR_LT 256                                      // loader threads

__global__ void __launch_bounds__(768, 3)
conv3_wgrad_split_ring_kernel(const float* __restrict__ x1, int C1, const float* __restrict__ x2, int C2,
                              const float* __restrict__ dy, float* __restrict__ dwp, float* __restrict__ dbias,
                              WgradView gv, int Cout, int nsplit, int n_ci_tiles, int64_t slab_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [2 sets][x hi | x lo | dy hi | dy lo]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cin = C1 + C2;
    const int tile = blockIdx.x / nsplit, split = blockIdx.x - tile * nsplit;
    const int ci0 = (tile % n_ci_tiles) * 32, co0 = (tile / n_ci_tiles) * 32;
    const int nbricks = gv.B * gv.nb[0] * gv.nb[1] * gv.nb[2];

    if (wave >= SR_CW) {
        // =========================================================== loader waves
        const int lt = tid - SR_CW * 64;
        const float* xs;
        int Cs, cbase;
        if (ci0 < C1) { xs = x1; Cs = C1; cbase = ci0; } else { xs = x2; Cs = C2; cbase = ci0 - C1; }
        constexpr int XP = (SR::NHALO * 4 + SR_LT - 1) / SR_LT;  // pieces (halo voxel, 8 fp32 channels) per thread: 7
        constexpr int GP = (SR::NVOX * 4) / SR_LT;                // 2
        int xh[XP];  // hx | hy << 8 | hz << 16 | channels exist << 30
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int pc = lt + i * SR_LT;
            const int hv = min(pc >> 2, SR::NHALO - 1), q4 = pc & 3;
            int hx, hy, hz;
            SR::halo_coords(hv, hx, hy, hz);
            xh[i] = hx | (hy << 8) | (hz << 16) | ((cbase + q4 * 8 < Cs) ? (1 << 30) : 0);
        }
        auto stage = [&](int brick, int set) {
            int bx, by, bz;
            const int bb = wgrad_brick_coords(gv, brick, bx, by, bz);
            float4 xr[XP][2], gr[GP][2];
#pragma unroll
            for (int i = 0; i < XP; ++i) {
                const int pc = lt + i * SR_LT;
                xr[i][0] = xr[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pc < SR::NHALO * 4 && ((xh[i] >> 30) & 1)) {
                    const int64_t vox = SR::halo_source(gv, bb, bx, by, bz, xh[i] & 0xff, (xh[i] >> 8) & 0xff, (xh[i] >> 16) & 0xff);
                    const float4* src = reinterpret_cast<const float4*>(xs + vox * Cs + cbase + (pc & 3) * 8);
                    xr[i][0] = src[0];
                    xr[i][1] = src[1];
                }
            }
#pragma unroll
            for (int i = 0; i < GP; ++i) {
                const int pc = lt + i * SR_LT;
                const int v = pc >> 2, q8 = pc & 3;
                const int vx = bx * SR::BX + (v >> 6), vy = by * SR::BY + ((v >> 3) & 7), vz = bz * SR::BZ + (v & 7);
                gr[i][0] = gr[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (vx < gv.E[0] && vy < gv.E[1] && vz < gv.E[2]) {
                    const int64_t vox = wgrad_voxel(gv, bb, vx, vy, vz);
                    const float4* src = reinterpret_cast<const float4*>(dy + vox * Cout + co0 + q8 * 8);
                    gr[i][0] = src[0];
                    gr[i][1] = src[1];
                }
            }
            unsigned char* sX = smem + set * SR_SET;
            unsigned char* sG = sX + 2 * SR::XBYTES;
#pragma unroll
            for (int i = 0; i < XP; ++i) {
                const int pc = lt + i * SR_LT;
                if (pc < SR::NHALO * 4) {
                    uint4 hi, lo;
                    split8(xr[i][0], xr[i][1], hi, lo);
                    *reinterpret_cast<uint4*>(sX + pc * 16) = hi;
                    *reinterpret_cast<uint4*>(sX + SR::XBYTES + pc * 16) = lo;
                }
            }
#pragma unroll
            for (int i = 0; i < GP; ++i) {
                const int pc = lt + i * SR_LT;
                uint4 hi, lo;
                split8(gr[i][0], gr[i][1], hi, lo);
                *reinterpret_cast<uint4*>(sG + pc * 16) = hi;
                *reinterpret_cast<uint4*>(sG + SR::GPLANE + pc * 16) = lo;
            }
        };
        int brick = split, it = 0;
        if (brick < nbricks) stage(brick, 0);
        for (; brick < nbricks; brick += nsplit, ++it) {
            vmem_lds_barrier();  // brick `it` is staged, the computing waves are done with brick it - 1
            if (brick + nsplit < nbricks) stage(brick + nsplit, (it + 1) & 1);
        }
        return;
    }

    // =============================================================== computing waves
    // waves 0-2 own 4 taps, waves 3-7 own 3 (27 = 3 x 4 + 5 x 3); wave 7's fourth slot sums the bias gradient
    const int first = wave < 3 ? 4 * wave : 12 + 3 * (wave - 3);
    const int cnt = wave < 3 ? 4 : 3;
    const bool bias_slot = wave == 7;

    const WgradLane L = wgrad_lane(lane);  // fragment lane geometry
    const int q = L.q, kh = L.kh, col_off = L.col_off;
    int a_off[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        a_off[t] = wgrad_x_frag_row<SR>(L, SR::tap_offset(min(first + t, 26))) * 64 + col_off;
    }
    const int b_row = (8 * kh + q) * 64 + col_off;

    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    // specialised at compile time on whether the wave's fourth slot is in use; the K-step loop stays rolled, two steps per
    // trip (dy fragment sets by step parity)
    auto run = [&](auto fourth_c) {
        constexpr bool FOURTH = decltype(fourth_c)::value;
        int it = 0;
        for (int brick = split; brick < nbricks; brick += nsplit, ++it) {
            vmem_lds_barrier();
            const unsigned char* bX = smem + (it & 1) * SR_SET;
            const unsigned char* bG = bX + 2 * SR::XBYTES + b_row;
            auto step_off = [&](int s) { return wgrad_x_step_offset<SR>(s); };
            auto read_a = [&](int s, int t, bf16x8& h, bf16x8& l) {
                const unsigned char* ap = bX + a_off[t] + step_off(s);
                h = tr_frag(ap, ap + 4 * 64);
                l = tr_frag(ap + SR::XBYTES, ap + SR::XBYTES + 4 * 64);
            };
            auto read_b = [&](int s, bf16x8& h, bf16x8& l) {
                const unsigned char* bp = bG + s * (16 * 64);
                h = tr_frag(bp, bp + 4 * 64);
                l = tr_frag(bp + SR::GPLANE, bp + SR::GPLANE + 4 * 64);
            };
            bf16x8 Ah[4], Al[4], Bh[2], Bl[2];
#pragma unroll
            for (int t = 0; t < 4; ++t) read_a(0, t, Ah[t], Al[t]);
            read_b(0, Bh[0], Bl[0]);

            auto step = [&](int s, int cur) {
                const int sn = min(s + 1, SR_NSTEPS - 1), nx = cur ^ 1;
                read_b(sn, Bh[nx], Bl[nx]);
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah[t], Bh[cur], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al[t], Bh[cur], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah[t], Bl[cur], acc[t], 0, 0, 0);
                    read_a(sn, t, Ah[t], Al[t]);
                    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                }
                if (FOURTH) {  // the fourth tap (waves 0-2) or the bias column sums (wave 7: ones x (dy_hi + dy_lo))
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bias_slot ? ones : Ah[3], Bh[cur], acc[3], 0, 0, 0);
                    if (!bias_slot) acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al[3], Bh[cur], acc[3], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bias_slot ? ones : Ah[3], Bl[cur], acc[3], 0, 0, 0);
                    if (!bias_slot) read_a(sn, 3, Ah[3], Al[3]);
                }
            };
#pragma unroll 1
            for (int s2 = 0; s2 < SR_NSTEPS / 2; ++s2) {
                step(2 * s2, 0);
                step(2 * s2 + 1, 1);
            }
        }
    };
    if (cnt == 4 || bias_slot) run(std::true_type{}); else run(std::false_type{});

    // ---- merge: D[row = ci][col = co]; lane holds col (lane & 31), rows (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const int r = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ltap = first + i;
        if (i < cnt) {
            const int tap = wgrad_global_tap(gv, ltap);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = ci0 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                if (ci >= Cin) continue;  // half-filled last tile
                float* dst = &dwp[((int64_t)tap * Cin + ci) * Cout + co0 + r];
                if (slab_stride) dst[(int64_t)split * slab_stride] = acc[i][e];
                else atomicAdd(dst, acc[i][e]);
            }
        } else if (bias_slot && i == 3 && dbias != nullptr && ci0 == 0 && hh == 0) {
            atomicAdd(&dbias[co0 + r], acc[i][0]);
        }
    }
}

bool conv3_wgrad_split_ring_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs) {
    const int Cout = c.Cout;
    if (tdx_switch(SW_WGRAD_SPLIT_RING) == 0) return false;  // A/B switch
    if (!conv3_wgrad_mfma_split_supported(c.C1, c.C2, Cout)) return false;
    const int Cin = c.C1 + c.C2;
    // local axes: brick 2 x 8 x 8; the short axis goes where it leaves the fewest bricks
    WgradView g;
    const int order = conv3_wgrad_view_order(c, SR::BX, SR::BY, SR::BZ);
    const int nbricks = conv3_wgrad_view(g, c, SR::BX, SR::BY, SR::BZ, order);
    const int n_ci = (Cin + 31) / 32, n_co = Cout / 32;
    const int ntiles = n_ci * n_co;
    const int cus = tdx_persistent_cus();
    int nsplit = cus >= 256 ? (256 + ntiles - 1) / ntiles : std::max(cus / ntiles, 1);  // one workgroup per CU (at most `cus`)
    if (nsplit > nbricks) nsplit = nbricks;
    if (nsplit < 1) nsplit = 1;
    // a workgroup should walk several bricks, or the double buffering has nothing to overlap
    if (nbricks < 4 * nsplit) return false;
    p.kernel = TDX_WGRAD_SPLIT_RING; p.nt = 1; p.depth = SR::BX; p.nbricks = nbricks; p.order = order;
    conv3_wgrad_plan_merge(p, nsplit, max_slabs);  // may lower nsplit (TDX_DETERMINISTIC)
    return true;
}

int conv3_wgrad_split_ring_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p) {
    const int Cout = c.Cout;
    const int Cin = c.C1 + c.C2;
    WgradView g;
    conv3_wgrad_view(g, c, SR::BX, SR::BY, SR::BZ, p.order);
    const int n_ci = (Cin + 31) / 32, n_co = Cout / 32;
    const int ntiles = n_ci * n_co;
    const int nsplit = p.nsplit;
    const size_t lds = (size_t)2 * SR_SET;
    int64_t slab_stride;
    float* out = conv3_wgrad_out(c, p, slab_stride);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)conv3_wgrad_split_ring_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    hipLaunchKernelGGL(conv3_wgrad_split_ring_kernel, dim3((unsigned)(ntiles * nsplit)), dim3(768), lds, c.st, (const float*)c.x1, c.C1,
                       (const float*)c.x2, c.C2, (const float*)c.dy, out, c.dbias, g, Cout, nsplit, n_ci, slab_stride);
    return tdx_launch_status();
}
