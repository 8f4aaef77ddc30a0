// bf16 MFMA implicit-GEMM 3x3x3 convolution for gfx950 (forward and, with zero padding, the main
// term of the data gradient; its halo-shell term is tdx_conv3_shell.hip).
//
//   M = output voxels (a 256-voxel brick per workgroup), N = output channels (BN = 32/64 per
//   workgroup), K = 27 taps x input channels, walked in 16-channel slices.
//
// Per K slice the workgroup stages ONE halo'd input brick (6 x 10 x 10 voxels x 16 ch = 19 KB)
// and the slice's weights for all 27 taps (27 x BN x 16 = 54 KB at BN = 64) into LDS; every tap
// then re-reads the same brick at a shifted voxel offset, so the 27-fold input reuse of the
// convolution is served from LDS, not from L2/HBM.  78 KB of LDS per workgroup -> two
// workgroups per CU, one staging while the other issues MFMAs.
//
// Pipeline: the global loads of slice c+1 are issued into registers right after slice c has been
// written to LDS and stay in flight during the 27 x 2 x NT MFMAs of slice c (the wait lands at
// the next LDS write); inside a slice the fragments of tap t+1 are read while the MFMAs of tap t
// issue (pinned with sched_group_barrier).
//
// Wave w owns an 8 x 8 (y, z) slab of the brick = two 32-voxel M tiles (r <-> y = 4*mt + (r & 3),
// z = r >> 2) x NT 32-channel N tiles.  The MFMA is issued as D^T = W^T X^T (weights as the A
// operand), so a lane owns ONE voxel and 4 consecutive channels per accumulator quad: the
// epilogue packs them to 8-B writes of an LDS output tile [256 voxels][BN] that is then stored to
// HBM in whole 16-B-per-lane voxel rows (+ fused GroupNorm moments, + fused residual addend for
// the data gradient).
//
// LDS images, each split in two half-planes (channels 0-7 / 8-15 of the slice) of 16-B entries:
//   brick  : [half][voxel h = (hx*HY + hy)*SZ + hz]; with the main shape's z stride padded
//            10 -> 12 the 16 voxels of every ds_read_b128 lane group are distinct mod 16, i.e.
//            conflict-free with plain affine addresses (tap offsets are instruction immediates;
//            found by exhaustive enumeration of lane groups x tap offsets)
//   weights: [half][tap*BN + n]
//
// Brick shapes (tdx_conv3_brick.h: Brick<SHAPE>, BrickView, up to three regions per launch).  The main
// shape is 4 x 8 x 8 (wave = x plane).  Grids whose extent leaves a remainder of 1-2 voxels along an
// axis -- the reference's real 194 x 50 x 50 grids -- would waste a whole row of mostly empty bricks
// per such axis (+34 % bricks at 194 x 66 x 50), so those remainder slabs are tiled with a thin
// 2 x 16 x 8 brick (XT: wave = (x plane, y half)), with the kernel's local axes permuted so that
// its thin axis is the slab's thin axis.
//
// Measured alternatives that lost (kept out of the build): an 8 x 8 x 8 brick with a 128 x 64
// register tile per wave and one workgroup per CU (-5...-30 %), and a ping-pong-LDS single
// workgroup per CU with one barrier per slice (700 vs 840 TFLOP/s): with this much LDS traffic
// per MFMA, two co-resident workgroups hide more than a deeper pipeline in one.
#include "tdx_common.h"
#include "tdx_conv3.h"
#include "tdx_conv3_epilogue.h"

#define M3_KC 16

bool conv3_mfma_supported(int C1, int C2, int Cout) {
    return C1 > 0 && (C1 % M3_KC) == 0 && (C2 % M3_KC) == 0 && (Cout % 32) == 0;
}

// EXT: strided inputs (row strides ld1 / ld2 >= C1 / C2) and the `init` tensor of tdx_conv3_fwd_partial (init_batch:
// voxels between its samples, 0 = shared by the batch); a separate instantiation, the only one that reads those
// arguments, so that the hot kernels carry none of it (it cost the 32-channel layers 7-19 %)
// HF: the operand format (H16<HF>: bf16 or fp16 words behind the bf16-typed pointers)
template <int NT, bool XT, bool ZERO_PAD, bool PERM, bool EXT, bool HF>
__global__ void __launch_bounds__(256, 2)
conv3_mfma_kernel(const bf16* __restrict__ x1, int C1, const bf16* __restrict__ x2, int C2,
                  const bf16* __restrict__ wp, const float* __restrict__ bias, bf16* __restrict__ y, BrickRegions R,
                  int Cout, double* __restrict__ gn_acc, bf16* __restrict__ d1, int D1, bf16* __restrict__ d2,
                  const bf16* __restrict__ a1, const bf16* __restrict__ a2, const bf16* __restrict__ init, int ld1, int ld2,
                  int init_batch) {
    typedef H16<HF> H;
    typedef typename H::T HT;
    using BR = Brick<XT ? BRICK_THIN : BRICK_MAIN>;
    constexpr bool LOCAL = XT || PERM;                  // local axes differ from the grid's (thin bricks always run permuted)
    constexpr int BN = NT * 32;
    constexpr int HX = BR::HX, HY = BR::HY, HZ = BR::HZ;
    constexpr int SZ = XT ? 10 : BR::SZ;                // z stride of the LDS brick: padded for the main shape only
    constexpr int NHALO = BR::NHALO;                    // 600 / 720 staged voxels
    constexpr int APLANE = HX * HY * SZ * 16 + 64;      // +64 B: the two halves of a voxel land 4 slots apart
    constexpr int BRICK_BYTES = 2 * APLANE;
    constexpr int B_PLANE = 27 * BN * 16 + 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;
    unsigned char* sB = smem + BRICK_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;

    // block -> region -> (b, brick); neighbouring bricks share an XCD's L2 (halo reuse)
    int b, o[3];
    const BrickView& g = brick_decode<XT ? BRICK_THIN : BRICK_MAIN>(R, xcd_contiguous((int)blockIdx.x, (int)gridDim.x), b, o);
    const int n0 = blockIdx.y * BN;
    const int Cin = C1 + C2;

    // ---- staging plan for the input brick: 2 * NHALO 16-B pieces, 5-6 per thread.
    // a_src: (voxel index in the sample's input grid) * 2 + half, or -1 for zero fill / no piece
    constexpr int A_PIECES = NHALO * 2;
    constexpr int A_PER_THREAD = (A_PIECES + 255) / 256;
    constexpr int B_PIECES = 27 * BN * 2;
    constexpr int B_PER_THREAD = (B_PIECES + 255) / 256;  // 14 (NT=2) / 7 (NT=1)
    int a_src[A_PER_THREAD];
    int a_dst[A_PER_THREAD];
#pragma unroll
    for (int i = 0; i < A_PER_THREAD; ++i) {
        const int p = tid + i * 256;
        a_dst[i] = -1;
        a_src[i] = -1;
        if (p < A_PIECES) {
            // lanes 0-3 / 4-7 of every 8-lane group: 4 consecutive voxels x the two halves
            const int hv = ((p >> 3) << 2) + (p & 3), half = (p >> 2) & 1;
            const int hx = hv / (HY * HZ), rem = hv - hx * (HY * HZ);
            const int hy = rem / HZ, hz = rem - hy * HZ;
            a_dst[i] = half * APLANE + ((hx * HY + hy) * SZ + hz) * 16;
            const int src = brick_halo_source<ZERO_PAD, LOCAL>(g, o, hx, hy, hz);
            if (src >= 0) a_src[i] = src * 2 + half;
        }
    }
    const int64_t batch_vox = (int64_t)b * g.Ei[0] * g.Ei[1] * g.Ei[2];

    // weight staging role of this thread: (row = b_row0 + 128 i, half); 128 rows = 128/BN taps per
    // step, so both the global and the LDS address advance by a constant per i
    const int b_half = (tid >> 2) & 1;
    const int b_row0 = ((tid >> 3) << 2) + (tid & 3);                             // 0..127
    const int b_goff = ((b_row0 / BN) * Cout + (b_row0 % BN)) * 16 + b_half * 8;  // elements
    const int b_dst = b_half * B_PLANE + b_row0 * 16;

    uint4 areg[A_PER_THREAD], breg[B_PER_THREAD];
    auto load_slice = [&](int c) {
        const int k0 = c * M3_KC;
        const bf16* xs;
        int Cs, kk;
        if (k0 < C1) { xs = x1; Cs = EXT ? ld1 : C1; kk = k0; } else { xs = x2; Cs = EXT ? ld2 : C2; kk = k0 - C1; }
        xs += batch_vox * Cs + kk;
#pragma unroll
        for (int i = 0; i < A_PER_THREAD; ++i) {
            areg[i] = make_uint4(0, 0, 0, 0);
            if (a_src[i] >= 0)
                areg[i] = *reinterpret_cast<const uint4*>(xs + (int64_t)(a_src[i] >> 1) * Cs + (a_src[i] & 1) * 8);
        }
        const bf16* wc = wp + (int64_t)c * 27 * Cout * 16 + (int64_t)n0 * 16 + b_goff;
#pragma unroll
        for (int i = 0; i < B_PER_THREAD; ++i) {
            breg[i] = make_uint4(0, 0, 0, 0);
            if (b_row0 + 128 * i < 27 * BN)
                breg[i] = *reinterpret_cast<const uint4*>(wc + (int64_t)i * (128 / BN) * Cout * 16);
        }
    };
    auto store_slice = [&]() {
#pragma unroll
        for (int i = 0; i < A_PER_THREAD; ++i)
            if (a_dst[i] >= 0) *reinterpret_cast<uint4*>(sA + a_dst[i]) = areg[i];
#pragma unroll
        for (int i = 0; i < B_PER_THREAD; ++i)
            if (b_row0 + 128 * i < 27 * BN) *reinterpret_cast<uint4*>(sB + b_dst + i * 2048) = breg[i];
    };

    // ---- per-lane fragment bases: this lane's voxel of M tile mt (Brick<>::lane_voxel: wave w owns a brick plane and 8 y
    // rows of it, y = 4 mt + (r & 3), z = r >> 2)
    int a_h[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int lx, ly, lz;
        BR::lane_voxel(wave, mt, r, lx, ly, lz);
        a_h[mt] = ((lx + 1) * HY + (ly + 1)) * SZ + (lz + 1);
    }
    int b_off[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_off[nt] = hh * B_PLANE + (nt * 32 + r) * 16;

    f32x16 acc[NT][2];  // D[row = channel][col = voxel]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][mt][i] = 0.f;

    const int nchunks = Cin / M3_KC;
    load_slice(0);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();  // previous slice's fragment reads are done
        store_slice();
        __syncthreads();
        if (c + 1 < nchunks) load_slice(c + 1);  // in flight during the MFMAs below

        // fragments of tap t+1 are read while the MFMAs of tap t issue (two register sets)
        bf16x8 xf[2][2], wf[2][NT];
        auto read_frags = [&](int tap, int buf) {
            const int ex = tap / 9 - 1, ey = (tap / 3) % 3 - 1, ez = tap % 3 - 1;
            const int toff = (ex * HY + ey) * SZ + ez;
            // the weight tap is indexed in GLOBAL axes; thin bricks run on permuted local axes
            const int wtap = LOCAL ? brick_tap(g, ex, ey, ez) : tap;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                xf[buf][mt] = *reinterpret_cast<const bf16x8*>(sA + hh * APLANE + (a_h[mt] + toff) * 16);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                wf[buf][nt] = *reinterpret_cast<const bf16x8*>(sB + wtap * (BN * 16) + b_off[nt]);
        };
        read_frags(0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2 + NT, 0);  // DS_READ: tap 0's fragments
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            if (tap + 1 < 27) read_frags(tap + 1, (tap + 1) & 1);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[nt][mt] = H::mfma(wf[tap & 1][nt], xf[tap & 1][mt], acc[nt][mt]);
            // pin the interleave: one fragment read of tap+1 behind each MFMA of tap
            if (tap + 1 < 27) {
#pragma unroll
                for (int k = 0; k < 2 * NT; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
                    if (k < 2 + NT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS_READ
                }
            } else {
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NT, 0);
            }
        }
    }

    // ---------------- epilogue.  Lane (r, hh) of wave w holds, for M tile mt, the voxel lane_voxel(w, mt, r) and channels
    // nt*32 + 8 j + 4 hh + (0..3) in accumulator registers 4 j .. 4 j + 3.  Tile voxel index v = (x*BY + y)*8 + z.
    __syncthreads();
    unsigned char* sO = smem;  // [256 voxels][BN] 16-bit
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = nt * 32 + 8 * j + 4 * hh;
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            if (bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[e] = bias[n0 + ch + e];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                int lx, ly, lz;
                BR::lane_voxel(wave, mt, r, lx, ly, lz);
                const int v = BR::tile_index(lx, ly, lz);
                const unsigned lo = H::pack2(acc[nt][mt][4 * j] + bv[0], acc[nt][mt][4 * j + 1] + bv[1]);
                const unsigned hi = H::pack2(acc[nt][mt][4 * j + 2] + bv[2], acc[nt][mt][4 * j + 3] + bv[3]);
                *reinterpret_cast<uint2*>(sO + conv3_tile_addr16<BN>(v, ch >> 3) + (ch & 7) * 2) = make_uint2(lo, hi);
            }
        }
    __syncthreads();
    // store loop: thread -> 16-B chunk (tid % CHUNKS) of voxels tid / CHUNKS + (256 / CHUNKS) i: whole voxel rows to y
    // (+ the fused GroupNorm moments from the same registers), or to dx (ZERO_PAD)
    constexpr int CHUNKS = BN / 8;
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        const int p = tid + i * 256;
        const int v = p / CHUNKS, cidx = p % CHUNKS;
        int lx, ly, lz, vox;
        BR::tile_voxel(v, lx, ly, lz);
        if (brick_out_voxel<LOCAL>(g, o, lx, ly, lz, vox)) {
            const int64_t ov = (int64_t)b * g.Eo[0] * g.Eo[1] * g.Eo[2] + vox;
            uint4 val = *reinterpret_cast<const uint4*>(sO + conv3_tile_addr16<BN>(v, cidx));
            if (ZERO_PAD) {
                conv3_store_dx<HT>(val, ov, n0 + cidx * 8, Cout, d1, D1, d2, a1, a2);
            } else {
                if (EXT && init != nullptr) {
                    // continue from a precomputed partial convolution ([B or 1][voxels][Cout]), added in the coalesced
                    // store loop; the statistics below see the sum
                    const int64_t iv = (int64_t)b * init_batch + vox;
                    Vec8<HT> va, vb;
                    va.load(reinterpret_cast<const HT*>(&val));
                    vb.load(reinterpret_cast<const HT*>(init + iv * Cout + n0 + cidx * 8));
#pragma unroll
                    for (int e = 0; e < 8; ++e) va.v[e] += vb.v[e];
                    va.store(reinterpret_cast<HT*>(&val));
                }
                *reinterpret_cast<uint4*>(y + ov * Cout + n0 + cidx * 8) = val;
                if (gn_acc != nullptr) conv3_moments_add<H>(val, s1, s2);
            }
        }
    }
    if (!ZERO_PAD && gn_acc != nullptr)
        conv3_moments_merge<BN, 8>(s1, s2, reinterpret_cast<float*>(smem + 256 * BN * 2), gn_acc, g.B, b, Cout, n0);
}

template <int NT, bool XT, bool ZP, bool PERM, bool EXT, bool HF>
static int mfma_go(const Conv3Call& c, const BrickRegions& reg) {
    constexpr int BN = NT * 32;
    using BR = Brick<XT ? BRICK_THIN : BRICK_MAIN>;
    const size_t lds = (size_t)2 * (BR::HX * BR::HY * (XT ? 10 : BR::SZ) * 16 + 64) + (size_t)27 * BN * 32 + 128;
    const Conv3Ext none = {0, 0, nullptr, false};
    if (!brick_closed(reg)) return TDX_EINVAL;
    const Conv3Ext& x = EXT ? *c.ext : none;
    return tdx_launch_lds<conv3_mfma_kernel<NT, XT, ZP, PERM, EXT, HF>>(
        dim3((unsigned)reg.start[reg.n], c.N / BN), dim3(256), lds, c.st, (const bf16*)c.x1, c.C1, (const bf16*)c.x2, c.C2,
        (const bf16*)c.wp, c.bias, (bf16*)c.y, reg, c.N, c.gn_acc, (bf16*)c.d1, c.D1, (bf16*)c.d2, (const bf16*)c.a1,
        (const bf16*)c.a2, (const bf16*)x.init, x.ld1 ? x.ld1 : c.C1, x.ld2 ? x.ld2 : c.C2,
        x.init && !x.init_shared ? c.X * c.Y * c.Z : 0);
}

// The 16-bit kernel's planning rule (the fp32 kernels': brick_plan).  An axis whose extent leaves a remainder of 1-2 voxels
// gets a thin slab instead of a row of mostly empty main bricks, in the forward as in the data gradient, on grids of
// 60000 voxels and more (measured: pays on the two finest U-Net levels, loses to the extra launch below ~50k voxels) or
// under TDX_CONV3_THIN=2; the slabs' permutations are fixed; the main bricks' short edge goes to the axis that leaves the
// fewest bricks over the MAIN extents (48 x 16 x 12: 36 bricks with the 4 along z instead of 48).  slabs_beyond: the main
// region is another kernel's (the ring kernel's); only the slabs beyond it.  Strided input / init tensor (ext): main bricks
// in grid orientation only.  false: not a call for this kernel.
static bool mfma_plan(const Conv3Call& c, BrickRegions& main, BrickRegions& thin) {
    static const int cand[3][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}};  // which global axis gets the short (4 / 2) edge
    const Conv3Geom g = c.geom();
    const int Eo[3] = {g.Xo, g.Yo, g.Zo}, bdim[3] = {4, 8, 8};
    const int mode = conv3_thin_slabs();
    const bool big = mode == 2 || (int64_t)g.Xo * g.Yo * g.Zo >= 60000;
    int Em[3];  // extent of the main region
    bool slab[3];
    for (int a = 0; a < 3; ++a) {
        const int rem = Eo[a] % bdim[a];
        slab[a] = mode != 0 && rem >= 1 && rem <= 2 && Eo[a] > bdim[a] && big && c.ext == nullptr;
        Em[a] = slab[a] ? Eo[a] - rem : Eo[a];
        if (c.slabs_beyond != nullptr) {
            const int m = c.slabs_beyond[a];
            if (c.ext != nullptr || m <= 0 || Eo[a] - m > 2 || Eo[a] < m) return false;
            Em[a] = m;
            slab[a] = m < Eo[a];
        }
    }
    int mperm = 0;
    if (conv3_perm_bricks() && c.ext == nullptr) {
        int64_t best = -1;
        for (int k = 0; k < 3; ++k) {
            const int64_t n = brick_count(Em, cand[k], BRICK_MAIN);
            if (best < 0 || n < best) { best = n; mperm = k; }
        }
    }
    const int org0[3] = {0, 0, 0};
    main.n = c.slabs_beyond ? 0 : 1;
    brick_fill_view(main.v[0], g, cand[mperm], org0, Em, BRICK_MAIN);
    main.start[0] = 0;
    brick_close(main, (int)((int64_t)g.B * main.v[0].nb[0] * main.v[0].nb[1] * main.v[0].nb[2]));
    // remainder slabs, all in ONE launch of the thin-brick kernel (each has too few workgroups to fill the chip alone):
    //   x slab: [Em_x, Xo) x all y x all z     (local axes x, y, z)
    //   y slab: main x range x [Em_y, Yo) x all z  (local axes y, x, z)
    //   z slab: main x, y ranges x [Em_z, Zo)   (local axes z, x, y)
    thin.n = 0;
    int nblk = 0;
    for (int a = 0; a < 3; ++a) {
        if (!slab[a]) continue;
        int org[3], ext[3];
        for (int k = 0; k < 3; ++k) { org[k] = 0; ext[k] = k < a ? Em[k] : Eo[k]; }
        org[a] = Em[a]; ext[a] = Eo[a] - Em[a];
        BrickView& v = thin.v[thin.n];
        brick_fill_view(v, g, cand[a], org, ext, BRICK_THIN);
        thin.start[thin.n++] = nblk;
        nblk += (int)((int64_t)g.B * v.nb[0] * v.nb[1] * v.nb[2]);
    }
    brick_close(thin, nblk);
    return true;
}

int conv3_mfma_launch(const Conv3Call& c) {
    if (!tdx_is_h16(c.fmt) || (c.zero_pad && c.d1 == nullptr)) return TDX_EINVAL;
    if ((int64_t)c.X * c.Y * c.Z * 2 >= (1ll << 31)) return TDX_ESHAPE;
    BrickRegions main, thin;
    if (!mfma_plan(c, main, thin)) return TDX_ESHAPE;
    int rc = TDX_OK;
    if (c.ext != nullptr) {  // strided input / init tensor: forward, main bricks in grid orientation (what mfma_plan gave it)
        if (c.zero_pad) return TDX_ESHAPE;
        TDX_DISPATCH_BOOL(c.N % 64 == 0, WIDE, TDX_DISPATCH_H16(c.hf(),
            rc = mfma_go<WIDE ? 2 : 1, false, false, false, true, HF>(c, main)));
        return rc;
    }
    if (main.n > 0)
        TDX_DISPATCH_BOOL(c.N % 64 == 0, WIDE, TDX_DISPATCH_BOOL(c.zero_pad, ZP, TDX_DISPATCH_BOOL(main.v[0].perm[0] != 0, PM,
            TDX_DISPATCH_H16(c.hf(), rc = mfma_go<WIDE ? 2 : 1, false, ZP, PM, false, HF>(c, main)))));
    if (rc != TDX_OK || thin.n == 0) return rc;
    TDX_DISPATCH_BOOL(c.N % 64 == 0, WIDE, TDX_DISPATCH_BOOL(c.zero_pad, ZP, TDX_DISPATCH_H16(c.hf(),
        rc = mfma_go<WIDE ? 2 : 1, true, ZP, false, false, HF>(c, thin))));
    return rc;
}
