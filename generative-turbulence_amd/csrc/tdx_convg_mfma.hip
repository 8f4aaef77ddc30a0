// Matrix-core kernels of the general 3-D convolution family (the vector-ALU kernels and the layer list
// are in tdx_convg.hip), gfx950, bf16 tensors with fp32 accumulation:
//   convg_mfma_kernel<TRANSPOSED, NT, EPI>  gather / scatter^T   = forward and data gradient of the dilated (dilresnet.py:22-38),
//                                        strided (tfnet.py:185-199) and transposed (tfnet.py:201-208) convolutions
//   convg_wgrad_mfma_kernel              their weight gradients
// Same entry points, same operands as the vector-ALU kernels (weights [taps][Cin][Cout] fp32): tdx_convg_apply and
// tdx_convg_bwd_weight route bf16 tensors here.
//
// These layers have no brick structure to exploit (dilation 8 spreads the 27 taps over a 17^3 neighbourhood; stride 2 reads
// every 8th voxel), so the input operand is NOT staged: an MFMA B fragment of v_mfma_f32_32x32x16_bf16 is 8 consecutive
// channels of one voxel = one 16-B global load per lane straight from the NDHWC row of the tap's source voxel (rows of
// neighbouring taps are served by L1 / L2).  Only the weights go through LDS: per (tap, <= 128-channel slice) the fp32
// [ci][co] block is converted to bf16 and laid out as fragments, double-buffered, one barrier per stage.  The accumulator
// rows are channels in a permuted order so that a lane ends up with 16 consecutive channels of its voxel (two 16-B stores).
//
// scatter^T with stride s (transposed conv forward, strided conv data gradient): an output voxel o only receives the taps
// with (o + pad - t dil) divisible by s along every axis.  Workgroups therefore own voxels of ONE residue class o mod s, the
// divisibility test is uniform per workgroup and the dead taps (7 of 8 at stride 2) are skipped, not masked.
#include "tdx_common.h"
#include "tdx_convg.h"
#include "tdx_mfma.h"

#define CGM_KCH 128   // channels per weight stage

// the accumulator row rho = 8 j + 4 hh + i (register 4 j + i of lane half hh) holds channel 16 hh + 4 j + i
__device__ __forceinline__ int cgm_row_channel(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }

// EPI: the fused epilogues of the DilResNet chain (TdxConvgEpilogue, include/tdx.h; tdx_convg_chain.hip); EPI = false is the
// plain `acc + bias` store of tdx_convg_apply
template <bool TRANSPOSED, int NT, bool EPI>
__global__ void __launch_bounds__(256, 2)
convg_mfma_kernel(const bf16* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, bf16* __restrict__ out,
                  ConvG g, TdxConvgEpilogue e) {
    constexpr int BN = 32 * NT;
    constexpr int WBUF = (CGM_KCH / 8) * BN * 16;  // one weight stage: [k group][channel][8] bf16
    __shared__ __attribute__((aligned(16))) unsigned char sW[2 * WBUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int cls = blockIdx.x / g.cls_blocks, blk = blockIdx.x - cls * g.cls_blocks;
    const int n0 = blockIdx.y * BN;
    const int cs = g.cs;
    int c[3], Ec[3];  // the residue class, and its voxels per axis
    convg_tap(cls, cs, c);
    convg_class_grid(g.Eo, c, cs, Ec);
    const int64_t Mc = (int64_t)g.B * Ec[0] * Ec[1] * Ec[2];
    if ((int64_t)blk * CGM_ROWS >= Mc) return;  // uniform

    // this lane's two output voxels (M tiles mt = 0, 1 of the wave's 64 rows)
    int o[2][3], ob[2];
    bool live[2];
    int64_t orow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        int64_t m = (int64_t)blk * CGM_ROWS + wave * 64 + mt * 32 + r;
        live[mt] = m < Mc;
        if (!live[mt]) m = 0;
        ob[mt] = convg_class_row_voxel(m, Ec, c, cs, o[mt]);
        orow[mt] = convg_row(ob[mt], o[mt], g.Eo);
    }

    f32x16 acc[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][mt][i] = 0.f;

    const int k = g.k, ntaps = k * k * k;
    const int nkc = (g.Cin + CGM_KCH - 1) / CGM_KCH;
    // scatter^T: a tap is live for this residue class iff (c + pad - t dil) is divisible by the stride along every axis
    auto tap_live = [&](int t) -> bool {
        if (!TRANSPOSED || cs == 1) return true;
        int tt[3];
        convg_tap(t, k, tt);
        return convg_tap_live(g, c, tt);
    };
    // stage = (tap, channel slice); stages are walked in order, dead taps skipped
    auto next_stage = [&](int& t, int& kc) {
        if (++kc < nkc) return;
        kc = 0;
        do { ++t; } while (t < ntaps && !tap_live(t));
    };

    // weight staging: thread (kg, c4) converts the 8 x 4 block  ci = c0 + 8 kg .. + 7,  co = n0 + 4 c4 .. + 3
    constexpr int C4 = BN / 4;
    const int s_kg = tid / C4, s_c4 = tid - s_kg * C4;
    const bool s_on = s_kg < CGM_KCH / 8;
    float4 wreg[8];
    auto stage_load = [&](int t, int kc) {
        const int c0 = kc * CGM_KCH;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = c0 + 8 * s_kg + e, co = n0 + 4 * s_c4;
            wreg[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s_on && ci < g.Cin && co < g.Cout) wreg[e] = *reinterpret_cast<const float4*>(w + ((int64_t)t * g.Cin + ci) * g.Cout + co);
        }
    };
    auto stage_store = [&](int buf) {
        if (!s_on) return;
        unsigned char* dst = sW + buf * WBUF + (s_kg * BN + 4 * s_c4) * 16;
        const float* f = reinterpret_cast<const float*>(wreg);  // [e][j]
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<uint4*>(dst + j * 16) = make_uint4(pack_bf16x2(f[0 + j], f[4 + j]), pack_bf16x2(f[8 + j], f[12 + j]),
                                                                 pack_bf16x2(f[16 + j], f[20 + j]), pack_bf16x2(f[24 + j], f[28 + j]));
    };

    int t = 0, kc = 0;
    while (t < ntaps && !tap_live(t)) ++t;
    if (t < ntaps) stage_load(t, kc);
    const int wslot = cgm_row_channel(r) * 16;  // the weight row this lane feeds into the MFMA
    int it = 0;
    while (t < ntaps) {
        const int buf = it & 1;
        stage_store(buf);
        __syncthreads();
        int tn = t, kn = kc;
        next_stage(tn, kn);
        if (tn < ntaps) stage_load(tn, kn);
        // source voxel of this tap for the lane's two rows
        int tt[3];
        convg_tap(t, k, tt);
        const bf16* src[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            int q[3];
            const bool ok = live[mt] && (TRANSPOSED ? convg_scatter_src<true>(g, o[mt], tt, q) : convg_gather_src(g, o[mt], tt, q));
            src[mt] = ok ? in + convg_row(ob[mt], q, g.Ei) * g.Cin + kc * CGM_KCH + 8 * hh : nullptr;
        }
        const int kcs = min(CGM_KCH, g.Cin - kc * CGM_KCH);  // channels of this slice
        const unsigned char* wb = sW + buf * WBUF + hh * (BN * 16) + wslot;

        for (int ks = 0; ks * 16 < kcs; ++ks) {
            const bool kin = ks * 16 + 8 * hh < kcs;  // (a slice of 8 (mod 16) channels ends in a half K step)
            bf16x8 xf[2], wf[NT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                uint4 u = make_uint4(0, 0, 0, 0);
                if (src[mt] != nullptr && kin) u = *reinterpret_cast<const uint4*>(src[mt] + ks * 16);
                xf[mt] = __builtin_bit_cast(bf16x8, u);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                wf[nt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(wb + (2 * ks * BN + nt * 32) * 16));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[nt], xf[mt], acc[nt][mt], 0, 0, 0);
        }
        t = tn; kc = kn;
        ++it;
    }

    // ---- epilogue: lane (r, hh) holds channels n0 + 32 nt + 16 hh + (0..15) of its voxel in registers 0..15
    const int64_t V = (int64_t)g.Eo[0] * g.Eo[1] * g.Eo[2];
    // the rollout update of the decode conv (e.x != nullptr; the host guarantees Cout <= 16, so the lane with ch == 0 holds every
    // channel of its voxel): x_next = inside ? x + dx_mean + dx_std (acc + bias) : x in fp32 for the F state channels, and its bf16
    // copy in `out`, padded with zeros to Cout.  (A lambda like the staging steps above: as a free function taking `e` the
    // compiler keeps both EPI kernels at 256 VGPRs with scratch.)
    auto rollout_update = [&](const f32x16& a, const float* bv, int64_t vox) {
        const bool upd = e.inside[vox % V] != 0;
        const float* xs = e.x + vox * e.F;
        float* xn = e.x_next + vox * e.F;
        float nx[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            nx[i] = 0.f;
            if (i < e.F) {
                const float xv = xs[i];
                nx[i] = upd ? xv + (e.dx_mean[i] + e.dx_std[i] * (a[i] + bv[i])) : xv;
                xn[i] = nx[i];
            }
        }
#pragma unroll
        for (int h8 = 0; h8 < 2; ++h8) {
            if (8 * h8 >= g.Cout) continue;
            Vec8<bf16> v;
#pragma unroll
            for (int i = 0; i < 8; ++i) v.v[i] = nx[8 * h8 + i];
            v.store(out + vox * g.Cout + 8 * h8);
        }
    };
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ch = n0 + 32 * nt + 16 * hh;
        if (ch >= g.Cout) continue;
        float bv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) bv[i] = (bias != nullptr && ch + i < g.Cout) ? bias[ch + i] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (!live[mt]) continue;
            const int64_t vox = orow[mt];
            if constexpr (EPI) {
                if (e.x != nullptr) {
                    if (ch == 0) rollout_update(acc[nt][mt], bv, vox);
                    continue;
                }
            }
#pragma unroll
            for (int h8 = 0; h8 < 2; ++h8) {
                if (ch + 8 * h8 >= g.Cout) continue;
                const int64_t off = vox * g.Cout + ch + 8 * h8;
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = acc[nt][mt][8 * h8 + i] + bv[8 * h8 + i];
                if constexpr (EPI) {
                    if (e.relu) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
                    }
                    if (e.h != nullptr) {  // the pre-add activation
                        Vec8<bf16> hv;
#pragma unroll
                        for (int i = 0; i < 8; ++i) hv.v[i] = v[i];
                        hv.store(reinterpret_cast<bf16*>(e.h) + off);
                    }
                    const void* adds[2] = {e.add0, e.add1};
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        if (adds[a] == nullptr) continue;
                        const int64_t aoff = ((e.add_bcast >> a) & 1) ? (vox % V) * g.Cout + ch + 8 * h8 : off;
                        Vec8<bf16> av;
                        av.load(reinterpret_cast<const bf16*>(adds[a]) + aoff);
#pragma unroll
                        for (int i = 0; i < 8; ++i) v[i] += av.v[i];
                    }
                }
                if (EPI && e.out_f32) {
                    Vec8<float> ov;
#pragma unroll
                    for (int i = 0; i < 8; ++i) ov.v[i] = v[i];
                    ov.store(reinterpret_cast<float*>(out) + off);
                } else {
                    Vec8<bf16> ov;
#pragma unroll
                    for (int i = 0; i < 8; ++i) ov.v[i] = v[i];
                    ov.store(out + off);
                }
            }
        }
    }
}

int convg_mfma_apply(const ConvG& g, const void* in, const float* w, const float* bias, void* out, bool transposed,
                     const TdxConvgEpilogue* ep, hipStream_t st) {
    const int nt = g.Cout > 32 ? 2 : 1;
    dim3 grid((unsigned)(g.cls_blocks * g.cs * g.cs * g.cs), (unsigned)ceil_div(g.Cout, 32 * nt));
    TdxConvgEpilogue e = {};
    if (ep != nullptr) e = *ep;
#define CGM_GO(TR, NTV, EP) \
    hipLaunchKernelGGL((convg_mfma_kernel<TR, NTV, EP>), grid, dim3(256), 0, st, (const bf16*)in, w, bias, (bf16*)out, g, e)
    if (ep != nullptr) { if (nt == 2) CGM_GO(false, 2, true); else CGM_GO(false, 1, true); }
    else if (transposed)   { if (nt == 2) CGM_GO(true, 2, false); else CGM_GO(true, 1, false); }
    else                   { if (nt == 2) CGM_GO(false, 2, false); else CGM_GO(false, 1, false); }
#undef CGM_GO
    return tdx_launch_status();
}

// ------------------------------------------------------------------------------------------ weight gradient
// dW[t][ci][co] = sum over output voxels o of in[src(o, t)][ci] dy[o][co]: per tap a GEMM with K = voxels, both operands
// voxel-major, so every fragment is a transposed LDS read (ds_read_b64_tr_b16, as tdx_conv1_mfma.hip's weight gradient).
// One workgroup = (tap, 64 ci x 64 co tile, every nsplit-th chunk of 256 output voxels); thread i stages row i of a chunk
// (its source voxel for the tap is computed once per chunk), the next chunk's rows are in flight during the MFMAs.
// Partial tiles are merged with fp32 atomics; dW / dbias must be zero on entry.
#define CGW_PLANE (CGM_ROWS * 64)  // one [256 voxels][32 channels] bf16 plane

__global__ void __launch_bounds__(256, 2)
convg_wgrad_mfma_kernel(const bf16* __restrict__ in, const bf16* __restrict__ dy, float* __restrict__ dw, float* __restrict__ dbias,
                        ConvG g, int nsplit, int n_ci_tiles) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * CGW_PLANE];
    unsigned char* sX = smem;
    unsigned char* sG = smem + 2 * CGW_PLANE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x / nsplit, split = blockIdx.x - tile * nsplit;
    const int ci0 = (tile % n_ci_tiles) * 64, co0 = (tile / n_ci_tiles) * 64;
    const int tap = blockIdx.y;
    int tt[3];
    convg_tap(tap, g.k, tt);
    const int grp = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
    const int col_off = (16 * (grp & 1) + 4 * p4) * 2;
    const int kh = grp >> 1;

    f32x16 acc[2][2], accb[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[0][0][i] = acc[0][1][i] = acc[1][0][i] = acc[1][1][i] = 0.f;
        accb[0][i] = accb[1][i] = 0.f;
    }
    const bool do_bias = dbias != nullptr && tap == 0 && ci0 == 0;
    const int64_t rows = (int64_t)g.B * g.Eo[0] * g.Eo[1] * g.Eo[2];
    const int64_t nchunks = (rows + CGM_ROWS - 1) / CGM_ROWS;

    uint4 xr[8], gr[8];
    auto load_chunk = [&](int64_t ch) {
        int64_t m = ch * CGM_ROWS + tid;
        const bool live = m < rows;
        const bf16* gp = dy + m * g.Cout + co0;
        if (!live) m = 0;
        int oo[3], qq[3];
        const int b = convg_row_voxel(m, g.Eo, oo);
        const bool ok = convg_gather_src(g, oo, tt, qq) && live;
        const bf16* xp = in + convg_row(b, qq, g.Ei) * g.Cin + ci0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            xr[i] = gr[i] = make_uint4(0, 0, 0, 0);
            // a row whose source voxel is outside contributes nothing: its x piece is zero (dy still feeds the bias sum)
            if (ok && ci0 + 8 * i < g.Cin) xr[i] = *reinterpret_cast<const uint4*>(xp + 8 * i);
            if (live && co0 + 8 * i < g.Cout) gr[i] = *reinterpret_cast<const uint4*>(gp + 8 * i);
        }
    };
    const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u));
    if (split < nchunks) load_chunk(split);
    for (int64_t ch = split; ch < nchunks; ch += nsplit) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // piece i of row tid: plane i >> 2, 16-B chunk i & 3 of the plane's 64-B row
            *reinterpret_cast<uint4*>(sX + (i >> 2) * CGW_PLANE + tid * 64 + (i & 3) * 16) = xr[i];
            *reinterpret_cast<uint4*>(sG + (i >> 2) * CGW_PLANE + tid * 64 + (i & 3) * 16) = gr[i];
        }
        __syncthreads();
        if (ch + nsplit < nchunks) load_chunk(ch + nsplit);
#pragma unroll
        for (int s = 0; s < 4; ++s) {  // the wave reduces rows [64 wave, 64 wave + 64): 4 K steps of 16 voxels
            const int row = wave * 64 + 16 * s + 8 * kh + q4;
            bf16x8 af[2], bfv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const unsigned char* ap = sX + m * CGW_PLANE + row * 64 + col_off;
                af[m] = tr_frag(ap, ap + 4 * 64);
                const unsigned char* bp = sG + m * CGW_PLANE + row * 64 + col_off;
                bfv[m] = tr_frag(bp, bp + 4 * 64);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[m], bfv[n], acc[m][n], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int n = 0; n < 2; ++n) accb[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, bfv[n], accb[n], 0, 0, 0);
            }
        }
    }
    const int r = lane & 31, hh = lane >> 5;
    float* dwt = dw + (int64_t)tap * g.Cin * g.Cout;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ci = acc_row(i, hh, ci0 + m * 32), co = co0 + n * 32 + r;
                if (ci < g.Cin && co < g.Cout) atomicAdd(&dwt[(int64_t)ci * g.Cout + co], acc[m][n][i]);
            }
    if (do_bias && hh == 0) {  // every row of accb is the column sum; row 0 sits in register 0 of lane half 0
#pragma unroll
        for (int n = 0; n < 2; ++n)
            if (co0 + n * 32 + r < g.Cout) atomicAdd(&dbias[co0 + n * 32 + r], accb[n][0]);
    }
}

int convg_mfma_bwd_weight(const ConvG& g, const void* in, const void* dy, float* dw, float* dbias, hipStream_t st) {
    const int k = g.k, n_ci = ceil_div(g.Cin, 64), n_co = ceil_div(g.Cout, 64);
    const int64_t rows = (int64_t)g.B * g.Eo[0] * g.Eo[1] * g.Eo[2];
    const int64_t nchunks = (rows + CGM_ROWS - 1) / CGM_ROWS;
    // enough workgroups for four rounds of the chip, at least four chunks per workgroup
    const int64_t base = (int64_t)k * k * k * n_ci * n_co;
    int64_t nsplit = (2048 + base - 1) / base;
    if (nsplit > nchunks / 4) nsplit = nchunks / 4;
    if (nsplit < 1) nsplit = 1;
    dim3 grid((unsigned)(n_ci * n_co * nsplit), (unsigned)(k * k * k));
    hipLaunchKernelGGL(convg_wgrad_mfma_kernel, grid, dim3(256), 0, st, (const bf16*)in, (const bf16*)dy, dw, dbias, g, (int)nsplit, n_ci);
    return tdx_launch_status();
}
