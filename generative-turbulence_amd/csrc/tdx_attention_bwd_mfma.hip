// bf16 / fp16 MFMA flash attention, backward (long token sequences; BASELINE config 5 sizes).  gfx950.
//
// Same data layout and the same "swapped" MFMA orientation as the forward kernel
// (tdx_attention_mfma.hip): a lane owns ONE row of the side its workgroup keeps resident, so every
// per-row scalar (log-sum-exp, delta) is a per-lane register and the probability tile that comes out of
// one MFMA is, converted to bf16 in registers, directly the B operand of the next.
//
// With P = softmax(Q K^T / sqrt(D)) (recomputed from the saved log-sum-exp), dP = dO V^T,
// dS = P o (dP - delta), delta_i = dO_i . O_i:
//
//   dQ kernel   workgroup = 256 queries (a wave = 2 x 32), walks the keys in staged tiles of 64:
//               S^T  = K Q^T            (Q resident, pre-scaled by log2(e)/sqrt(D))
//               dP^T = V dO^T           (dO resident)
//               dS^T = exp2(S^T - lse) o (dP^T - delta)          per-lane lse, delta
//               dQ^T += K^T dS^T        (K^T fragments: transposed LDS reads of the row-major K tile)
//   dK/dV kernel  workgroup = 256 keys, walks the queries in staged tiles of 64 (Q, dO, lse, delta):
//               S  = Q K^T,  dP = dO V^T   (K and V resident as B operands; Q pre-scaled by log2(e)/sqrt(D) when staged)
//               P  = exp2(S - lse_row),  dS = P o (dP - delta_row)     per-register lse, delta
//               dV^T += dO^T P,  dK^T += Q^T dS   (dO^T / Q^T fragments: transposed LDS reads)
//
// The operand that carries log2(e)/sqrt(D), rounded to the format once more, is Q in ALL kernels, with the forward's own
// expression: the saved log-sum-exp belongs to the forward's scores, and exp2(S' - lse) is a row of probabilities only if S'
// are those scores bit for bit in their operands.  (Scaling K in the dK/dV pass instead would move every score by an
// independent 2^-9 |s| in bf16: with |s| ~ 50-200 the recomputed rows sum to 1 +- 0.2 -- tests/test_attention_backward.py.)
//
// 6 + 8 MFMAs per 32 x 32 tile against the forward's 4; no atomics, no running maximum.
#include "tdx_attention.h"
#include <type_traits>

// TW = resident 32-row tiles per wave: 2 (the default: 4 waves per workgroup, 2 waves per SIMD, ~250 / 230 registers) or 1
// (round 6 experiment: 8 waves per workgroup, 3-4 waves per SIMD at <= 168 / 128 registers, as the forward kernel since round 5).
// The ablations (profiles/r13_attention_bwd_ablation.txt) put 2.4 of the 11.5 ms in vector-ALU work next to a 9.1-ms floor of
// the 14 MFMAs per tile pair; more waves per SIMD do not hide it (10.99-12.3 ms): kept as an A/B knob (TDX_ATTN_BWD_TW).
// The walked side is staged in tiles of FB_T(TW) rows, one 16-B piece per thread.
// (FB_RB = 256 resident rows per workgroup and FB_WAVES(TW) = its waves: tdx_attention.h, the plan's grid needs them)
// waves per SIMD the one-tile-per-wave kernels are compiled for (HIP: the second __launch_bounds__ argument is waves per
// execution unit): 4 = at most 128 registers, 3 = at most 168
#ifndef FB_MINW_DQ
#define FB_MINW_DQ 4
#endif
#ifndef FB_MINW_DKV
#define FB_MINW_DKV 4
#endif
#define FB_T(TW) (16 * FB_WAVES(TW))
#define FB_LOG2E 1.4426950408889634f
// Diagnostic builds only (tools/attn_bwd_ablation.sh compiles this file with -DFB_ABL=<bits>): what bounds the two kernels.
//   1 no exponentials (the score stands in for P)          2 no elementwise product dS = P o dP
//   4 no fp32 -> 16-bit conversions of P / dS (a resident fragment stands in as the B operand)
//   8 no dP products (2 of the 6 / 8 MFMAs per tile)      16 no transposed LDS fragment reads (K^T, Q^T, dO^T)
// The product build defines none of it.
#ifndef FB_ABL
#define FB_ABL 0
#endif

// one staged 16-B piece (8 elements) times `scale`, rounded to the format: the forward's expression on Q, so the bits agree
template <typename E>
__device__ __forceinline__ uint4 fb_scale_piece(const uint4& piece, float scale) {
    return __builtin_bit_cast(uint4, row_frag<E>(reinterpret_cast<const typename E::T*>(&piece), scale));
}

// ------------------------------------------------------------------ dQ ---------------------------
template <typename E, int TW>
__global__ void __launch_bounds__(64 * FB_WAVES(TW), TW == 1 ? FB_MINW_DQ : 2)
attn_bwd_dq_mfma_kernel(const typename E::T* __restrict__ qkv, const typename E::T* __restrict__ dout, const float* __restrict__ lse,
                        const float* __restrict__ delta, typename E::T* __restrict__ dqkv, int N, int H) {
    constexpr int T = FB_T(TW), RW = 32 * TW;
    __shared__ __attribute__((aligned(16))) unsigned char smem[3 * T * 64];
    unsigned char* sK = smem;                  // K tile, swizzled chunks (S^T = K Q^T: A operand rows = keys)
    unsigned char* sKp = smem + T * 64;        // K tile, plain rows (K^T fragments by transposed reads)
    unsigned char* sV = smem + 2 * T * 64;     // V tile, swizzled chunks (dP^T = V dO^T)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const AttnHead<FA_D> hd(blockIdx.y, N, H);
    const typename E::T* base = hd.batch(qkv);
    const int q0 = blockIdx.x * FB_RB + wave * RW;
    const float sm_scale = rsqrtf((float)FA_D);

    bf16x8 qf[TW][2], gf[TW][2];  // Q (pre-scaled) and dO as B operands: col = query r, k = d
    // -lse log2(e) and -delta of the lane's query, broadcast over the 16 accumulator registers: as the C operands of the
    // score / dP products they deliver S^T - lse and dP^T - delta straight from the matrix pipe (the kernel is bound by its
    // vector-ALU work: that was 32 subtractions and 32 zeroing moves of ~110 issue slots per 32 x 32 tile)
    f32x16 nl[TW], nd[TW];
    f32x16 dq[TW];               // dQ^T[d][q]
#pragma unroll
    for (int qt = 0; qt < TW; ++qt) {
        const int q = min(q0 + qt * 32 + r, N - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[qt][ks] = row_frag<E>(hd.q(base, q) + ks * 16 + hh * 8, FB_LOG2E * sm_scale);
            gf[qt][ks] = row_frag<E>(hd.out_row(dout, q) + ks * 16 + hh * 8, 1.0f);
        }
        const float ml = -lse[hd.stat(q)] * FB_LOG2E, md = -delta[hd.stat(q)];
#pragma unroll
        for (int i = 0; i < 16; ++i) { dq[qt][i] = 0.f; nl[qt][i] = ml; nd[qt][i] = md; }
    }

    const int st_row = tid >> 2, st_c = tid & 3;
    uint4 kreg, vreg;
    auto load_tile = [&](int k0) {
        const int key = min(k0 + st_row, N - 1);
        // (hd.k(base, key), written out: through the helper the two-tile instances schedule their prologue differently)
        const typename E::T* kp = base + (int64_t)key * hd.ld + H * FA_D + hd.h * FA_D + st_c * 8;
        kreg = *reinterpret_cast<const uint4*>(kp);
        vreg = *reinterpret_cast<const uint4*>(kp + H * FA_D);
    };
    const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
    const int t_col = (16 * (g & 1) + 4 * tp) * 2;

    load_tile(0);
    for (int k0 = 0; k0 < N; k0 += T) {
        __syncthreads();
        *reinterpret_cast<uint4*>(sK + sw64(st_row, st_c)) = kreg;
        *reinterpret_cast<uint4*>(sKp + st_row * 64 + st_c * 16) = kreg;
        *reinterpret_cast<uint4*>(sV + sw64(st_row, st_c)) = vreg;
        __syncthreads();
        if (k0 + T < N) load_tile(k0 + T);

        auto key_block = [&](int kb, auto tail_c) {
            constexpr bool TAIL = decltype(tail_c)::value;
            bf16x8 kf[2], vf[2], ktf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                kf[ks] = attn_row_frag(sK, kb, r, ks, hh);
                vf[ks] = attn_row_frag(sV, kb, r, ks, hh);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)  // K^T: rows = d, k = key 16 s + 8 (j >> 2) + 4 hh + (j & 3)
                ktf[s] = (FB_ABL & 16) ? kf[s] : attn_tr_frag(sKp, kb, s, g, tq, t_col);
#pragma unroll
            for (int qt = 0; qt < TW; ++qt) {
                f32x16 st = E::mfma(kf[0], qf[qt][0], nl[qt]);   // S^T - lse
                st = E::mfma(kf[1], qf[qt][1], st);
                f32x16 dp = nd[qt];
                if (!(FB_ABL & 8)) {
                    dp = E::mfma(vf[0], gf[qt][0], nd[qt]);   // dP^T - delta
                    dp = E::mfma(vf[1], gf[qt][1], dp);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float p = (FB_ABL & 1) ? st[i] : __builtin_amdgcn_exp2f(st[i]);
                    if (TAIL && acc_row(i, hh, k0 + kb * 32) >= N) p = 0.f;  // keys beyond N
                    st[i] = (FB_ABL & 2) ? p : p * dp[i];  // dS^T
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) dq[qt] = E::mfma(ktf[s], (FB_ABL & 4) ? qf[qt][s] : acc_as_b<E>(st, s), dq[qt]);
                if (FB_ABL & 4) dq[qt][0] += st[0] + st[15];  // (keeps the elementwise work alive)
            }
        };
        if (k0 + T <= N) {
#pragma unroll
            for (int kb = 0; kb < T / 32; ++kb) key_block(kb, std::false_type{});
        } else {
#pragma unroll
            for (int kb = 0; kb < T / 32; ++kb) key_block(kb, std::true_type{});
        }
    }
    // dQ[q][h*D + d] = scale * dQ^T[d][q];  lane holds d = acc_row(i, hh)
#pragma unroll
    for (int qt = 0; qt < TW; ++qt) {
        const int q = q0 + qt * 32 + r;
        if (q < N) {
            typename E::T* op = hd.dq(dqkv, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) attn_store_row_piece<E>(op, dq[qt], j, sm_scale, hh);
        }
    }
}

// ------------------------------------------------------------------ dK, dV -----------------------
template <typename E, int TW>
__global__ void __launch_bounds__(64 * FB_WAVES(TW), TW == 1 ? FB_MINW_DKV : 2)
attn_bwd_dkv_mfma_kernel(const typename E::T* __restrict__ qkv, const typename E::T* __restrict__ dout, const float* __restrict__ lse,
                         const float* __restrict__ delta, typename E::T* __restrict__ dqkv, int N, int H) {
    constexpr int T = FB_T(TW), RW = 32 * TW;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * T * 64 + 2 * T * 4];
    unsigned char* sQ = smem;                   // Q tile, swizzled (S = Q K^T: A operand rows = queries)
    unsigned char* sQp = smem + T * 64;         // Q tile, plain rows (Q^T fragments)
    unsigned char* sG = smem + 2 * T * 64;      // dO tile, swizzled (dP = dO V^T)
    unsigned char* sGp = smem + 3 * T * 64;     // dO tile, plain rows (dO^T fragments)
    float* sL = reinterpret_cast<float*>(smem + 4 * T * 64);  // -lse * log2(e) of the tile's queries (-inf beyond N)
    float* sD = sL + T;                                        // -delta

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const AttnHead<FA_D> hd(blockIdx.y, N, H);
    const typename E::T* base = hd.batch(qkv);
    const int j0 = blockIdx.x * FB_RB + wave * RW;
    const float qscale = FB_LOG2E * rsqrtf((float)FA_D);
    const float dk_scale = 0.6931471805599453f;  // ln 2 = (1/sqrt(D)) / (log2(e)/sqrt(D)): the staged Q carries the rest

    bf16x8 kf[TW][2], vf[TW][2];  // K and V as stored, as B operands: col = key r, k = d
    f32x16 dk[TW], dv[TW];        // dK^T[d][key], dV^T[d][key]
#pragma unroll
    for (int kt = 0; kt < TW; ++kt) {
        const int key = min(j0 + kt * 32 + r, N - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[kt][ks] = row_frag<E>(hd.k(base, key) + ks * 16 + hh * 8, 1.0f);
            vf[kt][ks] = row_frag<E>(hd.v(base, key) + ks * 16 + hh * 8, 1.0f);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[kt][i] = dv[kt][i] = 0.f;
    }

    const int st_row = tid >> 2, st_c = tid & 3;
    uint4 qreg, greg;
    float lreg = 0.f, dreg = 0.f;
    auto load_tile = [&](int i0) {
        const int q = min(i0 + st_row, N - 1);
        qreg = *reinterpret_cast<const uint4*>(hd.q(base, q) + st_c * 8);
        greg = *reinterpret_cast<const uint4*>(hd.out_row(dout, q) + st_c * 8);
        if (tid < T) {
            const int qq = i0 + tid;
            lreg = qq < N ? -lse[hd.stat(qq)] * FB_LOG2E : -INFINITY;  // exp2(s - inf) = 0: no query there
            dreg = qq < N ? -delta[hd.stat(qq)] : 0.f;
        }
    };
    const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
    const int t_col = (16 * (g & 1) + 4 * tp) * 2;

    load_tile(0);
    for (int i0 = 0; i0 < N; i0 += T) {
        __syncthreads();
        // Q enters LDS as the forward's operand, round(q * log2(e)/sqrt(D)): the scores are the forward's, and the Q^T
        // fragments of dK^T += Q^T dS carry the factor too (taken out again in the epilogue)
        const uint4 qs = fb_scale_piece<E>(qreg, qscale);
        *reinterpret_cast<uint4*>(sQ + sw64(st_row, st_c)) = qs;
        *reinterpret_cast<uint4*>(sQp + st_row * 64 + st_c * 16) = qs;
        *reinterpret_cast<uint4*>(sG + sw64(st_row, st_c)) = greg;
        *reinterpret_cast<uint4*>(sGp + st_row * 64 + st_c * 16) = greg;
        if (tid < T) { sL[tid] = lreg; sD[tid] = dreg; }
        __syncthreads();
        if (i0 + T < N) load_tile(i0 + T);

#pragma unroll
        for (int qb = 0; qb < T / 32; ++qb) {
            bf16x8 qa[2], ga[2], qtf[2], gtf[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {  // A operands: row = query r, k = d
                qa[ks] = attn_row_frag(sQ, qb, r, ks, hh);
                ga[ks] = attn_row_frag(sG, qb, r, ks, hh);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {  // Q^T, dO^T: rows = d, k = query 16 s + 8 (j >> 2) + 4 hh + (j & 3)
                const int off = (qb * 32 + 16 * s + 4 * (g >> 1) + tq) * 64 + t_col;  // (attn_tr_frag's address, once for two tiles)
                qtf[s] = (FB_ABL & 16) ? qa[s] : tr_frag(sQp + off, sQp + off + 8 * 64);
                gtf[s] = (FB_ABL & 16) ? ga[s] : tr_frag(sGp + off, sGp + off + 8 * 64);
            }
            // per-register row scalars: register i <-> query row (i & 3) + 8 (i >> 2) + 4 hh of the block.  The sixteen
            // (negated) values ARE the C operands of the score / dP products: S - lse and dP - delta come out of the
            // matrix pipe, the vector ALU keeps the exponential, one product and the conversions
            f32x16 lrow, drow;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 l4 = *reinterpret_cast<const float4*>(sL + qb * 32 + 8 * c + 4 * hh);
                const float4 d4 = *reinterpret_cast<const float4*>(sD + qb * 32 + 8 * c + 4 * hh);
                lrow[4 * c] = l4.x; lrow[4 * c + 1] = l4.y; lrow[4 * c + 2] = l4.z; lrow[4 * c + 3] = l4.w;
                drow[4 * c] = d4.x; drow[4 * c + 1] = d4.y; drow[4 * c + 2] = d4.z; drow[4 * c + 3] = d4.w;
            }
#pragma unroll
            for (int kt = 0; kt < TW; ++kt) {
                f32x16 st = E::mfma(qa[0], kf[kt][0], lrow);
                st = E::mfma(qa[1], kf[kt][1], st);
                f32x16 dp = drow;
                if (!(FB_ABL & 8)) {
                    dp = E::mfma(ga[0], vf[kt][0], drow);
                    dp = E::mfma(ga[1], vf[kt][1], dp);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (!(FB_ABL & 1)) st[i] = __builtin_amdgcn_exp2f(st[i]);  // P
                    if (!(FB_ABL & 2)) dp[i] = st[i] * dp[i];                   // dS
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    dv[kt] = E::mfma(gtf[s], (FB_ABL & 4) ? kf[kt][s] : acc_as_b<E>(st, s), dv[kt]);
                    dk[kt] = E::mfma(qtf[s], (FB_ABL & 4) ? vf[kt][s] : acc_as_b<E>(dp, s), dk[kt]);
                }
                if (FB_ABL & 4) dv[kt][0] += st[0] + st[15] + dp[0] + dp[15];  // (keeps the elementwise work alive)
            }
        }
    }
    // dK[key][..] = ln 2 * dK^T (Q^T was pre-scaled), dV[key][..] = dV^T;  lane holds d = acc_row(i, hh)
#pragma unroll
    for (int kt = 0; kt < TW; ++kt) {
        const int key = j0 + kt * 32 + r;
        if (key < N) {
            typename E::T* okp = hd.dk(dqkv, key);
            typename E::T* ovp = okp + H * FA_D;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                attn_store_row_piece<E>(okp, dk[kt], j, dk_scale, hh);
                attn_store_row_piece<E>(ovp, dv[kt], j, 1.0f, hh);
            }
        }
    }
}

// the plan's instance (tiles per wave) of each of the two kernels on the plan's grid
template <typename E, int TWQ, int TWK>
static int attn_bwd_mfma_go(const AttnBwdCall& c, const AttnPlan& p) {
    using T = typename E::T;
    const dim3 grid(p.bwd_gx, p.bwd_gy);
    hipLaunchKernelGGL((attn_bwd_dq_mfma_kernel<E, TWQ>), grid, dim3(64 * FB_WAVES(TWQ)), 0, c.st, (const T*)c.qkv,
                       (const T*)c.dout, c.lse, c.delta, (T*)c.dqkv, c.N, c.H);
    hipLaunchKernelGGL((attn_bwd_dkv_mfma_kernel<E, TWK>), grid, dim3(64 * FB_WAVES(TWK)), 0, c.st, (const T*)c.qkv,
                       (const T*)c.dout, c.lse, c.delta, (T*)c.dqkv, c.N, c.H);
    return tdx_launch_status();
}

int attn_bwd_mfma_launch(const AttnBwdCall& c, const AttnPlan& p) {
    if (p.bwd != TDX_ATTN_MFMA) return TDX_EINVAL;
    return attn_h16_dispatch(c.dtype, [&](auto e) {
        using E = decltype(e);
        switch (10 * p.twq + p.twk) {
            case 11: return attn_bwd_mfma_go<E, 1, 1>(c, p);
            case 12: return attn_bwd_mfma_go<E, 1, 2>(c, p);
            case 21: return attn_bwd_mfma_go<E, 2, 1>(c, p);
            case 22: return attn_bwd_mfma_go<E, 2, 2>(c, p);
        }
        return (int)TDX_EINVAL;
    });
}
