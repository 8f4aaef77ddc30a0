// bf16 / fp16 MFMA flash attention (forward) for long token sequences (BASELINE config 5:
// N = 96*32*24 = 73 728 voxels, 4 heads x 32).  gfx950.
//
// qkv is the NDHWC to_qkv output [B][N][3*H*D] (q | k | v thirds, head-major), D = 32.
// One wave owns 32 queries of one (b, h); a workgroup = 8 waves = 256 queries, and walks the
// keys in tiles of 64 staged through LDS (K and V, 4 KB each, shared by the 8 waves; the next
// tile's global loads are in flight during the current tile).
//
// Per 32-key block and 32-query tile:
//   S^T = K Q^T        2 x v_mfma_f32_32x32x16_bf16 (sum over d = 32).  Issued "swapped" (keys
//                      as rows) so that a lane owns ONE query and 16 of the 32 keys: the
//                      softmax row max / row sum are 16 in-register ops + one lane<->lane+32
//                      exchange, no LDS.
//   P^T = exp2(S^T - m)  in registers; Q is pre-scaled by log2(e)/sqrt(D).
//   O^T += V^T P^T     2 x MFMA (sum over the 32 keys): the P^T accumulator tile is converted
//                      to bf16 and used directly as the B operand (its rows are the summed
//                      index); the matching k-permuted V^T fragments are transposed LDS reads
//                      (ds_read_b64_tr_b16) of the row-major V tile.
// O^T[d][q] keeps the query on the lane, so the online-softmax rescale is a per-lane scalar.
//
// With D = 32 the kernel is bound by the softmax VALU work (N^2 exponentials), not by the
// matrix cores: 4 MFMAs (128 pipe cycles) per 32x32 tile against 16 quarter-rate v_exp_f32 (256
// cycles) + ~60 plain VALU instructions (v_max3, packed f32 sub / sum, packed bf16 conversion).
#include "tdx_attention.h"

// ---------------------------------------------------------------------------------------------------------------
// Forward kernel, round 5.  What bound the round-3 kernel (0.21 of the matrix peak at N = 73 728): per 32 x 32 score tile
// 4 MFMAs (128 matrix-pipe cycles) against ~100 vector instructions -- 16 v_exp_f32 (8 issue cycles each on gfx950), 16
// two-wide packed f32 adds (v_pk_add_f32: ~13 cycles each beside MFMAs, MI355X_MICROARCH.md per-instruction table:
// slower than two plain adds), the max chain with its lane <-> lane + 32 exchange, 16 accumulator zero moves, packed
// converts -- and a grid of 1152 equal workgroups on 512 slots (2.25 rounds run as 3).  Now:
//   * the running maximum is LAZY and enters through the MFMA's C operand: S^T - m comes out of the matrix pipe
//     (C = -m broadcast, 16 registers per query tile kept up to date), so there is no subtraction and no zeroing; m is only
//     raised when some score of the tile exceeds it by more than an allowance (wave-uniform branch, rare after the first
//     tiles): probabilities are then <= 2^allowance instead of <= 1 -- exact in floating point, fp32 accumulators;
//   * the row sums l = sum_k P come from the matrix pipe too (a 0 / 1 selector x P^T, two v_mfma_f32_16x16x32 per tile
//     and 4 accumulator registers, on a pipe that idled 60 % of the time): no vector adds, no cross-lane exchange, and l
//     is the sum of the ROUNDED probabilities the numerator uses.  The P^T fragment of the 32x32x16 product (lane = query
//     lane & 31, 8 keys of half lane >> 5) read as the B operand of a 16x16x32 product is column n = lane & 15, k group
//     lane >> 4: column n collects query n (k groups 0, 2) and query n + 16 (k groups 1, 3), so selector row 0 = ones on
//     k groups 0 and 2, row 1 = ones on k groups 1 and 3: lane n < 16 ends up with l(query n), l(query n + 16) in its
//     first two accumulator registers;
//   * whether a tile outgrew the allowance is decided by 8 v_max3_i32 + one compare on the score bit patterns -- and not
//     at all for a wave whose queries cannot get there: |s| <= |q| max_k |k| (Cauchy-Schwarz; the key norms' maximum per
//     head comes from a pre-pass over K, 10 us), so once bound - m <= allowance for every query of the wave the loop runs
//     without the check (9 of its ~60 issue slots per tile; with gaussian inputs from the first tile on);
//   * per tile the vector ALU is left with 16 v_exp_f32 and 8 packed converts (+ the check where it is needed);
//   * stream-K schedule: a persistent grid (2 workgroups per CU) splits the linear (query block, key tile) iteration
//     space evenly; a block whose key range straddles two workgroups is finished by a small merge kernel from the
//     partial (O, m, l) both wrote.  XCD x owns a contiguous eighth of the space (one head's K / V per L2).
// (allowance per operand type: E::lazy, tdx_attention.h)

struct AttnSkArgs {
    int N, H, nqb, ntile;      // tokens, heads, query blocks per (b, h), key tiles per block
    long long total;           // iterations = blocks * ntile
    int chunk, nwg;            // iterations per workgroup, workgroups
    float* part;               // [nwg][2 slots][FA_QB][34] f32 partials (O[32], m, l), or nullptr when chunk == ntile
    const float* kmax2;        // [B * H] max_k |k|^2 of each head's keys (attn_kmax_kernel), or nullptr: always check
};

template <typename E>
__global__ void __launch_bounds__(FA_THREADS, 4)
attn_fwd_mfma_kernel(const typename E::T* __restrict__ qkv, typename E::T* __restrict__ out, float* __restrict__ lse, AttnSkArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * FA_KT * 64];
    unsigned char* sK = smem;                // [64 keys][32 d], swizzled 16-B chunks
    unsigned char* sV = smem + FA_KT * 64;   // [64 keys][32 d], plain rows (transposed reads)
    using T = typename E::T;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int N = a.N, H = a.H;
    // XCD x (= hardware workgroup id mod 8) owns the x-th contiguous eighth of the iteration space
    int w = blockIdx.x;
    if ((a.nwg & 7) == 0) w = (w & 7) * (a.nwg >> 3) + (w >> 3);
    long long it = (long long)w * a.chunk;
    const long long it_end = it + a.chunk < a.total ? it + a.chunk : a.total;

    const float qscale = 1.4426950408889634f * rsqrtf((float)FA_D);
    // staging role: 64 keys x 4 chunks of 16 B, K by the first 256 threads, V by the other 256
    const int st_key = (tid & 255) >> 2, st_c = tid & 3, st_v = tid >> 8;
    const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
    const int v_col = (16 * (g & 1) + 4 * tp) * 2;
    bf16x8 sel;  // A operand of the row-sum product: A[m = lane & 15][k group = lane >> 4]
    {
        const unsigned one2 = (lane == 0 || lane == 32 || lane == 17 || lane == 49) ? E::pack2(1.0f, 1.0f) : 0u;
        sel = __builtin_bit_cast(bf16x8, make_uint4(one2, one2, one2, one2));
    }

    while (it < it_end) {
        const int blk = (int)(it / a.ntile);
        const int t0 = (int)(it - (long long)blk * a.ntile);
        const int t1 = (int)((long long)a.ntile - t0 <= it_end - it ? a.ntile : t0 + (it_end - it));
        const int bh = blk / a.nqb, qb = blk - bh * a.nqb;
        const AttnHead<FA_D> hd(bh, N, H);
        const T* base = hd.batch(qkv);
        const int q0 = qb * FA_QB + wave * FA_QW;

        // ---- Q fragments (B operand: col = query r, k = d), pre-scaled by log2(e)/sqrt(D)
        bf16x8 qf[2];
        {
            const int q = min(q0 + r, N - 1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) qf[ks] = row_frag<E>(hd.q(base, q) + ks * 16 + hh * 8, qscale);
        }
        // |q|^2 of the lane's (rounded, pre-scaled) query: 16 of its 32 components here, the rest in lane ^ 32
        float bound = INFINITY;  // upper bound of every score of this query against this head's keys (log2 units)
        if (a.kmax2 != nullptr) {
            float q2 = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint4 u = __builtin_bit_cast(uint4, qf[ks]);
                const unsigned wv[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = E::lo(wv[e]), hi = E::hi(wv[e]);
                    q2 = __builtin_fmaf(lo, lo, __builtin_fmaf(hi, hi, q2));
                }
            }
            q2 += __shfl_xor(q2, 32, 64);
            bound = 1.001f * sqrtf(q2 * a.kmax2[bh]) + 1e-3f;
        }
        f32x16 o, negm;  // O^T[d][q]; -m broadcast over the 16 score registers
        f32x4 ls;        // row sums: lanes 0..15, [0] = query lane, [1] = query lane + 16
        float m;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) ls[i] = 0.f;

        uint4 sreg;
        auto load_tile = [&](int k0) {
            const int key = min(k0 + st_key, N - 1);
            sreg = *reinterpret_cast<const uint4*>(hd.kv(base, key, st_v) + st_c * 8);
        };
        auto stage = [&](int t) {  // tile t: registers -> LDS, next tile's loads in flight
            __syncthreads();
            if (st_v == 0) *reinterpret_cast<uint4*>(sK + sw64(st_key, st_c)) = sreg;
            else *reinterpret_cast<uint4*>(sV + st_key * 64 + st_c * 16) = sreg;
            __syncthreads();
            if (t + 1 < t1) load_tile((t + 1) * FA_KT);
        };
        // raise the running maximum by what the scores `mx` (relative to the stale one) ask for; everything accumulated
        // under the old maximum shrinks by alpha.  Rare; it sits on the loop's retry edge, not in the
        // straight-line tile code: an in-place update of the 16-register MFMA tuples inside a branch there made the
        // compiler copy o / negm (18 v_mov_b64) on the common path of every tile.
        auto raise = [&](float mx) {
            const float d = fmaxf(fmaxf(mx, __shfl_xor(mx, 32, 64)), 0.f);
            const float alpha = __builtin_amdgcn_exp2f(-d);
            m += d;
            ls[0] *= alpha;                                // lane n < 16: query n ...
            ls[1] *= __shfl(alpha, (lane + 16) & 63, 64);  // ... and query n + 16
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                o[i] *= alpha;
                negm[i] -= d;
            }
            return d;
        };
        auto row_max = [&](const f32x16& st) {  // exact (the rare paths and the segment's first block)
            float mx = st[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, st[i]);
            return mx;
        };
        // "does any score exceed the allowance?" needs no float maximum: for positive floats the order of the bit patterns
        // as signed integers is the order of the values, and any negative float is a negative integer -- so the integer
        // maximum of the patterns exceeds bits(allowance) exactly when some score does.  v_max3_i32 straight on the MFMA
        // result: no canonicalising v_max in front (fmaxf on matrix-pipe outputs gets one per operand), no asm hazard nops.
        auto row_max_bits = [&](const f32x16& st) {
            int mx = max(max(__float_as_int(st[0]), __float_as_int(st[1])), __float_as_int(st[2]));
#pragma unroll
            for (int i = 3; i < 15; i += 2) mx = max(max(mx, __float_as_int(st[i])), __float_as_int(st[i + 1]));
            return max(mx, __float_as_int(st[15]));
        };
        auto frags = [&](int kb, bf16x8 (&kf)[2], bf16x8 (&vf)[2]) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) kf[ks] = attn_row_frag(sK, kb, r, ks, hh);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) vf[s2] = attn_tr_frag(sV, kb, s2, g, tq, v_col);
        };
        auto accumulate = [&](f32x16& st, const bf16x8 (&vf)[2]) {  // P = 2^st; O^T += V^T P^T; l += sum P
#pragma unroll
            for (int i = 0; i < 16; ++i) st[i] = __builtin_amdgcn_exp2f(st[i]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                // the probabilities are rounded to nearest (pack2: one v_cvt_pk_* per pair on gfx950), in fp16 too.  Not
                // v_cvt_pkrtz_f16_f32: truncation makes every row sum, and with it the exported log-sum-exp, 3.5e-4 too small
                // -- that cancels in O, but the backward normalises its round-to-nearest probabilities by that lse and its
                // rows would sum to 1 + 3.5e-4 (test_attention_backward.py)
                const bf16x8 pf = acc_as_b<E>(st, s2);
                o = E::mfma(vf[s2], pf, o);
                ls = E::mfma16(sel, pf, ls);  // row sums of the rounded probabilities
            }
        };

        load_tile(t0 * FA_KT);
        stage(t0);
        {   // the maximum over the segment's first 32 keys starts m (key t0 * 64 < N: finite)
            f32x16 s0;
#pragma unroll
            for (int i = 0; i < 16; ++i) s0[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                s0 = E::mfma(attn_row_frag(sK, 0, r, ks, hh), qf[ks], s0);
            if (t0 * FA_KT + 32 > N) {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (acc_row(i, hh, t0 * FA_KT) >= N) s0[i] = -INFINITY;
            }
            float mx = row_max(s0);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (E::headroom > 0.f) {  // (bound = inf without the key norms: no lift)
                const float lift = bound - E::lazy + 0.1f - mx;  // what m lacks for the check-free loop
                if (__builtin_amdgcn_ballot_w64(lift > E::headroom) == 0) mx += fmaxf(lift, 0.f);
            }
            m = mx;
#pragma unroll
            for (int i = 0; i < 16; ++i) negm[i] = -mx;
        }

        // ---- main loop over the 32-key blocks j of the tiles that lie wholly below N: no masking, and no in-place
        // update on the straight path (four waves per SIMD hide each other's matrix-pipe and LDS latencies)
        const int t_full = min(t1, N / FA_KT);  // tiles [t0, t_full) have all 64 keys
        int j = 2 * t0;
        bool staged = true;  // tile j >> 1 is in LDS
        // can some query of this wave still meet a score above its stale maximum + allowance?
        bool check = __builtin_amdgcn_ballot_w64(bound - m > E::lazy - 0.05f) != 0;
        while (check && j < 2 * t_full) {  // loop 1: looks at every block's scores
            if (!staged) { stage(j >> 1); staged = true; }
            bf16x8 kf[2], vf[2];
            frags(j & 1, kf, vf);
            f32x16 st = E::mfma(kf[0], qf[0], negm);  // S^T - m straight from the matrix pipe
            st = E::mfma(kf[1], qf[1], st);
            if (__builtin_amdgcn_ballot_w64(row_max_bits(st) > __float_as_int(E::lazy)) != 0) {
                raise(row_max(st));
                check = __builtin_amdgcn_ballot_w64(bound - m > E::lazy - 0.05f) != 0;
                continue;  // the same block again, under the new maximum (or in loop 2)
            }
            accumulate(st, vf);
            ++j;
            staged = (j & 1) != 0;
        }
        for (; j < 2 * t_full; ++j) {  // loop 2: no score of the rest can outgrow the allowance
            if (!staged) stage(j >> 1);
            bf16x8 kf[2], vf[2];
            frags(j & 1, kf, vf);
            f32x16 st = E::mfma(kf[0], qf[0], negm);
            st = E::mfma(kf[1], qf[1], st);
            accumulate(st, vf);
            staged = (j & 1) == 0;
        }
        // ---- the block's last tile when N is not a multiple of 64: keys beyond N masked, maxima exact
        if (t_full < t1) {
            if (t_full != t0) stage(t_full);  // (the segment's first tile is in LDS already)
            const int k0 = t_full * FA_KT;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                bf16x8 kf[2], vf[2];
                frags(kb, kf, vf);
                f32x16 st = E::mfma(kf[0], qf[0], negm);
                st = E::mfma(kf[1], qf[1], st);
#pragma unroll
                for (int i = 0; i < 16; ++i)  // register i <-> key (i & 3) + 8 (i >> 2) + 4 hh
                    if (acc_row(i, hh, k0 + kb * 32) >= N) st[i] = -INFINITY;
                const float mx = row_max(st);
                if (__builtin_amdgcn_ballot_w64(mx > 0.f) != 0) {
                    const float d = raise(mx);
#pragma unroll
                    for (int i = 0; i < 16; ++i) st[i] -= d;
                }
                accumulate(st, vf);
            }
        }

        // ---- segment epilogue; lane holds d = acc_row(i, hh) of query r
        const float l0 = __shfl(ls[0], r & 15, 64), l1 = __shfl(ls[1], r & 15, 64);
        const float lq = r < 16 ? l0 : l1;  // l of the lane's query: from lane r & 15, register r >> 4
        const int q = q0 + r;
        if (t0 == 0 && t1 == a.ntile) {  // the whole key range: final result
            if (q < N) {
                const float inv = 1.0f / lq;
                T* op = hd.out_row(out, q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) attn_store_row_piece<E>(op, o, jj, inv, hh);
                if (hh == 0) lse[hd.stat(q)] = (m + log2f(lq)) * 0.6931471805599453f;
            }
        } else {
            // part of the key range: (O, m, l) relative to this segment's m; slot 0 = the block began in an earlier
            // workgroup (this workgroup's first segment), slot 1 = it continues in the next one (its last segment)
            float* pq = a.part + ((size_t)w * 2 + (t0 == 0 ? 1 : 0)) * FA_PART_STRIDE + (size_t)(wave * FA_QW + r) * 34;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                float* pd = pq + 8 * jj + 4 * hh;  // 136-B rows: 8-B aligned
                *reinterpret_cast<float2*>(pd) = make_float2(o[4 * jj], o[4 * jj + 1]);
                *reinterpret_cast<float2*>(pd + 2) = make_float2(o[4 * jj + 2], o[4 * jj + 3]);
            }
            if (hh == 0) { pq[32] = m; pq[33] = lq; }
        }
        it += t1 - t0;  // (the next segment's stage() opens with a barrier: its LDS stores wait for this one's last reads)
    }
}

// max_k |k|^2 per (b, h): one pass over K, block maxima merged by integer atomics on the (non-negative) float patterns.
template <typename T>
__global__ void __launch_bounds__(256)
attn_kmax_kernel(const T* __restrict__ qkv, float* __restrict__ kmax2, int N, int H) {
    const int bh = blockIdx.y;
    const AttnHead<FA_D> hd(bh, N, H);
    const T* base = hd.k(hd.batch(qkv), 0);  // the head's first key
    float mx = 0.f;
    for (int key = blockIdx.x * 64 + (threadIdx.x >> 2); key < N; key += gridDim.x * 64) {
        Vec8<T> v;
        v.load(base + (int64_t)key * hd.ld + (threadIdx.x & 3) * 8);
        float s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s2 = __builtin_fmaf(v.v[e], v.v[e], s2);
        s2 += __shfl_xor(s2, 1, 64);
        s2 += __shfl_xor(s2, 2, 64);
        mx = fmaxf(mx, s2);
    }
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<int*>(kmax2) + bh, __float_as_int(mx));
}

// Blocks whose key range was split over workgroups: combine the partial (O, m, l) of every workgroup that touched them.
template <typename E>
__global__ void __launch_bounds__(FA_QB)
attn_fwd_merge_kernel(typename E::T* __restrict__ out, float* __restrict__ lse, AttnSkArgs a) {
    const int blk = blockIdx.x;
    const long long lo = (long long)blk * a.ntile, hi = lo + a.ntile;
    const int w_lo = (int)(lo / a.chunk), w_hi = (int)((hi - 1) / a.chunk);
    if (w_lo == w_hi) return;  // one workgroup had the whole block and wrote the result
    const int bh = blk / a.nqb, qb = blk - bh * a.nqb;
    const AttnHead<FA_D> hd(bh, a.N, a.H);
    const int ql = threadIdx.x, q = qb * FA_QB + ql;
    if (q >= a.N) return;
    float mt = -INFINITY;
    for (int w = w_lo; w <= w_hi; ++w)
        mt = fmaxf(mt, a.part[((size_t)w * 2 + (w == w_lo ? 1 : 0)) * FA_PART_STRIDE + (size_t)ql * 34 + 32]);
    float acc[FA_D], l = 0.f;
#pragma unroll
    for (int d = 0; d < FA_D; ++d) acc[d] = 0.f;
    for (int w = w_lo; w <= w_hi; ++w) {
        const float* pq = a.part + ((size_t)w * 2 + (w == w_lo ? 1 : 0)) * FA_PART_STRIDE + (size_t)ql * 34;
        const float sc = exp2f(pq[32] - mt);
        l += sc * pq[33];
#pragma unroll
        for (int d = 0; d < FA_D; d += 2) {
            const float2 v = *reinterpret_cast<const float2*>(pq + d);
            acc[d] += sc * v.x;
            acc[d + 1] += sc * v.y;
        }
    }
    const float inv = 1.0f / l;
    typename E::T* op = hd.out_row(out, q);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        *reinterpret_cast<uint4*>(op + 8 * j) =
            make_uint4(E::pack2(acc[8 * j] * inv, acc[8 * j + 1] * inv), E::pack2(acc[8 * j + 2] * inv, acc[8 * j + 3] * inv),
                       E::pack2(acc[8 * j + 4] * inv, acc[8 * j + 5] * inv), E::pack2(acc[8 * j + 6] * inv, acc[8 * j + 7] * inv));
    lse[hd.stat(q)] = (mt + log2f(l)) * 0.6931471805599453f;
}

// What the plan says, launched: the key-norm pre-pass into its table (bound), the flash kernel on the plan's grid, and under
// stream-K the merge of the blocks that were split over workgroups.
int attn_fwd_mfma_launch(const AttnFwdCall& c, const AttnPlan& p) {
    if (p.fwd != TDX_ATTN_MFMA) return TDX_EINVAL;
    AttnSkArgs a;
    a.N = c.N; a.H = c.H;
    a.nqb = p.nqb; a.ntile = p.ntile;
    a.total = (long long)p.nblk * p.ntile;
    a.chunk = p.chunk; a.nwg = p.nwg;
    a.part = p.streamk ? reinterpret_cast<float*>(tdx_scratch_region(FA_PART_OFFSET, FA_PART_BYTES)) : nullptr;
    float* km = p.bound ? reinterpret_cast<float*>(tdx_scratch_region(FA_KMAX_OFFSET, FA_KMAX_BYTES)) : nullptr;
    a.kmax2 = km;
    if ((p.streamk && a.part == nullptr) || (p.bound && km == nullptr)) return TDX_EINVAL;  // not this arena's plan
    if (p.bound && tdx_zero_async(km, (size_t)c.B * c.H * sizeof(float), c.st) != TDX_OK) return TDX_EINVAL;
    return attn_h16_dispatch(c.dtype, [&](auto e) {
        using E = decltype(e);
        using T = typename E::T;
        if (p.bound)
            hipLaunchKernelGGL(attn_kmax_kernel<T>, dim3(min(ceil_div(c.N, 64), 64), c.B * c.H), dim3(256), 0, c.st, (const T*)c.qkv,
                               km, c.N, c.H);
        hipLaunchKernelGGL(attn_fwd_mfma_kernel<E>, dim3(a.nwg), dim3(FA_THREADS), 0, c.st, (const T*)c.qkv, (T*)c.out, c.lse, a);
        if (p.streamk) hipLaunchKernelGGL(attn_fwd_merge_kernel<E>, dim3(p.nblk), dim3(FA_QB), 0, c.st, (T*)c.out, c.lse, a);
        return tdx_launch_status();
    });
}
