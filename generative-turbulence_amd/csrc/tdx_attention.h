// Interface of the attention family: the plan of a call (attn_plan, tdx_attention.hip -- the one host function that decides
// what tdx_attn_fwd and tdx_attn_bwd launch), the call records the launchers take, and what the kernels of the three files
// (tdx_attention.hip: entry points and vector-ALU kernels; tdx_attention_mfma.hip: matrix-core forward;
// tdx_attention_bwd_mfma.hip: matrix-core backward) share on the device.
#pragma once
#include "tdx_common.h"
#include "tdx_mfma.h"
#include "tdx_runtime.h"

#define FA_D 32  // head dimension of every kernel of the family

// ---- geometry of the matrix-core kernels
#define FA_KT 64          // forward: keys per staged tile
#define FA_QW 32          // forward: queries per wave (one 32-query tile: <= 128 registers, four waves per SIMD)
#define FA_THREADS 512    // forward: 8 waves
#define FA_QB (8 * FA_QW) // forward: queries per workgroup
#define FB_RB 256         // backward: resident rows per workgroup
#define FB_WAVES(TW) (FB_RB / (32 * (TW)))  // backward: waves per workgroup at TW resident 32-row tiles per wave

// ---- the forward's share of the scratch arena (tdx_runtime.h), right behind the zero block:
//   [FA_KMAX_OFFSET, + FA_KMAX_BYTES)   max_k |k|^2 of up to FA_KMAX_PAIRS (b, h) pairs: the norm bound
//   [FA_PART_OFFSET, + FA_PART_BYTES)   stream-K partials (O[32], m, l) f32: [FA_SLOTS workgroups][2 slots][FA_QB queries][34],
//                                       2 x 512 x 34 816 B = 35.7 MB
#define FA_SLOTS 512  // workgroups of the persistent stream-K grid: 256 CUs x 2
#define FA_KMAX_PAIRS 256
#define FA_KMAX_OFFSET ((size_t)TDX_SCRATCH_ZERO_BYTES)
#define FA_KMAX_BYTES (FA_KMAX_PAIRS * sizeof(float))
#define FA_PART_STRIDE (FA_QB * 34)
#define FA_PART_OFFSET (FA_KMAX_OFFSET + FA_KMAX_BYTES)
#define FA_PART_BYTES ((size_t)FA_SLOTS * 2 * FA_PART_STRIDE * sizeof(float))

// ---- the plan ---------------------------------------------------------------------------------------------------------
// Everything tdx_attn_fwd and tdx_attn_bwd decide for one (B, N, H, D, dtype), from the library switches and the bound
// arena's size as they are at the call.  Fields that do not apply to the chosen family are 0.
struct AttnPlan {
    int status;         // what the entry points return before they launch anything: TDX_OK, TDX_ESHAPE (D != 32), TDX_EDTYPE
    int fwd, bwd;       // TDX_ATTN_VECTOR (the row-wise kernels of tdx_attention.hip) or TDX_ATTN_MFMA
    // matrix-core forward: the linear (query block, key tile) space of nblk * ntile iterations over nwg workgroups of chunk
    // iterations.  Stream-K: nwg = FA_SLOTS, blocks split over workgroups, partials in the arena and a merge launch;
    // otherwise one workgroup per block (nwg = nblk, chunk = ntile).
    int nqb, ntile, nblk, nwg, chunk;
    bool streamk;
    bool bound;         // key-norm pre-pass into the arena: waves whose scores cannot outgrow the allowance skip the check
    int twq, twk;       // matrix-core backward: resident 32-row tiles per wave of the dQ and of the dK/dV kernel (1 or 2)
    int bwd_gx, bwd_gy; // backward grid of both kernels of either family (the forward's too for the vector family)
    size_t workspace;   // bytes of tdx_attn_bwd's workspace: delta, one float per (b, token, head)
};
AttnPlan attn_plan(int B, int N, int H, int D, int dtype);

// One call of an entry point, as the launchers take it
struct AttnFwdCall {
    const void* qkv;
    void* out;
    float* lse;
    int B, N, H, dtype;
    hipStream_t st;
};
struct AttnBwdCall {
    const void *qkv, *dout;
    const float *lse, *delta;
    void* dqkv;
    int B, N, H, dtype;
    hipStream_t st;
};
// The matrix-core launchers: they launch what the plan says and read no switch; TDX_EINVAL for a plan of the other family.
int attn_fwd_mfma_launch(const AttnFwdCall& c, const AttnPlan& p);      // tdx_attention_mfma.hip
int attn_bwd_mfma_launch(const AttnBwdCall& c, const AttnPlan& p);      // tdx_attention_bwd_mfma.hip

// Operand element of the matrix-core attention kernels: bf16 (the model's bf16 mode) or fp16 (BASELINE configs[4]: "fp16
// MFMA QK^T / AV" -- 11 significand bits in P, K and V instead of 8).  H16<HF> with the forward's lazy-maximum constants:
// lazy = the allowance, log2 of how far a probability may exceed 1 under a stale running maximum (probabilities must stay
// finite in the operand format and their sums in fp32).
struct AttnBf16 : H16<false> {
    static constexpr float lazy = 32.0f;
    static constexpr float headroom = 0.0f;
};
struct AttnF16 : H16<true> {
    static constexpr float lazy = 15.0f;  // 2^15 < 65504
    // fp16's allowance is narrow: a segment may START with m up to 2^3 above its first block's maximum when that is what
    // lets the wave run without the check (probabilities then begin at 2^-3; what fp16 flushes to zero moves from 2^-24
    // to 2^-21 of the maximum)
    static constexpr float headroom = 3.0f;
};
// The launchers turn the call's dtype into that element type once: f(AttnBf16{}) or f(AttnF16{})
template <typename F>
static inline int attn_h16_dispatch(int dtype, F&& f) {
    if (dtype == TDX_BF16) return f(AttnBf16{});
    if (dtype == TDX_F16) return f(AttnF16{});
    return TDX_EDTYPE;
}

// One head (b, h) of a call and where its rows are: qkv and dqkv [B][N][3 H D] (q | k | v thirds, head-major inside each),
// out and dout [B][N][H D], lse and delta [B][H][N]
template <int D>
struct AttnHead {
    int b, h, N, H, ld;
    __device__ __forceinline__ AttnHead(int bh, int N_, int H_) : b(bh / H_), h(bh - b * H_), N(N_), H(H_), ld(3 * H_ * D) {}
    __device__ __forceinline__ AttnHead(int b_, int h_, int N_, int H_) : b(b_), h(h_), N(N_), H(H_), ld(3 * H_ * D) {}
    // this batch's tokens of qkv
    template <typename T>
    __device__ __forceinline__ T* batch(T* qkv) const { return qkv + (int64_t)b * N * ld; }
    // token i's row of this head in the q, k or v third of `base` = batch(qkv); kv: k (which = 0) or v (1)
    template <typename T>
    __device__ __forceinline__ T* q(T* base, int64_t i) const { return base + i * ld + h * D; }
    template <typename T>
    __device__ __forceinline__ T* k(T* base, int64_t i) const { return base + i * ld + H * D + h * D; }
    template <typename T>
    __device__ __forceinline__ T* v(T* base, int64_t i) const { return base + i * ld + 2 * H * D + h * D; }
    template <typename T>
    __device__ __forceinline__ T* kv(T* base, int64_t i, int which) const { return base + i * ld + (1 + which) * H * D + h * D; }
    // token i's row of this head in the dq and in the dk third of dqkv (dv: H * D further)
    template <typename T>
    __device__ __forceinline__ T* dq(T* dqkv, int i) const { return dqkv + ((int64_t)b * N + i) * ld + h * D; }
    template <typename T>
    __device__ __forceinline__ T* dk(T* dqkv, int i) const { return dqkv + ((int64_t)b * N + i) * ld + H * D + h * D; }
    template <typename T>
    __device__ __forceinline__ T* out_row(T* out, int i) const { return out_token(out, (int64_t)b * N + i); }
    template <typename T>
    __device__ __forceinline__ T* out_token(T* out, int64_t bi) const { return out + bi * (H * D) + h * D; }  // bi = b N + i
    __device__ __forceinline__ int64_t stat(int i) const { return ((int64_t)b * H + h) * N + i; }  // index into lse / delta
};

// ---- fragments of a staged 64-B-row tile (rows = tokens, 32 elements of 16 bits), in blocks of 32 rows
// A operand of a product over d: row r of block blk of a tile stored in swizzled 16-B chunks (sw64), k step ks, lane half hh
__device__ __forceinline__ bf16x8 attn_row_frag(const unsigned char* tile, int blk, int r, int ks, int hh) {
    return *reinterpret_cast<const bf16x8*>(tile + sw64(blk * 32 + r, 2 * ks + hh));
}
// A operand of a product over the tokens: the transposed fragment (rows = d, k = token 16 s + 8 (j >> 2) + 4 hh + (j & 3)) of
// block blk of a tile stored in plain rows, by transposed LDS reads.  g = lane >> 4, tq = (lane & 15) >> 2, and col, the
// lane's byte column, = (16 (g & 1) + 4 (lane & 3)) * 2
__device__ __forceinline__ bf16x8 attn_tr_frag(const unsigned char* tile, int blk, int s, int g, int tq, int col) {
    const unsigned char* p = tile + (blk * 32 + 16 * s + 4 * (g >> 1) + tq) * 64 + col;
    return tr_frag(p, p + 8 * 64);
}

// Store of a transposed 32 x 32 accumulator tile t[d][row] as 16-bit rows: the lane owns one row of the result, `dst`, of
// D = 32 elements, and its 16 registers are d = acc_row(i, hh).  Piece j of the four 8-byte pieces a lane writes: registers
// 4 j .. 4 j + 3 times `scale`, rounded, to d = 8 j + 4 hh .. + 3.  The callers loop over j (dK / dV alternate their two rows).
template <typename E>
__device__ __forceinline__ void attn_store_row_piece(typename E::T* dst, const f32x16& t, int j, float scale, int hh) {
    const uint2 v = make_uint2(E::pack2(t[4 * j] * scale, t[4 * j + 1] * scale), E::pack2(t[4 * j + 2] * scale, t[4 * j + 3] * scale));
    *reinterpret_cast<uint2*>(dst + 8 * j + 4 * hh) = v;
}
