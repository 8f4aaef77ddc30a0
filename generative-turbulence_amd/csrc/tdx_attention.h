// Interface of the attention family: what the two matrix-core files (tdx_attention_mfma.hip forward,
// tdx_attention_bwd_mfma.hip backward) share on the device, and their launchers as tdx_attention.hip (the entry points and
// the vector-ALU kernels) calls them.
#pragma once
#include "tdx_common.h"
#include "tdx_mfma.h"

#define FA_D 32  // head dimension of the matrix-core kernels

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

// Store of a transposed 32 x 32 accumulator tile t[d][row] as 16-bit rows: the lane owns one row of the result, `dst`, of
// D = 32 elements, and its 16 registers are d = acc_row(i, hh).  Piece j of the four 8-byte pieces a lane writes: registers
// 4 j .. 4 j + 3 times `scale`, rounded, to d = 8 j + 4 hh .. + 3.  The callers loop over j (dK / dV alternate their two rows).
template <typename E>
__device__ __forceinline__ void attn_store_row_piece(typename E::T* dst, const f32x16& t, int j, float scale, int hh) {
    const uint2 v = make_uint2(E::pack2(t[4 * j] * scale, t[4 * j + 1] * scale), E::pack2(t[4 * j + 2] * scale, t[4 * j + 3] * scale));
    *reinterpret_cast<uint2*>(dst + 8 * j + 4 * hh) = v;
}

// tdx_attention_mfma.hip
bool attn_mfma_supported(int N, int D);
int attn_fwd_mfma_launch(const void* qkv, void* out, float* lse, int B, int N, int H, int dtype, hipStream_t st);
// tdx_attention_bwd_mfma.hip
int attn_bwd_mfma_launch(const void* qkv, const void* dout, const float* lse, const float* delta, void* dqkv, int B, int N,
                         int H, int dtype, hipStream_t st);
