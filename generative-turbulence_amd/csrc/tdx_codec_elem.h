// The element of the 4 -> dim encoders and of the dim -> 4 decoder, written once for the codec kernels (tdx_codec.hip:
// encode_fwd_kernel, decode_fwd_kernel) and for the GroupNorm tails that evaluate it in place (tdx_groupnorm.hip:
// gn_apply_encoded_kernel, gn_apply_decode_kernel).
//
// include/tdx.h promises  tdx_gn_apply_encoded == tdx_encode_fwd + tdx_gn_apply(res = its output)  and
// tdx_gn_apply_decode == tdx_gn_apply(res, act = 1) + tdx_decode_fwd, bit for bit.  Both hold because the two sides call
// the functions below: explicit FMA chains in a fixed order (no contraction left to the compiler), the same butterfly, and
// round_as<T> wherever the unfused pair would have stored a T tensor in between.
#pragma once
#include "tdx_common.h"

// a rounded to T's precision: what a T tensor would have held
template <typename T> __device__ __forceinline__ float round_as(float a);
template <> __device__ __forceinline__ float round_as<float>(float a) { return a; }
template <> __device__ __forceinline__ float round_as<bf16>(float a) { return __uint_as_float(pack_bf16x2(a, 0.f) << 16); }
template <> __device__ __forceinline__ float round_as<f16>(float a) { return (float)(_Float16)a; }

// Encoder lane: channels [8 lc, 8 lc + 8) of cat(Wx x[b] + bx, Wc c + bc); the lane lies in the x half iff 8 lc < D.
template <int F>
struct EncLane {
    struct In { float v[F]; };  // one voxel of the lane's F raw planes
    const float* src;           // plane 0 of those: x of sample b, or c (shared by the batch)
    float w[8][F], bias[8];
    __device__ __forceinline__ EncLane(int lc, int b, int D, int64_t V, const float* __restrict__ x, const float* __restrict__ wx,
                                       const float* __restrict__ bx, const float* __restrict__ c, const float* __restrict__ wc,
                                       const float* __restrict__ bc) {
        const bool is_x = lc * 8 < D;
        const int ch0 = is_x ? lc * 8 : lc * 8 - D;
        const float* wp = is_x ? wx : wc;
        const float* bp = is_x ? bx : bc;
        src = is_x ? x + (int64_t)b * F * V : c;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bias[j] = bp[ch0 + j];
#pragma unroll
            for (int k = 0; k < F; ++k) w[j][k] = wp[(ch0 + j) * F + k];
        }
    }
    __device__ __forceinline__ In load(int64_t V, int64_t v) const {
        In in;
#pragma unroll
        for (int k = 0; k < F; ++k) in.v[k] = src[(int64_t)k * V + v];
        return in;
    }
    __device__ __forceinline__ float eval(int j, const In& in) const {  // channel j of the lane
        float a = bias[j];
#pragma unroll
        for (int k = 0; k < F; ++k) a = __builtin_fmaf(w[j][k], in.v[k], a);
        return a;
    }
};

// Decoder lane: its 8 channels' share of y[f] = sum_c W[f][c] h[c] + bias[f].  The L = C / 8 lanes of a voxel are adjacent
// in a wave (L a power of two <= 64, checked by the host) and ALL of them must call dot(): it ends in a butterfly over them.
template <int F>
struct DecLane {
    float w[F][8], bias[F];
    __device__ __forceinline__ DecLane(int lc, int C, const float* __restrict__ wp, const float* __restrict__ bp) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            bias[f] = bp[f];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[f][j] = wp[f * C + lc * 8 + j];
        }
    }
    __device__ __forceinline__ float dot(int f, const float (&h)[8], int L) const {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) t = __builtin_fmaf(w[f][j], h[j], t);
        for (int q = 1; q < L; q <<= 1) t += __shfl_xor(t, q, 64);
        return t + bias[f];
    }
};
