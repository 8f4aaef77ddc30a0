// The activation family of the GroupNorm tails (TDX_ACT_* of include/tdx.h), written once: Act<ACT>::f(n), its derivative
// df(n), and f_add(n, r) = f(n) + r.  The definitions are those of torch's nn.SiLU / nn.GELU / nn.ReLU / nn.Softplus / nn.Tanh
// at their default arguments.  GELU's erf and Tanh are the device library's, everything else is built from the hardware
// exp2 / log2 / rcp (1 ulp each) like sigmoid_f; the instruction sequences below are what tests/act_reference.py derives
// its error bounds from -- change one and the derivation there changes with it.
#pragma once
#include "tdx_common.h"

#define TDX_ACT_COUNT 6  // valid codes are [0, TDX_ACT_COUNT)

template <int ACT>
struct Act;

template <>
struct Act<TDX_ACT_NONE> {
    static __device__ __forceinline__ float f(float n) { return n; }
    static __device__ __forceinline__ float df(float) { return 1.0f; }
    static __device__ __forceinline__ float f_add(float n, float r) { return n + r; }
};

// SiLU: silu_f / dsilu_f of tdx_common.h.  silu(n) + r is ONE explicit fma: the three tail kernels (apply / apply_encoded /
// apply_decode) promise bit-identical results, which must not hinge on the compiler contracting n * sigmoid(n) + r the same
// way in each
template <>
struct Act<TDX_ACT_SILU> {
    static __device__ __forceinline__ float f(float n) { return silu_f(n); }
    static __device__ __forceinline__ float df(float n) { return dsilu_f(n); }
    static __device__ __forceinline__ float f_add(float n, float r) { return __builtin_fmaf(n, sigmoid_f(n), r); }
};

// GELU (approximate = "none"): n/2 (1 + erf(n / sqrt 2)) as one fma on h = n/2 (exact); erff is the device library's.
// f'(n) = Phi(n) + n phi(n), phi(n) = exp(-n^2 / 2) / sqrt(2 pi) on the hardware exp2.
template <>
struct Act<TDX_ACT_GELU> {
    static __device__ __forceinline__ float erf_arg(float n) { return erff(n * 0.70710678118654752f); }
    static __device__ __forceinline__ float f(float n) {
        const float h = 0.5f * n;
        return __builtin_fmaf(h, erf_arg(n), h);
    }
    static __device__ __forceinline__ float df(float n) {
        const float Phi = __builtin_fmaf(0.5f, erf_arg(n), 0.5f);
        const float q = __builtin_amdgcn_exp2f((n * n) * -0.72134752044448170f);  // exp(-n^2 / 2)
        return __builtin_fmaf(n * 0.39894228040143268f, q, Phi);
    }
    static __device__ __forceinline__ float f_add(float n, float r) { return f(n) + r; }
};

// ReLU: exact.  f'(0) = 0, as torch.
template <>
struct Act<TDX_ACT_RELU> {
    static __device__ __forceinline__ float f(float n) { return n > 0.0f ? n : 0.0f; }
    static __device__ __forceinline__ float df(float n) { return n > 0.0f ? 1.0f : 0.0f; }
    static __device__ __forceinline__ float f_add(float n, float r) { return f(n) + r; }
};

// Softplus (beta = 1, threshold = 20): n > 20 ? n : log(1 + e^n), evaluated as max(n, 0) + log(1 + e^-|n|) so that neither
// term overflows or cancels.  f'(n) = n > 20 ? 1 : sigmoid(n).
template <>
struct Act<TDX_ACT_SOFTPLUS> {
    static __device__ __forceinline__ float f(float n) {
        const float w = __builtin_amdgcn_exp2f(-1.4426950408889634f * __builtin_fabsf(n));
        // v_log_f32 is log2; ONE explicit fma, so that the tails' bit-identity does not hinge on contraction
        const float s = __builtin_fmaf(__builtin_amdgcn_logf(1.0f + w), 0.69314718055994531f, __builtin_fmaxf(n, 0.0f));
        return n > 20.0f ? n : s;
    }
    static __device__ __forceinline__ float df(float n) { return n > 20.0f ? 1.0f : sigmoid_f(n); }
    static __device__ __forceinline__ float f_add(float n, float r) { return f(n) + r; }
};

// Tanh: the device library's tanhf -- the function torch's nn.Tanh evaluates, so that f'(n) = 1 - tanh^2 n, one fma of the
// recomputed t, is the derivative autograd forms from its saved output.  (From the hardware exp2 / rcp, as
// sign(n) (1 - w) / (1 + w) with w = e^(-2 |n|), tanh costs 7 instructions instead of 23, but errs by up to 5 u ABSOLUTE where
// tanhf errs by 1-2 ulp: the per-channel sums of the backward over f32 tensors came out up to twice as far from float64 as
// those of the torch module.  The pass stays bound by HBM either way.)
template <>
struct Act<TDX_ACT_TANH> {
    static __device__ __forceinline__ float f(float n) { return tanhf(n); }
    static __device__ __forceinline__ float df(float n) {
        const float t = tanhf(n);
        return __builtin_fmaf(-t, t, 1.0f);
    }
    static __device__ __forceinline__ float f_add(float n, float r) { return f(n) + r; }
};

// activation dispatch for launchers: runs the statement with `constexpr int NAME`; any other code is a bad argument
#define TDX_DISPATCH_ACT(act, NAME, ...)                                                    \
    do {                                                                                    \
        switch (act) {                                                                      \
            case TDX_ACT_NONE: { constexpr int NAME = TDX_ACT_NONE; __VA_ARGS__; } break;         \
            case TDX_ACT_SILU: { constexpr int NAME = TDX_ACT_SILU; __VA_ARGS__; } break;         \
            case TDX_ACT_GELU: { constexpr int NAME = TDX_ACT_GELU; __VA_ARGS__; } break;         \
            case TDX_ACT_RELU: { constexpr int NAME = TDX_ACT_RELU; __VA_ARGS__; } break;         \
            case TDX_ACT_SOFTPLUS: { constexpr int NAME = TDX_ACT_SOFTPLUS; __VA_ARGS__; } break; \
            case TDX_ACT_TANH: { constexpr int NAME = TDX_ACT_TANH; __VA_ARGS__; } break;         \
            default: return TDX_EINVAL;                                                     \
        }                                                                                   \
    } while (0)
