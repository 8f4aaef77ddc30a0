// Launchers of the matrix-core general-convolution kernels (tdx_convg_mfma.hip; bf16 tensors), as tdx_convg.hip and
// tdx_convg_chain.hip call them.  Ei / Eo: input / output grid; the other arguments as in include/tdx.h.
#pragma once
#include "tdx_common.h"

int convg_mfma_apply(const void* in, const float* w, const float* bias, void* out, int B, const int* Ei, const int* Eo, int Cin,
                     int Cout, int k, int stride, int dil, int pad, int replicate, int transposed, hipStream_t st);
// gather form (stride 1) with a fused epilogue: the caller (tdx_convg_apply_fused) has checked the options
int convg_mfma_apply_epilogue(const void* in, const float* w, const float* bias, void* out, int B, const int* Ei, const int* Eo,
                              int Cin, int Cout, int k, int dil, int pad, int replicate, const TdxConvgEpilogue* ep, hipStream_t st);
int convg_mfma_bwd_weight(const void* in, const void* dy, float* dw, float* dbias, int B, const int* Ei, const int* Eo, int Cin,
                          int Cout, int k, int stride, int dil, int pad, int replicate, hipStream_t st);
