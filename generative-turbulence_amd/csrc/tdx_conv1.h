// Launchers of the matrix-core 1x1x1 convolution kernels, as tdx_conv1.hip (the entry points and the vector-ALU kernels)
// calls them.  Each serves the shapes its *_supported accepts.
#pragma once
#include "tdx_common.h"

// 16-bit tensors (tdx_conv1_mfma.hip); hf: IEEE half instead of bfloat16.  gn_stats != nullptr: the addend is
// silu(GroupNorm(add)) with these statistics and parameters (tdx_conv1_fwd_gn)
bool conv1_mfma_supported(int C1, int C2, int Cout);
int conv1_mfma_fwd_launch(const void* x1, int C1, const void* x2, int C2, const float* w, int ldw, const float* bias,
                          const void* add, void* y, int64_t rows, int Cout, hipStream_t st, const float* gn_stats = nullptr,
                          const float* gn_gamma = nullptr, const float* gn_beta = nullptr, int gn_groups = 1,
                          int64_t gn_voxels = 1, bool hf = false);
bool conv1_wgrad_mfma_supported(int Cin, int Cout);
// max_split / split_stride (TDX_DETERMINISTIC): at most max_split K splits (0 = the launcher's own choice), split k adds into
// dw + k * split_stride (and dbias + k * split_stride): zeroed slabs with ONE contributor per element, summed in order afterwards;
// plan_only: report the number of splits the launch would use (nsplit_out) without launching
int conv1_wgrad_mfma_launch(const void* x, int Cin, const void* dy, int Cout, float* dw, int ldw, float* dbias,
                            int64_t rows, bool transposed, hipStream_t st, bool hf = false, int max_split = 0,
                            int64_t split_stride = 0, int* nsplit_out = nullptr, bool plan_only = false);
// fp32 tensors, fp32-IEEE products (tdx_conv1_mfma_f32.hip)
bool conv1_mfma_f32_supported(int C1, int C2, int Cout, const float* w, int ldw);
int conv1_mfma_f32_fwd_launch(const void* x1, int C1, const void* x2, int C2, const float* w, int ldw, const float* bias,
                              const void* add, void* y, int64_t rows, int Cout, hipStream_t st);
bool conv1_wgrad_mfma_f32_supported(int Cin, int Cout);
int conv1_wgrad_mfma_f32_launch(const void* x, int Cin, const void* dy, int Cout, float* dw, int ldw, float* dbias,
                                int64_t rows, bool transposed, hipStream_t st, int max_split = 0, int64_t split_stride = 0,
                                int* nsplit_out = nullptr, bool plan_only = false);
