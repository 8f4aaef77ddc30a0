// Internal interface of the 1x1x1 convolution: the route of a forward call, the plan of a weight gradient, the call records and
// the launchers of the three kernel families.  tdx_conv1.hip holds the entry points of include/tdx.h, route, plan and the
// vector-ALU kernels; tdx_conv1_mfma.hip the 16-bit matrix-core kernels, tdx_conv1_mfma_f32.hip the fp32 ones.
#pragma once
#include "tdx_common.h"
#include "tdx_runtime.h"  // the switches, tdx_deterministic, the ordered sums, the scratch arena

// `add` through a normalisation: with stats != nullptr the addend is silu(GroupNorm(add)) -- the tail of a ResnetBlock
// with a projected skip, y = silu(GN(h2)) + conv1x1(x) (reference ddpm.py:176,197), in ONE pass: the skip tensor is never
// written or re-read.  Same arithmetic as gn_apply_kernel (tdx_groupnorm.hip): n = fma(h, rstd gamma, beta - mean rstd gamma).
struct Conv1GnAdd {
    const float* stats;   // [B][G][2] (mean, rstd), or nullptr: plain addend
    const float* gamma;   // [Cout]
    const float* beta;    // [Cout]
    int G;
    int64_t V;            // voxels per sample (rows = B V)
};

// One forward call: y[r, :] = bias + [x1 | x2][r, :] @ w (+ add[r, :], or + silu(GroupNorm(add))[r, :] with gn.stats)
struct Conv1Call {
    const void* x1; int C1;
    const void* x2; int C2;
    const float* w; int ldw;
    const float* bias;
    const void* add;
    void* y;
    int64_t rows; int Cout;
    int fmt;  // TDX_F32 / TDX_BF16 / TDX_F16: the tensors
    hipStream_t st;
    Conv1GnAdd gn;  // 16-bit matrix-core kernel only (tdx_conv1_fwd_gn)
};

// Which kernel serves a forward call: the ONE place that decides it and the one reader of TDX_CONV1_IMPL (the weight
// gradient's plan asks it too).  family: TDX_CONV1_* of include/tdx.h; nt: output tile in units of 32 channels (vector
// ALU: 0); status: TDX_OK, or what the entry point returns: TDX_EDTYPE for a dtype that is no tensor format, and the fused
// tail (gn_tail) has one kernel: TDX_EDTYPE for fp32 tensors, TDX_ESHAPE under TDX_CONV1_IMPL=direct or for ineligible
// channels.  w_mod16: the address of w modulo 16 (the fp32 kernel stages w with 16-byte loads).  Pure host code.
struct Conv1Route {
    int family, nt, status;
};
#define C1M_ROWS 256  // rows of a forward tile and of a weight-gradient chunk of the 16-bit kernels
#define F1_ROWS 128   // rows of a forward tile of the fp32 kernel
Conv1Route conv1_route(int dtype, int C1, int C2, int Cout, int ldw, unsigned w_mod16, bool gn_tail);
bool conv1_mfma_supported(int C1, int C2, int Cout);
bool conv1_mfma_f32_supported(int C1, int C2, int Cout, int ldw, unsigned w_mod16);

// The launchers: each serves the calls whose route (or plan) names it, TDX_EINVAL for any other; none reads a switch.
int conv1_vector_fwd_launch(const Conv1Call& c, const Conv1Route& r);    // tdx_conv1.hip
int conv1_mfma_fwd_launch(const Conv1Call& c, const Conv1Route& r);      // tdx_conv1_mfma.hip
int conv1_mfma_f32_fwd_launch(const Conv1Call& c, const Conv1Route& r);  // tdx_conv1_mfma_f32.hip

// One weight-gradient call: dw[ci][co] (transposed: dw[co][ci]; row stride ldw) += sum_r x[r, ci] dy[r, co], dbias[co] +=
// sum_r dy[r, co] (nullptr: not wanted).  The kernels only ever add: `accumulate` tells the entry point whether to zero first.
struct Conv1WgradCall {
    const void* x; int Cin;
    const void* dy; int Cout;
    float* dw; int ldw;
    float* dbias;
    int64_t rows;
    bool transposed, accumulate;
    int fmt;
    hipStream_t st;
};
// What a weight-gradient call launches: made once per call by conv1_wgrad_plan from the shape, TDX_DETERMINISTIC and the
// arena's size; read by the launchers, reported by tdx_conv1_bwd_weight_plan (include/tdx.h).
struct Conv1WgradPlan {
    int kernel;              // TDX_CONV1_*
    int mt, nt;              // tile in units of 32 channels: (ci, co) on the 16-bit kernel, co on the fp32 one; vector ALU: 0
    int nsplit;              // splits of the rows, each a contributor to every element it covers
    int step_rows;           // rows per loop trip: 256 on the 16-bit kernel, 32 on the other two
    int64_t rows_per_split;  // split s reduces rows [s, s + 1) * rows_per_split; 0: the step_rows-chunks s, s + nsplit, ...
    // TDX_DETERMINISTIC with an arena of two slabs or more: split s adds into the zeroed slab s ([nrow][ncol] compact, then
    // the bias gradient: ONE contributor per element), the slabs are then added in order into dw / dbias.  nslab = 0: the
    // splits merge with atomics into dw (TDX_DETERMINISTIC without such an arena: one split)
    int nslab;
    int64_t slab_stride;     // floats per slab; 0 with nslab = 0
    int status;              // TDX_OK, or TDX_EDTYPE for a dtype that is no tensor format
};
Conv1WgradPlan conv1_wgrad_plan(int dtype, int Cin, int Cout, int64_t rows);
// The split rule of each kernel: fills kernel, mt, nt, nsplit, step_rows, rows_per_split.  max_split > 0: at most that many.
bool conv1_wgrad_mfma_supported(int Cin, int Cout);
bool conv1_wgrad_mfma_f32_supported(int Cin, int Cout);
void conv1_wgrad_vector_plan(Conv1WgradPlan& p, int64_t rows, int max_split);
void conv1_wgrad_mfma_plan(Conv1WgradPlan& p, int Cin, int Cout, int64_t rows, int max_split);
void conv1_wgrad_mfma_f32_plan(Conv1WgradPlan& p, int Cin, int Cout, int64_t rows, int max_split);
// c.dw / c.ldw / c.dbias: where split 0 adds (the block itself, or slab 0); split s adds p.slab_stride * s floats further
int conv1_wgrad_vector_launch(const Conv1WgradCall& c, const Conv1WgradPlan& p);
int conv1_wgrad_mfma_launch(const Conv1WgradCall& c, const Conv1WgradPlan& p);
int conv1_wgrad_mfma_f32_launch(const Conv1WgradCall& c, const Conv1WgradPlan& p);
