// Internal interface of the 3x3x3 convolution: the route (which kernel serves a call), the call records the launchers
// take, and the launchers of every kernel family.  tdx_conv3_entry.hip holds the entry points of include/tdx.h and the
// route; tdx_conv3_direct.hip weight packing and the vector-ALU kernels; every other tdx_conv3_*.hip one kernel family.
#pragma once
#include "tdx_common.h"
#include "tdx_runtime.h"  // tdx_deterministic, the ordered sums, tdx_persistent_cus, the scratch arena

struct Conv3Geom {
    int B;
    int Xi, Yi, Zi;  // input grid
    int Xo, Yo, Zo;  // output grid
    int off;         // output voxel o reads input voxel o + off + e, e in {-1,0,1}^3
};

// Packed-operand layouts (element index of weight (tap, k, n); K = input channels of the
// conv being evaluated, N = its output channels):
//   generic : (tap*K + k)*N + n                                   [27][K][N]
//   mfma    : (((k/kc)*27 + tap)*N + n)*kc + (k%kc)               [K/kc][27][N][kc]
// with kc = 16 for bf16 iff conv3_mfma_supported(K, 0, N), kc = 8 for fp32 iff
// conv3_mfma_f32_supported(K, 0, N), else the generic layout (kc = 0) -- a function of (dtype, K, N)
// only, so that pack and consumers agree without carrying a flag through the ABI.
bool conv3_mfma_supported(int C1, int C2, int Cout);
bool conv3_mfma_f32_supported(int C1, int C2, int Cout);
static inline int conv3_layout_kc(int dtype, int K, int N) {
    if (dtype == 1 || dtype == 3) return conv3_mfma_supported(K, 0, N) ? 16 : 0;  // TDX_BF16, TDX_F16: one layout
    return conv3_mfma_f32_supported(K, 0, N) ? 8 : 0;
}
static inline bool conv3_uses_mfma_layout(int dtype, int K, int N) { return (dtype == 1 || dtype == 3) && conv3_mfma_supported(K, 0, N); }
bool conv3_mfma_split_supported(int C1, int C2, int Cout);

// optional extras of the MFMA forward: input row strides (0: dense) and a tensor the accumulators
// start from ([B][V][Cout] bf16, or [V][Cout] shared by the batch)
struct Conv3Ext {
    int ld1, ld2;
    const void* init;
    bool init_shared;
};

// One forward or data-gradient call, as every launcher below takes it.  Forward: y = conv3([x1 | x2]) + bias with N output
// channels.  Data gradient (zero_pad): x1 = dy (C2 = 0), wp = the data-gradient operand, the N result channels are split
// over d1 (channels [0, D1)) and d2, each plus its addend a1 / a2 where given.
struct Conv3Call {
    const void* x1; int C1;
    const void* x2; int C2;
    const void* wp;          // packed operand in the layout of `fmt` (tdx_conv3_pack_weight)
    const float* bias;
    void* y;                 // forward result; vector-ALU data gradient: the padded workspace
    int B, X, Y, Z, N;
    bool zero_pad;           // sources outside the grid read zero (data gradient) instead of the clamped voxel
    double* gn_acc;          // forward: per-channel f64 moments are added here (tdx_conv3_fwd_gn)
    void* d1; int D1; void* d2;
    const void* a1; const void* a2;
    // conv3_ring_launch only, data gradient of a block with a projected 1x1 skip: d1 | d2 += skip_x [voxel][C1] . skip_w [C1][N]
    // (f32) inside the kernel (conv3_ring_skip_supported says when)
    const void* skip_x; const float* skip_w;
    hipStream_t st;
    int fmt;                 // TDX_BF16 / TDX_F16 / TDX_F32 / TDX_F32_SPLIT: tensors and operand (split: fp32 tensors)
    const Conv3Ext* ext;     // conv3_mfma_launch only
    // conv3_mfma_launch only: {mx, my, mz} = another kernel has computed the region [0, mx) x [0, my) x [0, mz) of the
    // output; launch only the thin-brick kernel on the remainder slabs beyond it (1-2 voxels thick per axis)
    const int* slabs_beyond;
    // TDX_F16: the tensors and the packed operand are IEEE half instead of bfloat16: same kernels, same layouts,
    // v_mfma_f32_32x32x16_f16 and half rounding of the results (H16<HF>, tdx_common.h)
    bool hf() const { return fmt == TDX_F16; }
    Conv3Geom geom() const { return Conv3Geom{B, X, Y, Z, X, Y, Z, 0}; }
};

// launch geometry of the small-grid kernel (tdx_conv3_small_kernel.h)
struct SmallGeom {
    int B;
    int Ev[3];     // virtual grid (rows)
    int Es[3];     // source grid
    int off;       // source coordinate = virtual coordinate - off
    int clamp;     // 1: clamp sources into the grid (forward), 0: zero outside (data gradient)
    int nbg;       // samples per row group (1 when a sample is cut into x slabs)
    int xs;        // virtual x planes per row group
    int gx;        // x slabs per sample
    int Ix, Iy, Iz;  // LDS image per sample of a group: (xs + 2) x (Ev[1] + 2) x (Ev[2] + 2) entries
    int K, N;      // channels of the source tensor(s) / of the result
    int per_split; // K slices per split
    int nsplit;
};
struct Conv3SmallPlan {
    SmallGeom g;
    size_t lds;
    int mtw;  // M tiles per wave
};

// Which kernel serves a call: the ONE place that decides it.  fmt: the arithmetic and operand layout (TDX_BF16 / TDX_F16:
// 16-bit MFMA, TDX_F32: fp32-IEEE MFMA, TDX_F32_SPLIT: split-precision MFMA; with family TDX_KERNEL_DIRECT the tensors'
// dtype, on the vector ALU).  family: TDX_KERNEL_* of include/tdx.h.  status: TDX_OK, or what the entry point returns for
// this combination (family is then what tdx_conv3_fwd_kernel reports).  The plan of the chosen family rides along, so
// that "would this launcher take the call" and the launch itself are one computation.
struct Conv3Route {
    int fmt, family, status;
    int ring_depth;        // TDX_KERNEL_RING: 8- or 4-deep bricks
    Conv3SmallPlan small;  // TDX_KERNEL_SMALL
};
// C1 | C2: channels of the conv's inputs, N of its result (data gradient: C1 = Cout, C2 = 0, N = Cin); impl: TDX_CONV_*
// (flag bits above 0xff are ignored).  Pure host code: reads the environment switches and the arena's size, launches nothing.
Conv3Route conv3_route(int dtype, int impl, int C1, int C2, int N, int B, int X, int Y, int Z, bool data_gradient);

// The launchers.  Each serves the calls the route gives it and returns an error for any other: none is a fall-through.
// brick kernels: 16-bit (tdx_conv3_mfma.hip), split-precision (tdx_conv3_mfma_split.hip), fp32-IEEE (tdx_conv3_mfma_f32.hip)
int conv3_mfma_launch(const Conv3Call& c);
int conv3_mfma_split_launch(const Conv3Call& c);
int conv3_mfma_f32_launch(const Conv3Call& c);
// vector-ALU kernel (tdx_conv3_direct.hip); zero_pad: the adjoint on the padded grid (X + 2)(Y + 2)(Z + 2) into c.y
int conv3_direct_launch(const Conv3Call& c);
// halo fold of that adjoint (the same call): d1 | d2 = fold(c.y) (+ a1 | a2)
int conv3_fold_launch(const Conv3Call& c);

// persistent LDS-DMA ring kernel (tdx_conv3_ring.hip; 16-bit): forward or main term of the data gradient on grids whose
// whole 8 x 8 x 8 (or 4-deep) bricks fill the chip and leave remainders of at most 2 voxels per axis (those go to the
// thin-brick kernel of tdx_conv3_mfma.hip in a second launch: the reference's 194 x 50 x 50 and its 97 x 25 x 25 level).
// Results equal the brick kernel's up to the fp32 summation order: ~1 bf16 ulp on a few % of the elements.
// conv3_ring_depth: brick depth the kernel would run this call with, 0 = not a case for it (the data gradient also needs
// the arena's zero block)
int conv3_ring_depth(int C1, int C2, int N, int B, int X, int Y, int Z, bool data_gradient);
int conv3_ring_launch(const Conv3Call& c, int depth);
// may the data gradient (K channels of dy -> N of dx) on bricks of this depth carry the skip term of Conv3Call::skip_x?
// Reads TDX_SKIP_DGRAD_FUSE (0: never) and TDX_RING_LOADERS per call.
bool conv3_ring_skip_supported(int fmt, int depth, int K, int N, int X, int Y, int Z);

// small-grid conv (tdx_conv3_small.hip; 16-bit tensors, or fp32 tensors with split-precision products): forward or data
// gradient (halo fold included).  Needs the scratch arena.  conv3_small_plan: false = not a small-grid case.
bool conv3_small_plan(Conv3SmallPlan& p, int C1, int C2, int N, int B, int X, int Y, int Z, bool data_gradient, bool split);
int conv3_small_launch(const Conv3Call& c, const Conv3SmallPlan& p);

// One weight-gradient call: dwp [27][Cin][Cout] (+)= x^T dy, dbias (+)= column sums of dy (nullptr: not wanted).
// slabs: region of the plan's max_slabs x 27*Cin*Cout floats (max_slabs = 0: none, slabs is not read); when the plan uses at
// most max_slabs K-splits every split stores its partial tiles there (no atomics) and the plan's nslab tells the caller how
// many slabs to add up (0: the result was accumulated into dwp).  The plan functions read the shape (C1, C2, Cout, B, X, Y, Z) only.
struct Conv3WgradCall {
    const void* x1; int C1;
    const void* x2; int C2;
    const void* dy;
    float* dwp;
    float* dbias;
    int B, X, Y, Z, Cout;
    hipStream_t st;
    float* slabs;
    bool hf;
};
// What a weight-gradient call launches: the ONE decision, made on the host by conv3_wgrad_plan (tdx_conv3_entry.hip) from the
// per-kernel plan functions below, read by the launchers and reported by tdx_conv3_bwd_weight_plan (include/tdx.h).
struct Conv3WgradPlan {
    int kernel;      // TDX_WGRAD_* of include/tdx.h
    int status;      // TDX_OK, or what tdx_conv3_bwd_weight returns for the call (kernel is then TDX_WGRAD_DIRECT)
    int nt;          // output tile in units of 32 channels (NT / NTN: 1 or 2); vector-ALU kernel: 0
    int depth;       // brick depth along the kernel's local x (4 or 2); packed-K and vector-ALU kernels: 0
    int nsplit;      // K splits launched (vector-ALU kernel: voxel chunks)
    int nslab;       // slabs the unpack adds up; 0: fp32 atomics into dwp
    int sum_unpack;  // 1: conv3_unpack_sum_kernel (more slabs than the tiled unpack walks)
    int max_slabs;   // slabs the call may use (the capacity the plan function was given)
    int nbricks;     // bricks of the grid (brick kernels)
    int order;       // brick kernels: the axis order of their view of the grid (WGRAD_ORDERS, tdx_conv3_wgrad.h)
    // packed-K kernel: samples per row group, x planes per group, x slabs per sample, row groups; bytes of one x image buffer,
    // dy rows per buffer and the dynamic LDS of the launch
    int nbg, xs, gx, ngroups, xbytes, grows, lds;
};
// The merge rule of the MFMA kernels: a launch of nsplit K-splits stores per-split slabs (every (tile, split) pair stores its
// whole partial tile, so the slabs need no zeroing) when the workspace holds that many, else merges with atomics into dwp.
// TDX_DETERMINISTIC: never the atomic merge -- nsplit is held to the slabs the workspace has (added in order by the unpack
// kernel).
static inline void conv3_wgrad_plan_merge(Conv3WgradPlan& p, int nsplit, int max_slabs) {
    if (tdx_deterministic() && nsplit > max_slabs) nsplit = max_slabs > 0 ? max_slabs : 1;
    p.nsplit = nsplit;
    p.nslab = nsplit <= max_slabs ? nsplit : 0;
    p.max_slabs = max_slabs;
}
// where the launch of plan p puts its partial tiles: the base (slabs or dwp) and the slab stride (0: atomics into dwp)
static inline float* conv3_wgrad_out(const Conv3WgradCall& c, const Conv3WgradPlan& p, int64_t& slab_stride) {
    slab_stride = p.nslab ? (int64_t)27 * (c.C1 + c.C2) * c.Cout : 0;
    return p.nslab ? c.slabs : c.dwp;
}
// The seven weight-gradient kernels.  16-bit tensors: the packed-K kernel for small grids on the deep U-Net levels
// (tdx_conv3_wgrad_small.hip), the producer / consumer form on the fine levels (tdx_conv3_wgrad_ring.hip: 8 computing + 4
// loader waves per workgroup, 64- and 32-wide output tiles), else the brick kernel (tdx_conv3_wgrad_mfma.hip).  fp32
// tensors: split-precision (tdx_conv3_wgrad_mfma_split.hip, after its producer / consumer form
// tdx_conv3_wgrad_split_ring.hip: 2 x 8 x 8 bricks) or fp32-IEEE products (tdx_conv3_wgrad_mfma_f32.hip).  Any shape and
// dtype: the vector ALU (tdx_conv3_direct.hip).
// *_plan: pure host code (the shape of c, the slab capacity max_slabs, the environment switches, whether an arena is bound):
// true and p filled when the call is a case for that kernel.  *_launch(c, p): the launch of a plan its own *_plan made; it
// reads no switch and repeats no decision -- tile width, axis order, K splits, slabs and the packed-K kernel's row groups
// all come from p.
// What the brick kernels among them share on the device, and their launch geometry (WgradView, conv3_wgrad_view):
// tdx_conv3_wgrad.h.
bool conv3_wgrad_mfma_supported(int C1, int C2, int Cout);
bool conv3_wgrad_mfma_split_supported(int C1, int C2, int Cout);
bool conv3_wgrad_mfma_f32_supported(int C1, int C2, int Cout);
bool conv3_wgrad_mfma_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
bool conv3_wgrad_small_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
bool conv3_wgrad_ring_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
bool conv3_wgrad_mfma_split_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
bool conv3_wgrad_split_ring_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
bool conv3_wgrad_mfma_f32_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
int conv3_wgrad_mfma_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p);
int conv3_wgrad_small_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p);
int conv3_wgrad_ring_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p);
int conv3_wgrad_mfma_split_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p);
int conv3_wgrad_split_ring_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p);
int conv3_wgrad_mfma_f32_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p);
// vector-ALU weight gradient (tdx_conv3_direct.hip), atomics into dwp; max_slabs > 0 (deterministic runs): at most that many
// voxel chunks, chunk k stores into slab k
bool conv3_wgrad_direct_plan(Conv3WgradPlan& p, const Conv3WgradCall& c, int max_slabs);
int conv3_wgrad_direct_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p, int dtype);
// after the launch of plan p: dwp [27][Cin][Cout] (or the sum of its p.nslab slabs) -> dw (Cout, Cin, 27); the bias-gradient
// accumulator dbw -> dbias.  The accumulators are left all-zero.  p.sum_unpack: the per-tap summing kernel for more slabs
// than the tiled one walks.
int conv3_unpack_wgrad_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p, float* dw, float* dbw, float* dbias);
// The whole decision for one call of tdx_conv3_bwd_weight (impl: TDX_CONV_*, flag bits above 0xff are ignored): which kernel,
// its plan, the slab capacity it is given (p.max_slabs), which unpack.
Conv3WgradPlan conv3_wgrad_plan(int dtype, int impl, int C1, int C2, int Cout, int B, int X, int Y, int Z);

// halo-shell term of the data gradient, added onto dx with atomics (tdx_conv3_shell.hip); mode 0 bf16, 1 fp32 MFMA,
// 2 split-precision, 3 fp16; wb = the packed data-gradient operand for (K -> N) in that mode's layout
// sbuf: conv3_shell_buffer_bytes() of scratch, used when TDX_SHELL_DETERMINISTIC=1 (positions stored, then folded in a
// fixed order by a second kernel, instead of atomics on edge / corner voxels); nullptr: always the atomics route
size_t conv3_shell_buffer_bytes(int B, int X, int Y, int Z, int N);
int conv3_shell_launch(const void* dy, const void* wb, void* d1, int D1, void* d2, int B, int X, int Y, int Z, int K, int N,
                       int mode, hipStream_t st, void* sbuf = nullptr);

// tdx_groupnorm.hip: (mean, rstd) per (b, group) from per-channel f64 (sum, sumsq)
#define TDX_GN_REPLICAS 32  // == GN_REPLICAS in tdx_groupnorm.hip (sizes tdx_gn_workspace_bytes)
int gn_finalize_launch(double* acc, float* stats, int B, int C, int G, int64_t V, float eps, int replicas,
                       hipStream_t st);
// tdx_gn_stats with the TDX_WS_CLEAN promise passed through (tdx_groupnorm.hip)
int gn_stats_launch(const void* x, float* stats, int B, int64_t V, int C, int G, float eps, int dtype, void* workspace,
                    bool clean, hipStream_t stream);
