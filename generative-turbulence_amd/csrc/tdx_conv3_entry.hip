// 3x3x3 convolution: the entry points of include/tdx.h and the route that says which kernel serves a call.  Host code only.  The kernels and their launchers: tdx_conv3_direct.hip (weight packing, vector ALU),
// tdx_conv3_mfma*.hip (brick kernels), tdx_conv3_small*.hip, tdx_conv3_ring.hip, tdx_conv3_shell.hip (halo shell of the
// data gradient), tdx_conv3_wgrad_*.hip (weight gradient); their interface: tdx_conv3.h.
#include "tdx_common.h"
#include "tdx_conv3.h"
#include <stdlib.h>
#include <algorithm>

// ------------------------------------------------------------------ route ----------------
Conv3Route conv3_route(int dtype, int impl, int C1, int C2, int N, int B, int X, int Y, int Z, bool data_gradient) {
    Conv3Route r;
    r.fmt = dtype; r.family = TDX_KERNEL_DIRECT; r.status = TDX_OK; r.ring_depth = 0;
    impl &= 0xff;
    // deep U-Net levels: the small-grid kernel (packed M tiles, split K); else the brick kernel
    auto small_or_brick = [&](bool split) {
        r.family = conv3_small_plan(r.small, C1, C2, N, B, X, Y, Z, data_gradient, split) ? TDX_KERNEL_SMALL : TDX_KERNEL_BRICK;
    };
    if (dtype == TDX_F32 && impl == TDX_CONV_SPLIT && conv3_mfma_split_supported(C1 + C2, 0, N)) {
        r.fmt = TDX_F32_SPLIT;
        // the operand was packed as split images (layout is a function of (K, N)); both inputs must be sliceable
        if (!conv3_mfma_split_supported(C1, C2, N)) { r.family = TDX_KERNEL_BRICK; r.status = TDX_ESHAPE; return r; }
        small_or_brick(true);
    } else if (dtype == TDX_F32 && impl != TDX_CONV_DIRECT && conv3_mfma_f32_supported(C1, C2, N)) {
        r.family = TDX_KERNEL_BRICK;
    } else {
        // the matrix-core kernels of the 16-bit formats (bf16 and fp16 tensors share them: H16<HF>, tdx_common.h); the data
        // gradient of fp32 tensors takes the vector ALU where the forward reports TDX_CONV_MFMA on an unsupported shape
        const bool ok = tdx_is_h16(dtype) && conv3_mfma_supported(C1, C2, N);
        const bool asked = impl == TDX_CONV_MFMA && (tdx_is_h16(dtype) || !data_gradient);
        if (!ok) { r.status = asked ? TDX_ESHAPE : TDX_OK; return r; }
        if (!asked && impl != TDX_CONV_AUTO) return r;
        small_or_brick(false);
        // the two finest levels: persistent LDS-DMA ring kernel (same products, fp32 sums in another order: equal to the brick
        // kernel up to ~1 bf16 ulp on a few % of the elements, tdx_conv3_ring.hip)
        if (r.family == TDX_KERNEL_BRICK && (r.ring_depth = conv3_ring_depth(C1, C2, N, B, X, Y, Z, data_gradient)) != 0)
            r.family = TDX_KERNEL_RING;
    }
    return r;
}

static int conv3_launch(const Conv3Call& c, const Conv3Route& r) {
    switch (r.family) {
        case TDX_KERNEL_SMALL: return conv3_small_launch(c, r.small);
        case TDX_KERNEL_RING: return conv3_ring_launch(c, r.ring_depth);
        case TDX_KERNEL_BRICK:
            if (c.fmt == TDX_F32_SPLIT) return conv3_mfma_split_launch(c);
            return c.fmt == TDX_F32 ? conv3_mfma_f32_launch(c) : conv3_mfma_launch(c);
        default: return conv3_direct_launch(c);
    }
}

// ------------------------------------------------------------------ entry points ---------
static Conv3Call conv3_fwd_call(const void* x1, int C1, const void* x2, int C2, const void* wf, const float* bias, void* y, int B,
                                int X, int Y, int Z, int Cout, int fmt, void* stream) {
    Conv3Call c = {};
    c.x1 = x1; c.C1 = C1; c.x2 = x2; c.C2 = C2; c.wp = wf; c.bias = bias; c.y = y;
    c.B = B; c.X = X; c.Y = Y; c.Z = Z; c.N = Cout;
    c.st = as_stream(stream); c.fmt = fmt;
    return c;
}

extern "C" int tdx_conv3_fwd(const void* x1, int C1, const void* x2, int C2, const void* wf, const float* bias,
                             void* y, int B, int X, int Y, int Z, int Cout, int dtype, int impl, void* stream) {
    TDX_CHECK_ARG(x1 && wf && y && B > 0 && X > 0 && Y > 0 && Z > 0 && C1 > 0 && C2 >= 0 && Cout > 0);
    TDX_CHECK_ARG(C2 == 0 || x2);
    const Conv3Route r = conv3_route(dtype, impl, C1, C2, Cout, B, X, Y, Z, false);
    if (r.status != TDX_OK) return r.status;
    return conv3_launch(conv3_fwd_call(x1, C1, x2, C2, wf, bias, y, B, X, Y, Z, Cout, r.fmt, stream), r);
}

// Which kernel family tdx_conv3_fwd / tdx_conv3_fwd_gn run for this call
extern "C" int tdx_conv3_fwd_kernel(int C1, int C2, int Cout, int B, int X, int Y, int Z, int dtype, int impl) {
    return conv3_route(dtype, impl, C1, C2, Cout, B, X, Y, Z, false).family;
}

extern "C" int tdx_conv3_fwd_gn(const void* x1, int C1, const void* x2, int C2, const void* wf, const float* bias,
                                void* y, float* stats, int G, float eps, void* gn_workspace, int B, int X, int Y, int Z,
                                int Cout, int dtype, int impl, void* stream) {
    TDX_CHECK_ARG(x1 && wf && y && stats && gn_workspace && B > 0 && X > 0 && Y > 0 && Z > 0 && C1 > 0 && C2 >= 0);
    TDX_CHECK_ARG(Cout > 0 && G > 0 && (Cout % G) == 0 && (C2 == 0 || x2));
    const bool clean = (impl & TDX_WS_CLEAN) != 0;
    const Conv3Route r = conv3_route(dtype, impl, C1, C2, Cout, B, X, Y, Z, false);
    if (r.status != TDX_OK) return r.status;
    Conv3Call c = conv3_fwd_call(x1, C1, x2, C2, wf, bias, y, B, X, Y, Z, Cout, r.fmt, stream);
    const int64_t V = (int64_t)X * Y * Z;
    // Unfused, conv and then the statistics pass over its result: the vector-ALU kernels; the small-grid conv (deep U-Net
    // levels, a tiny result); and deterministic runs -- the conv kernels' epilogues merge their moments with f64 atomics in
    // arrival order, the block partials of the statistics pass are exact in f64 (gn_stats_launch)
    if (r.family == TDX_KERNEL_DIRECT || r.family == TDX_KERNEL_SMALL || tdx_deterministic()) {
        int rc = conv3_launch(c, r);
        if (rc != TDX_OK) return rc;
        if (r.family == TDX_KERNEL_DIRECT && !tdx_deterministic())
            return tdx_gn_stats(y, stats, B, V, Cout, G, eps, dtype, gn_workspace, stream);
        return gn_stats_launch(y, stats, B, V, Cout, G, eps, dtype, gn_workspace, clean, c.st);
    }
    // the MFMA brick and ring kernels accumulate the moments in their store loop
    c.gn_acc = (double*)gn_workspace;
    if (!clean) {
        int e = tdx_zero_async(c.gn_acc, (size_t)TDX_GN_REPLICAS * B * Cout * 2 * sizeof(double), c.st);
        if (e != TDX_OK) return e;
    }
    int rc = conv3_launch(c, r);
    if (rc != TDX_OK) return rc;
    return gn_finalize_launch(c.gn_acc, stats, B, Cout, G, V, eps, TDX_GN_REPLICAS, c.st);
}

// Forward with a strided first input and accumulators that start from a precomputed partial
// convolution (bf16 MFMA path only): y = conv3(x1[..., :C1] with row stride ld1, wf) + bias + init.
extern "C" int tdx_conv3_fwd_partial(const void* x1, int C1, int ld1, const void* wf, const float* bias,
                                     const void* init, int init_shared, void* y, float* stats, int G, float eps,
                                     void* gn_workspace, int B, int X, int Y, int Z, int Cout, int dtype, int impl,
                                     void* stream) {
    TDX_CHECK_ARG(x1 && wf && y && B > 0 && X > 0 && Y > 0 && Z > 0 && C1 > 0 && Cout > 0 && ld1 >= C1 && (ld1 % 8) == 0);
    TDX_CHECK_ARG(stats == nullptr || (gn_workspace && G > 0 && (Cout % G) == 0));
    const bool clean = (impl & TDX_WS_CLEAN) != 0;
    // only the brick kernel has the strided / init form: no route to take
    if (!tdx_is_h16(dtype)) return TDX_EDTYPE;
    if (!conv3_mfma_supported(C1, 0, Cout)) return TDX_ESHAPE;
    const bool det = tdx_deterministic();  // then: conv, and the ordered statistics pass over its result (as tdx_conv3_fwd_gn)
    const Conv3Ext ext = {ld1, 0, init, init_shared != 0};
    Conv3Call c = conv3_fwd_call(x1, C1, nullptr, 0, wf, bias, y, B, X, Y, Z, Cout, dtype, stream);
    c.ext = &ext;
    c.gn_acc = (stats && !det) ? (double*)gn_workspace : nullptr;
    if (c.gn_acc && !clean) {
        int e = tdx_zero_async(c.gn_acc, (size_t)TDX_GN_REPLICAS * B * Cout * 2 * sizeof(double), c.st);
        if (e != TDX_OK) return e;
    }
    int rc = conv3_mfma_launch(c);
    if (rc != TDX_OK || !stats) return rc;
    if (det) return gn_stats_launch(y, stats, B, (int64_t)X * Y * Z, Cout, G, eps, dtype, gn_workspace, clean, c.st);
    return gn_finalize_launch(c.gn_acc, stats, B, Cout, G, (int64_t)X * Y * Z, eps, TDX_GN_REPLICAS, c.st);
}

extern "C" size_t tdx_conv3_bwd_data_workspace_bytes(int B, int X, int Y, int Z, int Cin, int dtype, int impl) {
    // the padded tensor of the vector-ALU path (shapes the MFMA kernels do not cover, TDX_CONV_DIRECT); which path a
    // call takes also depends on Cout, so the size is the same for all; the MFMA paths use it only for the position buffer
    // of the deterministic halo-shell route
    (void)impl;
    const size_t padded = (size_t)B * (X + 2) * (Y + 2) * (Z + 2) * Cin * (tdx_is_h16(dtype) ? 2 : 4);
    const size_t shell = conv3_shell_buffer_bytes(B, X, Y, Z, Cin);  // TDX_SHELL_DETERMINISTIC=1: one fp32 row per shell position
    return (padded > shell ? padded : shell) + 256;
}

// dx = adjoint of the replicate-padded conv.  Brick and ring kernels: main term = zero-padded correlation on the original
// grid (the conv kernel, epilogue writes dx incl. the fused addend), then the halo-shell term added by conv3_shell_launch.
// Small-grid kernel: adjoint on the padded grid, halo fold in its reduce pass.  Vector-ALU path: correlation on the
// padded grid into the workspace, then the fold.
// skip_dy / skip_w (tdx_conv3_bwd_data_skip): the skip term rides in the ring kernel's main-term launch; a call the route does
// not give to that kernel variant is refused, never served another way.
static bool conv3_skip_routed(const Conv3Route& r, int Cin, int Cout, int X, int Y, int Z) {
    return r.status == TDX_OK && r.family == TDX_KERNEL_RING && conv3_ring_skip_supported(r.fmt, r.ring_depth, Cout, Cin, X, Y, Z);
}
static int conv3_bwd_data_impl(const void* dy, const void* wb, void* dx1, int C1, void* dx2, int C2, const void* add1,
                               const void* add2, int B, int X, int Y, int Z, int Cout, int dtype, int impl,
                               void* workspace, void* stream, const void* skip_dy = nullptr, const float* skip_w = nullptr) {
    TDX_CHECK_ARG(dy && wb && dx1 && workspace && B > 0 && X > 0 && Y > 0 && Z > 0 && C1 > 0 && C2 >= 0 && Cout > 0);
    TDX_CHECK_ARG(C2 == 0 || dx2);
    const int Cin = C1 + C2;
    if ((C1 % 8) || (C2 % 8) || (Cout % 8)) return TDX_ESHAPE;
    const Conv3Route r = conv3_route(dtype, impl, Cout, 0, Cin, B, X, Y, Z, true);
    if (r.status != TDX_OK) return r.status;
    if (skip_dy != nullptr && !conv3_skip_routed(r, Cin, Cout, X, Y, Z)) return TDX_ESHAPE;
    Conv3Call c = {};
    c.skip_x = skip_dy; c.skip_w = skip_w;
    c.x1 = dy; c.C1 = Cout; c.wp = wb;
    c.B = B; c.X = X; c.Y = Y; c.Z = Z; c.N = Cin;
    c.zero_pad = true;
    c.d1 = dx1; c.D1 = C1; c.d2 = dx2; c.a1 = add1; c.a2 = add2;
    c.st = as_stream(stream); c.fmt = r.fmt;
    if (r.family == TDX_KERNEL_DIRECT) c.y = workspace;
    int rc = conv3_launch(c, r);
    if (rc != TDX_OK || r.family == TDX_KERNEL_SMALL) return rc;
    if (r.family == TDX_KERNEL_DIRECT) return conv3_fold_launch(c);
    const int shell_mode = r.fmt == TDX_F16 ? 3 : (r.fmt == TDX_F32_SPLIT ? 2 : (r.fmt == TDX_F32 ? 1 : 0));
    return conv3_shell_launch(dy, wb, dx1, C1, dx2, B, X, Y, Z, Cout, Cin, shell_mode, c.st, workspace);
}

extern "C" int tdx_conv3_bwd_data(const void* dy, const void* wb, void* dx1, int C1, void* dx2, int C2,
                                  int accumulate, int B, int X, int Y, int Z, int Cout, int dtype, int impl,
                                  void* workspace, void* stream) {
    return conv3_bwd_data_impl(dy, wb, dx1, C1, dx2, C2, accumulate ? dx1 : nullptr, accumulate ? dx2 : nullptr, B, X, Y, Z,
                               Cout, dtype, impl, workspace, stream);
}

extern "C" int tdx_conv3_bwd_data_add(const void* dy, const void* wb, void* dx1, int C1, void* dx2, int C2,
                                      const void* add1, const void* add2, int B, int X, int Y, int Z, int Cout, int dtype,
                                      int impl, void* workspace, void* stream) {
    return conv3_bwd_data_impl(dy, wb, dx1, C1, dx2, C2, add1, add2, B, X, Y, Z, Cout, dtype, impl, workspace, stream);
}

extern "C" int tdx_conv3_bwd_data_skip_supported(int C1, int C2, int Cout, int B, int X, int Y, int Z, int dtype, int impl) {
    if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || C1 <= 0 || C2 < 0 || Cout <= 0 || (C1 % 8) || (C2 % 8) || (Cout % 8)) return 0;
    return conv3_skip_routed(conv3_route(dtype, impl, Cout, 0, C1 + C2, B, X, Y, Z, true), C1 + C2, Cout, X, Y, Z) ? 1 : 0;
}

extern "C" int tdx_conv3_bwd_data_skip(const void* dy, const void* wb, void* dx1, int C1, void* dx2, int C2, const void* skip_dy,
                                       const float* skip_w, int B, int X, int Y, int Z, int Cout, int dtype, int impl,
                                       void* workspace, void* stream) {
    TDX_CHECK_ARG(skip_dy && skip_w);
    return conv3_bwd_data_impl(dy, wb, dx1, C1, dx2, C2, nullptr, nullptr, B, X, Y, Z, Cout, dtype, impl, workspace, stream,
                               skip_dy, skip_w);
}

#define W3_MAX_SLABS 8
// per-split slabs a workspace holds: 8 for the wide layers (few K splits), up to 512 for the narrow ones of the fine
// levels, whose launches split K over 32-512 workgroups -- about 2 MB x 27 of slabs either way
static int w3_slab_capacity(int Cin, int Cout) {
    const int64_t c = ((int64_t)1 << 19) / ((int64_t)Cin * Cout);
    return (int)(c < W3_MAX_SLABS ? W3_MAX_SLABS : (c > 512 ? 512 : c));
}
extern "C" size_t tdx_conv3_bwd_weight_workspace_bytes(int Cin, int Cout, int impl) {
    (void)impl;
    // dw + dbias accumulators (the part covered by TDX_WS_CLEAN), then the partial-sum slabs (scratch, never needs zeroing)
    return (size_t)(1 + w3_slab_capacity(Cin, Cout)) * 27 * Cin * Cout * sizeof(float) + (size_t)Cout * sizeof(float) + 512;
}

// The ONE decision of a weight-gradient call: the kernel family by (dtype, impl, channels), the slab capacity that family is
// given, then the kernels of the family in the order they are asked (each *_plan says whether the call is a case for it),
// and the unpack that follows.  Pure host code: reads the environment switches and whether an arena is bound, launches nothing.
Conv3WgradPlan conv3_wgrad_plan(int dtype, int impl, int C1, int C2, int Cout, int B, int X, int Y, int Z) {
    Conv3WgradPlan p = {};
    p.kernel = TDX_WGRAD_DIRECT;
    auto refuse = [&](int status) { p.status = status; return p; };
    if (!(B > 0 && X > 0 && Y > 0 && Z > 0 && C1 > 0 && C2 >= 0 && Cout > 0)) return refuse(TDX_EINVAL);
    if ((C1 % 8) || (C2 % 8) || (Cout % 8)) return refuse(TDX_ESHAPE);
    impl &= 0xff;
    const int Cin = C1 + C2;
    enum { FAM_DIRECT, FAM_H16, FAM_F32, FAM_SPLIT } fam = FAM_DIRECT;
    if (dtype == TDX_F32 && impl == TDX_CONV_SPLIT && conv3_wgrad_mfma_split_supported(C1, C2, Cout)) {
        fam = FAM_SPLIT;
    } else if (dtype == TDX_F32 && impl != TDX_CONV_DIRECT && conv3_wgrad_mfma_f32_supported(C1, C2, Cout)) {
        fam = FAM_F32;
    } else if (impl == TDX_CONV_MFMA || (impl == TDX_CONV_AUTO && tdx_is_h16(dtype) && conv3_wgrad_mfma_supported(C1, C2, Cout))) {
        if (!tdx_is_h16(dtype)) return refuse(TDX_EDTYPE);
        if (!conv3_wgrad_mfma_supported(C1, C2, Cout)) return refuse(TDX_ESHAPE);
        fam = FAM_H16;
    }
    // TDX_DETERMINISTIC: the launchers hold their K splits to the slab capacity (per-split slabs added in order: their
    // default for few splits)
    const bool det = tdx_deterministic();
    Conv3WgradCall c = {};  // the shape: all a plan function reads of it
    c.C1 = C1; c.C2 = C2; c.Cout = Cout; c.B = B; c.X = X; c.Y = Y; c.Z = Z;
    bool ok;
    if (fam == FAM_DIRECT) {
        // any shape, the three tensor dtypes (conv3_wgrad_direct_launch dispatches on it)
        if (dtype != TDX_F32 && dtype != TDX_BF16 && dtype != TDX_F16) return refuse(TDX_EDTYPE);
        ok = conv3_wgrad_direct_plan(p, c, det ? std::min(w3_slab_capacity(Cin, Cout), 64) : 0);
    } else {
        // the fp32-tensor kernels split K 256-fold on the fine levels and merge with atomics by default (8 slabs); deterministic
        // runs give them the slab capacity the 16-bit kernels use
        const int ms = (fam != FAM_H16 && !det) ? W3_MAX_SLABS : w3_slab_capacity(Cin, Cout);
        if (fam == FAM_SPLIT) {
            // grids that give every workgroup several bricks: the producer / consumer form
            ok = conv3_wgrad_split_ring_plan(p, c, ms) || conv3_wgrad_mfma_split_plan(p, c, ms);
        } else if (fam == FAM_F32) {
            ok = conv3_wgrad_mfma_f32_plan(p, c, ms);
        } else {
            // deep U-Net levels: the packed-K kernel; fine levels: the producer / consumer form (8 computing + 4 loader
            // waves); else the brick kernel
            ok = conv3_wgrad_small_plan(p, c, ms) || conv3_wgrad_ring_plan(p, c, ms) || conv3_wgrad_mfma_plan(p, c, ms);
        }
    }
    if (!ok) return refuse(TDX_ESHAPE);
    // more slabs than the 16 x 16 unpack kernel walks (MFMA kernels only): the per-tap summing unpack
    p.sum_unpack = (p.kernel != TDX_WGRAD_DIRECT && p.nslab > W3_MAX_SLABS) ? 1 : 0;
    p.status = TDX_OK;
    return p;
}

static int conv3_wgrad_launch(const Conv3WgradCall& c, const Conv3WgradPlan& p, int dtype) {
    switch (p.kernel) {
        case TDX_WGRAD_BRICK16: return conv3_wgrad_mfma_launch(c, p);
        case TDX_WGRAD_SMALL: return conv3_wgrad_small_launch(c, p);
        case TDX_WGRAD_RING: return conv3_wgrad_ring_launch(c, p);
        case TDX_WGRAD_BRICK_F32: return conv3_wgrad_mfma_f32_launch(c, p);
        case TDX_WGRAD_SPLIT: return conv3_wgrad_mfma_split_launch(c, p);
        case TDX_WGRAD_SPLIT_RING: return conv3_wgrad_split_ring_launch(c, p);
        default: return conv3_wgrad_direct_launch(c, p, dtype);
    }
}

extern "C" int tdx_conv3_bwd_weight_plan(int C1, int C2, int Cout, int B, int X, int Y, int Z, int dtype, int impl, int* plan) {
    TDX_CHECK_ARG(plan);
    const Conv3WgradPlan p = conv3_wgrad_plan(dtype, impl, C1, C2, Cout, B, X, Y, Z);
    for (int i = 0; i < TDX_WGRAD_PLAN_INTS; ++i) plan[i] = 0;
    plan[TDX_WGRAD_PLAN_KERNEL] = p.kernel;
    plan[TDX_WGRAD_PLAN_TILE] = p.nt;
    plan[TDX_WGRAD_PLAN_DEPTH] = p.depth;
    plan[TDX_WGRAD_PLAN_NSPLIT] = p.nsplit;
    plan[TDX_WGRAD_PLAN_NSLAB] = p.nslab;
    plan[TDX_WGRAD_PLAN_SUM_UNPACK] = p.sum_unpack;
    plan[TDX_WGRAD_PLAN_NBG] = p.nbg;
    plan[TDX_WGRAD_PLAN_XS] = p.xs;
    plan[TDX_WGRAD_PLAN_GX] = p.gx;
    plan[TDX_WGRAD_PLAN_NGROUPS] = p.ngroups;
    plan[TDX_WGRAD_PLAN_MAX_SLABS] = p.max_slabs;
    plan[TDX_WGRAD_PLAN_NBRICKS] = p.nbricks;
    plan[TDX_WGRAD_PLAN_ORDER] = p.order;
    return p.status;
}

extern "C" int tdx_conv3_bwd_weight(const void* x1, int C1, const void* x2, int C2, const void* dy, float* dw,
                                    float* dbias, int B, int X, int Y, int Z, int Cout, int dtype, int impl,
                                    void* workspace, void* stream) {
    TDX_CHECK_ARG(x1 && dy && dw && workspace && B > 0 && X > 0 && Y > 0 && Z > 0 && C1 > 0 && C2 >= 0 && Cout > 0);
    TDX_CHECK_ARG(C2 == 0 || x2);
    const int Cin = C1 + C2;
    if ((C1 % 8) || (C2 % 8) || (Cout % 8)) return TDX_ESHAPE;
    hipStream_t st = as_stream(stream);
    const bool clean = (impl & TDX_WS_CLEAN) != 0;
    float* dwp = (float*)workspace;
    float* dbw = dwp + (size_t)27 * Cin * Cout;  // bias-gradient accumulator
    if (!clean) {
        int e = tdx_zero_async(dwp, ((size_t)27 * Cin * Cout + Cout) * sizeof(float), st);
        if (e != TDX_OK) return e;
    }
    const Conv3WgradPlan p = conv3_wgrad_plan(dtype, impl, C1, C2, Cout, B, X, Y, Z);
    if (p.status != TDX_OK) return p.status;
    // TDX_DETERMINISTIC: no bias-gradient atomics inside the weight-gradient kernels -- the bias gradient is summed from dy in a
    // fixed order afterwards (partials in the slab region, free again once the unpack kernel has read it)
    const bool det = tdx_deterministic();
    float* slab_base = dbw + ((Cout + 63) / 64) * 64;
    auto ordered_bias = [&]() -> int {
        if (!det || !dbias) return TDX_OK;
        return bias_grad_ordered_launch(dy, (int64_t)B * X * Y * Z, Cout, dtype, dbias, slab_base,
                                        (size_t)W3_MAX_SLABS * 27 * Cin * Cout, st);
    };
    const Conv3WgradCall c = {x1, C1, x2, C2, dy, dwp, (dbias && !det) ? dbw : nullptr, B, X, Y, Z, Cout, st, slab_base,
                              dtype == TDX_F16};
    const int rc = conv3_wgrad_launch(c, p, dtype);
    if (rc != TDX_OK) return rc;
    const int rc_unpack = conv3_unpack_wgrad_launch(c, p, dw, dbw, dbias);
    return rc_unpack != TDX_OK ? rc_unpack : ordered_bias();
}
