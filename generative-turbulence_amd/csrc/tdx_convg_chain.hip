// The DilResNet chain (dilresnet.py:47-94) on the matrix-core gather kernel, gfx950, bf16 tensors with fp32 arithmetic:
//   tdx_convg_apply_fused   forward: the conv's epilogue also does the ReLU, the residual / conditioning adds, the copy of the
//                           pre-add activation a training step keeps, or the rollout state update of the decode conv
//                           (convg_mfma_kernel<false, NT, true> in tdx_convg_mfma.hip)
//   tdx_convg_fold_fused    backward: the fold of the padded-grid adjoint onto the clamped voxels (as tdx_convg_fold_clamp)
//                           plus the residual gradient, the ReLU mask of the producing layer and the sum into d c_enc
//                           (convg_fold_kernel<bf16, true> in tdx_convg.h)
// Without them a layer's forward is conv + relu + one or two adds and its backward fold + relu mask + add: five extra passes
// over B x V x 48 bf16 per layer.  Semantics and operand layouts are in include/tdx.h.
#include "tdx_common.h"
#include "tdx_convg.h"

extern "C" int tdx_convg_apply_fused(const void* in, const float* w, const float* bias, void* out, int B, int Xi, int Yi, int Zi,
                                     int Cin, int Xo, int Yo, int Zo, int Cout, int k, int dilation, int pad, int replicate,
                                     const TdxConvgEpilogue* ep, int dtype, void* stream) {
    TDX_CHECK_ARG(in && w && out);
    if (dtype != TDX_BF16) return TDX_EDTYPE;
    const ConvG g = convg_geometry(B, Xi, Yi, Zi, Cin, Xo, Yo, Zo, Cout, k, 1, dilation, pad, replicate, 0);
    int rc = convg_check(g);
    if (rc != TDX_OK) return rc;
    for (int a = 0; a < 3; ++a)
        if (g.Eo[a] != g.Ei[a] + 2 * pad - dilation * (k - 1)) return TDX_ESHAPE;  // stride-1 gather
    if (ep != nullptr && ep->x != nullptr) {
        TDX_CHECK_ARG(ep->x_next && ep->inside && ep->dx_mean && ep->dx_std && ep->F > 0);
        if (Cout > 16 || ep->F > Cout) return TDX_ESHAPE;
    }
    return convg_mfma_apply(g, in, w, bias, out, false, ep, as_stream(stream));
}

extern "C" int tdx_convg_fold_fused(const void* dpad, const void* res, const void* mask_src, void* dx, void* dx_masked, float* acc,
                                    int B, int X, int Y, int Z, int pad, int C, int dtype, void* stream) {
    TDX_CHECK_ARG(dpad && B > 0 && X > 0 && Y > 0 && Z > 0 && pad >= 0 && C > 0);
    TDX_CHECK_ARG((mask_src == nullptr) == (dx_masked == nullptr));
    if (dtype != TDX_BF16) return TDX_EDTYPE;
    if (C % 8) return TDX_ESHAPE;
    const int nb = acc != nullptr ? B : 1;
    const int64_t total = (int64_t)(B / nb) * X * Y * Z * (C / 8);
    hipLaunchKernelGGL((convg_fold_kernel<bf16, true>), dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream),
                       (const bf16*)dpad, (const bf16*)res, (const bf16*)mask_src, (bf16*)dx, (bf16*)dx_masked, acc, B, nb, X, Y, Z,
                       pad, C);
    return tdx_launch_status();
}
