// The DilResNet chain (dilresnet.py:47-94) on the matrix-core gather kernel, gfx950, bf16 tensors with fp32 arithmetic:
//   tdx_convg_apply_fused   forward: the conv's epilogue also does the ReLU, the residual / conditioning adds, the copy of the
//                           pre-add activation a training step keeps, or the rollout state update of the decode conv
//                           (convg_mfma_kernel<false, NT, true> in tdx_convg_mfma.hip)
//   tdx_convg_fold_fused    backward: the fold of the padded-grid adjoint onto the clamped voxels (as tdx_convg_fold_clamp)
//                           plus the residual gradient, the ReLU mask of the producing layer and the sum into d c_enc
// Without them a layer's forward is conv + relu + one or two adds and its backward fold + relu mask + add: five extra passes
// over B x V x 48 bf16 per layer.  Semantics and operand layouts are in include/tdx.h.
#include "tdx_common.h"
#include "tdx_convg.h"

extern "C" int tdx_convg_apply_fused(const void* in, const float* w, const float* bias, void* out, int B, int Xi, int Yi, int Zi,
                                     int Cin, int Xo, int Yo, int Zo, int Cout, int k, int dilation, int pad, int replicate,
                                     const TdxConvgEpilogue* ep, int dtype, void* stream) {
    TDX_CHECK_ARG(in && w && out && B > 0 && k > 0 && dilation > 0 && pad >= 0);
    if (dtype != TDX_BF16) return TDX_EDTYPE;
    if ((Cin % 8) || (Cout % 8) || Cin <= 0 || Cout <= 0) return TDX_ESHAPE;
    const int Ei[3] = {Xi, Yi, Zi}, Eo[3] = {Xo, Yo, Zo};
    for (int a = 0; a < 3; ++a) {
        if (Ei[a] <= 0 || Eo[a] <= 0) return TDX_EINVAL;
        if (Eo[a] != Ei[a] + 2 * pad - dilation * (k - 1)) return TDX_ESHAPE;  // stride-1 gather
    }
    if (ep == nullptr)
        return convg_mfma_apply(in, w, bias, out, B, Ei, Eo, Cin, Cout, k, 1, dilation, pad, replicate, 0, as_stream(stream));
    if (ep->x != nullptr) {
        TDX_CHECK_ARG(ep->x_next && ep->inside && ep->dx_mean && ep->dx_std && ep->F > 0);
        if (Cout > 16 || ep->F > Cout) return TDX_ESHAPE;
    }
    return convg_mfma_apply_epilogue(in, w, bias, out, B, Ei, Eo, Cin, Cout, k, dilation, pad, replicate, ep, as_stream(stream));
}

// thread = (batch entry, voxel, 8-channel group); with `acc` it walks the whole batch (nb = B), so that the fp32 sum over b
// needs no atomics
__global__ void __launch_bounds__(256)
convg_fold_fused_kernel(const bf16* __restrict__ dpad, const bf16* __restrict__ res, const bf16* __restrict__ mask_src,
                        bf16* __restrict__ dx, bf16* __restrict__ dx_masked, float* __restrict__ acc, int B, int nb, int E0, int E1,
                        int E2, int pad, int C) {
    const int groups = C >> 3;
    const int64_t V = (int64_t)E0 * E1 * E2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)(B / nb) * V * groups) return;
    const int b0 = (int)(idx / (V * groups)) * nb;
    const int cg = (int)(idx % groups);
    int64_t v = (idx / groups) % V;
    const int i2 = (int)(v % E2); v /= E2;
    const int i1 = (int)(v % E1);
    const int i0 = (int)(v / E1);
    const int E[3] = {E0, E1, E2}, i[3] = {i0, i1, i2};
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = i[a] == 0 ? 0 : i[a] + pad;  // padded coordinates q = i + pad; q <= pad clamps to 0
        hi[a] = i[a] == E[a] - 1 ? E[a] - 1 + 2 * pad : i[a] + pad;
    }
    const int P0 = E0 + 2 * pad, P1 = E1 + 2 * pad, P2 = E2 + 2 * pad;
    const int64_t vox = (idx / groups) % V;
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = b0; b < b0 + nb; ++b) {
        float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int q0 = lo[0]; q0 <= hi[0]; ++q0)
            for (int q1 = lo[1]; q1 <= hi[1]; ++q1)
                for (int q2 = lo[2]; q2 <= hi[2]; ++q2) {
                    Vec8<bf16> d;
                    d.load(dpad + ((((int64_t)b * P0 + q0) * P1 + q1) * P2 + q2) * C + cg * 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) t[j] += d.v[j];
                }
        const int64_t off = ((int64_t)b * V + vox) * C + cg * 8;
        if (res != nullptr) {
            Vec8<bf16> r;
            r.load(res + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] += r.v[j];
        }
        if (dx != nullptr) {
            Vec8<bf16> o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = t[j];
            o.store(dx + off);
        }
        if (mask_src != nullptr) {
            Vec8<bf16> m, o;
            m.load(mask_src + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = m.v[j] > 0.f ? t[j] : 0.f;
            o.store(dx_masked + off);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] += t[j];
    }
    if (acc != nullptr) {
        Vec8<float> a;
        a.load(acc + vox * C + cg * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) a.v[j] += sum[j];
        a.store(acc + vox * C + cg * 8);
    }
}

extern "C" int tdx_convg_fold_fused(const void* dpad, const void* res, const void* mask_src, void* dx, void* dx_masked, float* acc,
                                    int B, int X, int Y, int Z, int pad, int C, int dtype, void* stream) {
    TDX_CHECK_ARG(dpad && B > 0 && X > 0 && Y > 0 && Z > 0 && pad >= 0 && C > 0);
    TDX_CHECK_ARG((mask_src == nullptr) == (dx_masked == nullptr));
    if (dtype != TDX_BF16) return TDX_EDTYPE;
    if (C % 8) return TDX_ESHAPE;
    const int nb = acc != nullptr ? B : 1;
    const int64_t total = (int64_t)(B / nb) * X * Y * Z * (C / 8);
    hipLaunchKernelGGL(convg_fold_fused_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), (const bf16*)dpad,
                       (const bf16*)res, (const bf16*)mask_src, (bf16*)dx, (bf16*)dx_masked, acc, B, nb, X, Y, Z, pad, C);
    return tdx_launch_status();
}
