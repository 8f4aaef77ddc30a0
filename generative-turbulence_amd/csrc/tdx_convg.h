// The general 3-D convolution family (tdx_convg.hip: vector-ALU kernels and the entry points; tdx_convg_mfma.hip: matrix-core
// kernels; tdx_convg_chain.hip: the DilResNet chain's entry points): its geometry record, the index arithmetic that decides
// where a tap reads from -- written here once, every kernel calls it -- the fold kernel, and the matrix-core launchers.
#pragma once
#include "tdx_common.h"

#define CGM_ROWS 256  // output voxels per workgroup of the matrix-core kernels

struct ConvG {
    int B;
    int Ei[3], Eo[3];  // grid of `in` and of `out` (weight gradient: of the conv's input and of dy)
    int k, stride, dil, pad;
    int clamp;         // gather only: 1 = replicate padding (clamp the source), 0 = zero padding
    int Cin, Cout;     // channels of `in` and of `out`
    int cs;            // residue classes per axis (= stride for scatter^T, else 1)
    int cls_blocks;    // workgroups of CGM_ROWS voxels per residue class (class 0 has the most voxels)
};

static inline ConvG convg_geometry(int B, int Xi, int Yi, int Zi, int Cin, int Xo, int Yo, int Zo, int Cout, int k, int stride,
                                   int dil, int pad, int replicate, int transposed) {
    ConvG g = {B, {Xi, Yi, Zi}, {Xo, Yo, Zo}, k, stride, dil, pad, replicate, Cin, Cout, transposed ? stride : 1, 0};
    if (g.cs >= 1) {
        int64_t mc = B;
        for (int a = 0; a < 3; ++a) mc *= (g.Eo[a] + g.cs - 1) / g.cs;
        g.cls_blocks = (int)((mc + CGM_ROWS - 1) / CGM_ROWS);
    }
    return g;
}

static inline int convg_check(const ConvG& g) {
    if (g.B <= 0 || g.k < 1 || g.k > 7 || g.stride < 1 || g.dil < 1 || g.pad < 0) return TDX_EINVAL;
    for (int a = 0; a < 3; ++a)
        if (g.Ei[a] <= 0 || g.Eo[a] <= 0) return TDX_EINVAL;
    if ((g.Cin % 8) || (g.Cout % 8) || g.Cin <= 0 || g.Cout <= 0) return TDX_ESHAPE;
    return TDX_OK;
}

// ---- index arithmetic
// row m of a (B, E[0], E[1], E[2]) grid -> its voxel o; returns b
__device__ __forceinline__ int convg_row_voxel(int64_t m, const int* E, int* o) {
    o[2] = (int)(m % E[2]); m /= E[2];
    o[1] = (int)(m % E[1]); m /= E[1];
    o[0] = (int)(m % E[0]);
    return (int)(m / E[0]);
}
// voxels per axis of residue class c (o = c mod cs along every axis) of grid E
__device__ __forceinline__ void convg_class_grid(const int* E, const int* c, int cs, int* Ec) {
#pragma unroll
    for (int a = 0; a < 3; ++a) Ec[a] = E[a] > c[a] ? (E[a] - c[a] + cs - 1) / cs : 0;
}
// row m of residue class c (Ec = convg_class_grid) -> its voxel o = c + cs * (position in the class); returns b
__device__ __forceinline__ int convg_class_row_voxel(int64_t m, const int* Ec, const int* c, int cs, int* o) {
    const int b = convg_row_voxel(m, Ec, o);
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = c[a] + cs * o[a];
    return b;
}
// tap (or residue class) index t -> (t0, t1, t2), base k
__device__ __forceinline__ void convg_tap(int t, int k, int* tt) { tt[0] = t / (k * k); tt[1] = (t / k) % k; tt[2] = t % k; }
// row of voxel s of sample b in an NDHWC tensor of grid E
__device__ __forceinline__ int64_t convg_row(int b, const int* s, const int* E) {
    return (((int64_t)b * E[0] + s[0]) * E[1] + s[1]) * E[2] + s[2];
}
// gather: tap tt of output voxel o reads s = o * stride - pad + tt * dilation, clamped onto the grid (replicate padding) or
// nothing when outside (zero padding: returns false)
__device__ __forceinline__ bool convg_gather_src(const ConvG& g, const int* o, const int* tt, int* s) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int q = o[a] * g.stride - g.pad + tt[a] * g.dil;
        if (g.clamp) q = min(max(q, 0), g.Ei[a] - 1);
        ok = ok && q >= 0 && q < g.Ei[a];
        s[a] = q;
    }
    return ok;
}
// scatter^T: tap tt of output voxel o reads s = (o + pad - tt * dilation) / stride where the stride divides that along every
// axis and s is in range.  Divisibility depends on o mod stride only, so a caller that walks ONE residue class c tests it once
// per tap (convg_tap_live) and passes DIVISIBLE = true.
template <bool DIVISIBLE>
__device__ __forceinline__ bool convg_scatter_src(const ConvG& g, const int* o, const int* tt, int* s) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int num = o[a] + g.pad - tt[a] * g.dil;
        if (!DIVISIBLE) ok = ok && num % g.stride == 0;
        s[a] = g.stride == 1 ? num : (num >= 0 ? num / g.stride : -1);
        ok = ok && s[a] >= 0 && s[a] < g.Ei[a];
    }
    return ok;
}
__device__ __forceinline__ bool convg_tap_live(const ConvG& g, const int* c, const int* tt) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int num = c[a] + g.pad - tt[a] * g.dil;
        ok = ok && (((num % g.cs) + g.cs) % g.cs) == 0;
    }
    return ok;
}
// fold: the padded positions q = i + pad of the (E + 2 pad) grid that clamp onto voxel i are [lo, hi] per axis (q <= pad
// clamps to 0, q >= E - 1 + pad to E - 1; interior voxels have one)
__device__ __forceinline__ void convg_fold_range(const int* i, const int* E, int pad, int* lo, int* hi) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = i[a] == 0 ? 0 : i[a] + pad;
        hi[a] = i[a] == E[a] - 1 ? E[a] - 1 + 2 * pad : i[a] + pad;
    }
}

// dx[i] = sum of dpad[q] over the padded positions q that clamp onto i: tdx_convg_fold_clamp (FUSED = false, nb = 1).
// FUSED (tdx_convg_fold_fused): plus the residual gradient, the copy masked by the ReLU of the producing layer and the sum
// over the batch into `acc`.  thread = (batch entry, voxel, 8-channel group); with `acc` it walks the whole batch (nb = B), so
// that the fp32 sum over b needs no atomics.
template <typename T, bool FUSED>
__global__ void __launch_bounds__(256)
convg_fold_kernel(const T* __restrict__ dpad, const T* __restrict__ res, const T* __restrict__ mask_src, T* __restrict__ dx,
                  T* __restrict__ dx_masked, float* __restrict__ acc, int B, int nb, int E0, int E1, int E2, int pad, int C) {
    const int groups = C >> 3;
    const int64_t V = (int64_t)E0 * E1 * E2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)(B / nb) * V * groups) return;
    const int cg = (int)(idx % groups);
    const int E[3] = {E0, E1, E2}, P[3] = {E0 + 2 * pad, E1 + 2 * pad, E2 + 2 * pad};
    int i[3], lo[3], hi[3];
    const int b0 = convg_row_voxel(idx / groups, E, i) * nb;
    convg_fold_range(i, E, pad, lo, hi);
    const int64_t vox = convg_row(0, i, E);
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = b0; b < b0 + nb; ++b) {
        float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int q[3];
        for (q[0] = lo[0]; q[0] <= hi[0]; ++q[0])
            for (q[1] = lo[1]; q[1] <= hi[1]; ++q[1])
                for (q[2] = lo[2]; q[2] <= hi[2]; ++q[2]) {
                    Vec8<T> d;
                    d.load(dpad + convg_row(b, q, P) * C + cg * 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) t[j] += d.v[j];
                }
        const int64_t off = ((int64_t)b * V + vox) * C + cg * 8;
        if (FUSED && res != nullptr) {
            Vec8<T> r;
            r.load(res + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] += r.v[j];
        }
        if (!FUSED || dx != nullptr) {
            Vec8<T> o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = t[j];
            o.store(dx + off);
        }
        if (FUSED && mask_src != nullptr) {
            Vec8<T> m, o;
            m.load(mask_src + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = m.v[j] > 0.f ? t[j] : 0.f;
            o.store(dx_masked + off);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] += t[j];
    }
    if (FUSED && acc != nullptr) {
        Vec8<float> a;
        a.load(acc + vox * C + cg * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) a.v[j] += sum[j];
        a.store(acc + vox * C + cg * 8);
    }
}

// ---- launchers of the matrix-core kernels (tdx_convg_mfma.hip; bf16 tensors), g checked by the caller
// gather, or scatter^T (transposed; g.cs = g.stride then); ep: the fused epilogue of a stride-1 gather (tdx_convg_apply_fused
// has checked its options), or nullptr for the plain `acc + bias` store
int convg_mfma_apply(const ConvG& g, const void* in, const float* w, const float* bias, void* out, bool transposed,
                     const TdxConvgEpilogue* ep, hipStream_t st);
int convg_mfma_bwd_weight(const ConvG& g, const void* in, const void* dy, float* dw, float* dbias, hipStream_t st);
