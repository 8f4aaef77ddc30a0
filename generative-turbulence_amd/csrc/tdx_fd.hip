// Finite differences of turbdiff/metrics.py:9-92 and the per-cell features of WassersteinMetric.features
// (turbdiff/models/metrics.py:570-586) on the device.
//   tdx_fd          : curl / divergence / enstrophy of a padded (B, 3, X, Y, Z) velocity grid at its unpadded
//                     interior (B, C, X-2, Y-2, Z-2) with centred differences (x[i+1] - x[i-1]) / (2 h_axis)
//   tdx_ot_features : [u, curl u, p] / std at the in-domain cells, (S, n_cells, 8) f32 with a zero 8th lane: the
//                     curl is evaluated at the gathered cells only, so the curl grid never reaches HBM
// The reference forms each derivative as (narrow(x, 2) - narrow(x, 0)) / (2 h) in fp32 and combines them in the
// order written there; the kernels keep that order, so the results agree to the last bit up to contraction.
#include "tdx_common.h"

struct FdGrid {
    int X, Y, Z;          // padded extents
    float two_h[3];       // fp32(2 h_axis), as torch converts the Python scalar
};

// the six off-diagonal derivatives at padded position (x, y, z) of one sample's (3, X, Y, Z) grid
__device__ __forceinline__ void curl_at(const float* __restrict__ u, const FdGrid& g, int x, int y, int z, float c[3]) {
    const int64_t V = (int64_t)g.X * g.Y * g.Z, sx = (int64_t)g.Y * g.Z, sy = g.Z;
    const int64_t o = x * sx + y * sy + z;
    const float* ux = u;
    const float* uy = u + V;
    const float* uz = u + 2 * V;
    const float ux_y = __fsub_rn(ux[o + sy], ux[o - sy]) / g.two_h[1];
    const float ux_z = __fsub_rn(ux[o + 1], ux[o - 1]) / g.two_h[2];
    const float uy_x = __fsub_rn(uy[o + sx], uy[o - sx]) / g.two_h[0];
    const float uy_z = __fsub_rn(uy[o + 1], uy[o - 1]) / g.two_h[2];
    const float uz_x = __fsub_rn(uz[o + sx], uz[o - sx]) / g.two_h[0];
    const float uz_y = __fsub_rn(uz[o + sy], uz[o - sy]) / g.two_h[1];
    c[0] = __fsub_rn(uz_y, uy_z);
    c[1] = __fsub_rn(ux_z, uz_x);
    c[2] = __fsub_rn(uy_x, ux_y);
}

// one thread per interior voxel; blockIdx.y = sample
__global__ void __launch_bounds__(256)
fd_kernel(const float* __restrict__ u, float* __restrict__ out, FdGrid g, int mode, float dv) {
    const int IX = g.X - 2, IY = g.Y - 2, IZ = g.Z - 2;
    const int64_t Vi = (int64_t)IX * IY * IZ;
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= Vi) return;
    const int z = (int)(v % IZ), y = (int)((v / IZ) % IY), x = (int)(v / ((int64_t)IY * IZ));
    const int b = blockIdx.y;
    const float* ub = u + (int64_t)b * 3 * g.X * g.Y * g.Z;
    if (mode == TDX_FD_DIVERGENCE) {
        const int64_t V = (int64_t)g.X * g.Y * g.Z, sx = (int64_t)g.Y * g.Z, sy = g.Z;
        const int64_t o = (x + 1) * sx + (y + 1) * sy + (z + 1);
        const float ux_x = __fsub_rn(ub[o + sx], ub[o - sx]) / g.two_h[0];
        const float uy_y = __fsub_rn(ub[V + o + sy], ub[V + o - sy]) / g.two_h[1];
        const float uz_z = __fsub_rn(ub[2 * V + o + 1], ub[2 * V + o - 1]) / g.two_h[2];
        out[(int64_t)b * Vi + v] = __fadd_rn(__fadd_rn(ux_x, uy_y), uz_z);
        return;
    }
    float c[3];
    curl_at(ub, g, x + 1, y + 1, z + 1, c);
    if (mode == TDX_FD_CURL) {
        float* ob = out + (int64_t)b * 3 * Vi + v;
        ob[0] = c[0];
        ob[Vi] = c[1];
        ob[2 * Vi] = c[2];
    } else {  // TDX_FD_ENSTROPHY: |curl|^2 * prod(h)
        const float s = __fadd_rn(__fadd_rn(__fmul_rn(c[0], c[0]), __fmul_rn(c[1], c[1])), __fmul_rn(c[2], c[2]));
        out[(int64_t)b * Vi + v] = __fmul_rn(s, dv);
    }
}

// one thread per (sample, cell)
__global__ void __launch_bounds__(256)
ot_features_kernel(const float* __restrict__ u_grid, const float* __restrict__ u_cells, const float* __restrict__ p_cells,
                   const int64_t* __restrict__ unpadded_idx, const float* __restrict__ scale, float* __restrict__ out,
                   FdGrid g, int64_t n_cells) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const int s = blockIdx.y;
    const int IY = g.Y - 2, IZ = g.Z - 2;
    const int64_t flat = unpadded_idx[c];
    const int z = (int)(flat % IZ), y = (int)((flat / IZ) % IY), x = (int)(flat / ((int64_t)IY * IZ));
    float cu[3];
    curl_at(u_grid + (int64_t)s * 3 * g.X * g.Y * g.Z, g, x + 1, y + 1, z + 1, cu);
    const int64_t sc = (int64_t)s * n_cells + c;
    const float* uc = u_cells + sc * 3;
    float4* o = reinterpret_cast<float4*>(out + sc * 8);
    o[0] = make_float4(uc[0] / scale[0], uc[1] / scale[1], uc[2] / scale[2], cu[0] / scale[3]);
    o[1] = make_float4(cu[1] / scale[4], cu[2] / scale[5], p_cells[sc] / scale[6], 0.0f);
}

static bool fd_grid(int X, int Y, int Z, float two_hx, float two_hy, float two_hz, FdGrid* g) {
    if (X < 3 || Y < 3 || Z < 3 || (int64_t)X * Y * Z >= (1ll << 31)) return false;
    *g = FdGrid{X, Y, Z, {two_hx, two_hy, two_hz}};
    return true;
}

extern "C" int tdx_fd(const float* u, float* out, int B, int X, int Y, int Z, float two_hx, float two_hy, float two_hz,
                      float dv, int mode, void* stream) {
    TDX_CHECK_ARG(u && out && B > 0 && X > 0 && Y > 0 && Z > 0);
    TDX_CHECK_ARG(mode == TDX_FD_CURL || mode == TDX_FD_DIVERGENCE || mode == TDX_FD_ENSTROPHY);
    FdGrid g;
    if (B > 65535 || !fd_grid(X, Y, Z, two_hx, two_hy, two_hz, &g)) return TDX_ESHAPE;
    const int64_t Vi = (int64_t)(X - 2) * (Y - 2) * (Z - 2);
    hipLaunchKernelGGL(fd_kernel, dim3((unsigned)ceil_div(Vi, (int64_t)256), B), dim3(256), 0, as_stream(stream), u, out, g,
                       mode, dv);
    return tdx_launch_status();
}

extern "C" int tdx_ot_features(const float* u_grid, const float* u_cells, const float* p_cells, const int64_t* unpadded_idx,
                               const float* scale, float* out, int S, int64_t n_cells, int X, int Y, int Z, float two_hx,
                               float two_hy, float two_hz, void* stream) {
    TDX_CHECK_ARG(u_grid && u_cells && p_cells && unpadded_idx && scale && out && S > 0 && n_cells > 0);
    FdGrid g;
    if (S > 65535 || !fd_grid(X, Y, Z, two_hx, two_hy, two_hz, &g)) return TDX_ESHAPE;
    hipLaunchKernelGGL(ot_features_kernel, dim3((unsigned)ceil_div(n_cells, (int64_t)256), S), dim3(256), 0,
                       as_stream(stream), u_grid, u_cells, p_cells, unpadded_idx, scale, out, g, n_cells);
    return tdx_launch_status();
}
