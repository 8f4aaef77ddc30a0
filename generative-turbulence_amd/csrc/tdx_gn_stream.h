// The streaming skeleton of the channels-last normalisation kernels (tdx_groupnorm.hip, tdx_batchnorm.hip): a thread owns
// one 8-channel vector of an NDHWC tensor and walks voxels with a grid stride, GN_UNROLL voxels per trip with their 16-B
// loads issued back to back.  Include after tdx_common.h (define TDX_NT_LOADS first for nontemporal bf16 loads).
#pragma once
#include "tdx_common.h"

#define GN_THREADS 256
#define GN_UNROLL 4

// Where a thread streams: lane vector lc (channels [8 lc, 8 lc + 8)) of the voxels first, first + stride, ... of sample
// blockIdx.y; element (v, its channels) of an activation tensor t is t + base + v * C.  Threads with r >= rows are spares
// (GN_THREADS % L != 0): their `first` belongs to the next block.
struct GnLane {
    int lc, r, rows;
    int64_t base, stride, first;
};
__device__ __forceinline__ GnLane gn_lane(int64_t V, int C) {
    const int L = C >> 3;
    GnLane p;
    p.rows = GN_THREADS / L;
    p.lc = threadIdx.x % L;
    p.r = threadIdx.x / L;
    p.base = ((int64_t)blockIdx.y * V) * C + p.lc * 8;
    p.stride = (int64_t)gridDim.x * p.rows;
    p.first = (int64_t)blockIdx.x * p.rows + p.r;
    return p;
}

// The two loops.  body(a, s, v) gets voxel v of the NIN tensors `in` as a[0..NIN) and s = side(v), a per-voxel load of
// the kernel's own that is issued with the trip's other loads.  Spare threads do nothing unless ALL_LANES: a body that
// ends in a cross-lane butterfly sets it, and every lane of a voxel's group then runs the same trips (v is theirs alike).
template <typename T, int NIN, bool ALL_LANES, typename Side, typename Body>
__device__ __forceinline__ void gn_stream(const GnLane& p, const T* const* in, int64_t V, int C, Side side, Body body) {
    if (!ALL_LANES && p.r >= p.rows) return;
    int64_t v = p.first;
    // full trips: GN_UNROLL independent loads in flight, no branches between them
    for (; v + (GN_UNROLL - 1) * p.stride < V; v += p.stride * GN_UNROLL) {
        Raw8<T> raw[GN_UNROLL][NIN];
        decltype(side(v)) s[GN_UNROLL];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) {
#pragma unroll
            for (int i = 0; i < NIN; ++i) raw[u][i].load(in[i] + p.base + (v + u * p.stride) * C);
            s[u] = side(v + u * p.stride);
        }
        __builtin_amdgcn_sched_barrier(0);  // all loads of the trip are issued before any arithmetic
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) {
            Vec8<T> a[NIN];
#pragma unroll
            for (int i = 0; i < NIN; ++i) a[i] = raw[u][i].get();
            body(a, s[u], v + u * p.stride);
        }
    }
    for (; v < V; v += p.stride) {
        Vec8<T> a[NIN];
#pragma unroll
        for (int i = 0; i < NIN; ++i) a[i].load(in[i] + p.base + v * C);
        body(a, side(v), v);
    }
}
// without a side load: body(a, v)
template <typename T, int NIN, bool ALL_LANES = false, typename Body>
__device__ __forceinline__ void gn_stream(const GnLane& p, const T* const* in, int64_t V, int C, Body body) {
    struct None {};
    gn_stream<T, NIN, ALL_LANES>(p, in, V, C, [](int64_t) { return None(); },
                                 [&](const Vec8<T>(&a)[NIN], None, int64_t v) { body(a, v); });
}
