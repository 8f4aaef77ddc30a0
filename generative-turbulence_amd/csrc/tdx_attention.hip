// Bottleneck self-attention on the to_qkv output (attention.py:9-15, ddpm.py:295-308).
//
// qkv is the NDHWC output of the 1x1 to_qkv conv: [B][N][3*H*D] with channel thirds q|k|v,
// head-major inside each third, so no permute/contiguous copies are needed (the reference
// makes three, ddpm.py:298-303).
//
// Vector-ALU "row" kernels: one lane owns one query (fwd, dQ) or one key (dK/dV) row with
// its D=32 vector in registers and walks the other side; all lanes of a wave read the same
// K/V (or Q/dO) row, i.e. wave-uniform broadcast loads, and keep an online softmax.  This is
// exact fp32 and is the path used at the U-Net bottleneck (N = 144 tokens at 192x64x48,
// 0.01 GFLOP).  The MFMA flash kernels for long sequences live in tdx_attention_mfma.hip and tdx_attention_bwd_mfma.hip.
//
// Host side, below the kernels: attn_plan decides what a call launches, the entry points check their arguments, ask it and
// hand a call record to the launcher of the planned family; tdx_attn_plan reports the same plan without launching.
#include "tdx_attention.h"

// The "other side" rows are walked in tiles of 64 staged in LDS as f32 (thread t stages row t with
// 16-B loads); the inner loops then read them with wave-uniform (broadcast) LDS loads instead of a
// chain of dependent global loads per row.
#define AT_TILE 64
template <typename T, int D>
__device__ __forceinline__ void attn_stage_row(float* __restrict__ dst, const T* __restrict__ src, bool ok) {
#pragma unroll
    for (int c = 0; c < D / 8; ++c) {
        Vec8<T> v;
        if (ok) v.load(src + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[c * 8 + e] = ok ? v.v[e] : 0.f;
    }
}

template <typename T, int D>
__global__ void __launch_bounds__(64)
attn_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, float* __restrict__ lse, int N, int H) {
    const AttnHead<D> hd(blockIdx.y, N, H);
    const int i = blockIdx.x * 64 + threadIdx.x;
    const T* base = hd.batch(qkv);
    const float scale = rsqrtf((float)D);
    float q[D], acc[D];
    const bool valid = i < N;
    const int ii = valid ? i : N - 1;
#pragma unroll
    for (int d = 0; d < D; ++d) { q[d] = ldf(hd.q(base, ii) + d) * scale; acc[d] = 0.f; }
    float m = -INFINITY, l = 0.f;
    __shared__ float sK[AT_TILE][D], sV[AT_TILE][D];
    for (int j0 = 0; j0 < N; j0 += AT_TILE) {
        const int jr = j0 + (int)threadIdx.x;
        __syncthreads();
        attn_stage_row<T, D>(sK[threadIdx.x], hd.k(base, jr), jr < N);
        attn_stage_row<T, D>(sV[threadIdx.x], hd.v(base, jr), jr < N);
        __syncthreads();
        const int nj = min(AT_TILE, N - j0);
        for (int j = 0; j < nj; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) s += q[d] * sK[j][d];
            const float mn = fmaxf(m, s);
            const float alpha = __expf(m - mn);
            const float p = __expf(s - mn);
            l = l * alpha + p;
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] = acc[d] * alpha + p * sV[j][d];
            m = mn;
        }
    }
    if (valid) {
        const float inv = 1.0f / l;
        T* o = hd.out_row(out, i);
#pragma unroll
        for (int d = 0; d < D; ++d) stf(o + d, acc[d] * inv);
        lse[hd.stat(i)] = m + __logf(l);
    }
}

// delta[b,h,i] = sum_d dO[i,d] O[i,d]
template <typename T, int D>
__global__ void attn_delta_kernel(const T* __restrict__ out, const T* __restrict__ dout, float* __restrict__ delta,
                                  int N, int H, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (b, i, h)
    if (idx >= total) return;
    const int h = (int)(idx % H);
    const int64_t bi = idx / H;
    const int i = (int)(bi % N);
    const int b = (int)(bi / N);
    const AttnHead<D> hd(b, h, N, H);
    const T* o = hd.out_token(out, bi);
    const T* g = hd.out_token(dout, bi);
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) s += ldf(o + d) * ldf(g + d);
    delta[hd.stat(i)] = s;
}

// lane = query i:  dQ_i = scale * sum_j dS_ij K_j,  dS_ij = P_ij (dO_i . V_j - delta_i)
template <typename T, int D>
__global__ void __launch_bounds__(64)
attn_bwd_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ dout, const float* __restrict__ lse,
                   const float* __restrict__ delta, T* __restrict__ dqkv, int N, int H) {
    const AttnHead<D> hd(blockIdx.y, N, H);
    const int i = blockIdx.x * 64 + threadIdx.x;
    const T* base = hd.batch(qkv);
    const float scale = rsqrtf((float)D);
    const bool valid = i < N;
    const int ii = valid ? i : N - 1;
    float q[D], g[D], acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        q[d] = ldf(hd.q(base, ii) + d) * scale;
        g[d] = ldf(hd.out_row(dout, ii) + d);
        acc[d] = 0.f;
    }
    const float L = lse[hd.stat(ii)];
    const float dl = delta[hd.stat(ii)];
    __shared__ float sK[AT_TILE][D], sV[AT_TILE][D];
    for (int j0 = 0; j0 < N; j0 += AT_TILE) {
        const int jr = j0 + (int)threadIdx.x;
        __syncthreads();
        attn_stage_row<T, D>(sK[threadIdx.x], hd.k(base, jr), jr < N);
        attn_stage_row<T, D>(sV[threadIdx.x], hd.v(base, jr), jr < N);
        __syncthreads();
        const int nj = min(AT_TILE, N - j0);
        for (int j = 0; j < nj; ++j) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) { s += q[d] * sK[j][d]; dp += g[d] * sV[j][d]; }
            const float ds = __expf(s - L) * (dp - dl);
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] += ds * sK[j][d];
        }
    }
    if (valid) {
        T* o = hd.dq(dqkv, i);
#pragma unroll
        for (int d = 0; d < D; ++d) stf(o + d, acc[d] * scale);
    }
}

// lane = key j:  dV_j = sum_i P_ij dO_i,  dK_j = scale * sum_i dS_ij Q_i
template <typename T, int D>
__global__ void __launch_bounds__(64)
attn_bwd_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ dout, const float* __restrict__ lse,
                    const float* __restrict__ delta, T* __restrict__ dqkv, int N, int H) {
    const AttnHead<D> hd(blockIdx.y, N, H);
    const int j = blockIdx.x * 64 + threadIdx.x;
    const T* base = hd.batch(qkv);
    const float scale = rsqrtf((float)D);
    const bool valid = j < N;
    const int jj = valid ? j : N - 1;
    float k[D], v[D], dk[D], dv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        k[d] = ldf(hd.k(base, jj) + d) * scale;
        v[d] = ldf(hd.v(base, jj) + d);
        dk[d] = dv[d] = 0.f;
    }
    __shared__ float sQ[AT_TILE][D], sG[AT_TILE][D], sL[AT_TILE], sDl[AT_TILE];
    for (int i0 = 0; i0 < N; i0 += AT_TILE) {
        const int ir = i0 + (int)threadIdx.x;
        __syncthreads();
        attn_stage_row<T, D>(sQ[threadIdx.x], hd.q(base, ir), ir < N);
        attn_stage_row<T, D>(sG[threadIdx.x], hd.out_row(dout, ir), ir < N);
        sL[threadIdx.x] = ir < N ? lse[hd.stat(ir)] : 0.f;
        sDl[threadIdx.x] = ir < N ? delta[hd.stat(ir)] : 0.f;
        __syncthreads();
        const int ni = min(AT_TILE, N - i0);
        for (int i = 0; i < ni; ++i) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) { s += k[d] * sQ[i][d]; dp += v[d] * sG[i][d]; }
            const float p = __expf(s - sL[i]);
            const float ds = p * (dp - sDl[i]);
#pragma unroll
            for (int d = 0; d < D; ++d) { dv[d] += p * sG[i][d]; dk[d] += ds * sQ[i][d]; }
        }
    }
    if (valid) {
        T* ok = hd.dk(dqkv, j);
        T* ov = ok + H * D;
#pragma unroll
        for (int d = 0; d < D; ++d) { stf(ok + d, dk[d] * scale); stf(ov + d, dv[d]); }
    }
}

// ---- the plan: every decision of a call, made once (what the fields mean: tdx_attention.h) --------------------------------
// Matrix core: 16-bit tensors at N >= 128 (incl. the U-Net bottleneck, N = 144 at 192x64x48) unless TDX_ATTN_IMPL=vector.
// Stream-K (TDX_ATTN_STREAMK): when the launch is big enough to care about whole rounds of workgroups -- more query blocks
// than slots and not a whole number of rounds, at least 16 key tiles -- and the arena can hold the partials; otherwise, and
// silently, one workgroup per query block.  Norm bound (TDX_ATTN_BOUND): at least 8 key tiles, at most FA_KMAX_PAIRS heads,
// and an arena that holds their table.  TDX_ATTN_BWD_TW = "<dq><dkv>" (A/B knob): tiles per wave of the two backward kernels;
// default 22 (two tiles per wave, two waves per SIMD): one tile per wave at three or four waves per SIMD measured 10.99-12.3 ms
// against 11.4-11.5 (profiles/r13_attention_bwd_ablation.txt) -- more waves do not hide the vector work either.
AttnPlan attn_plan(int B, int N, int H, int D, int dtype) {
    AttnPlan p = {};
    p.workspace = (size_t)B * N * H * sizeof(float);
    p.status = D != FA_D ? TDX_ESHAPE : dtype != TDX_F32 && !tdx_is_h16(dtype) ? TDX_EDTYPE : TDX_OK;
    if (p.status != TDX_OK) return p;
    const bool mfma = tdx_is_h16(dtype) && tdx_switch(SW_ATTN_IMPL) == 0 && N >= 128;
    p.fwd = p.bwd = mfma ? TDX_ATTN_MFMA : TDX_ATTN_VECTOR;
    p.bwd_gx = ceil_div(N, mfma ? FB_RB : 64);
    p.bwd_gy = B * H;
    if (!mfma) return p;
    const size_t arena = tdx_scratch_bytes();  // 0 without one
    auto fits = [arena](size_t offset, size_t bytes) { return offset <= arena && bytes <= arena - offset; };
    p.nqb = ceil_div(N, FA_QB);
    p.ntile = ceil_div(N, FA_KT);
    p.nblk = B * H * p.nqb;
    p.streamk = tdx_switch(SW_ATTN_STREAMK) != 0 && p.nblk > FA_SLOTS && p.nblk % FA_SLOTS != 0 && p.ntile >= 16 &&
                fits(FA_PART_OFFSET, FA_PART_BYTES);
    p.nwg = p.streamk ? FA_SLOTS : p.nblk;
    p.chunk = p.streamk ? (int)(((long long)p.nblk * p.ntile + FA_SLOTS - 1) / FA_SLOTS) : p.ntile;
    p.bound = tdx_switch(SW_ATTN_BOUND) != 0 && fits(FA_KMAX_OFFSET, FA_KMAX_BYTES) && B * H <= FA_KMAX_PAIRS && p.ntile >= 8;
    const int tw = tdx_switch(SW_ATTN_BWD_TW);
    p.twq = tw / 10;
    p.twk = tw % 10;
    return p;
}

static int attn_fwd_vector_launch(const AttnFwdCall& c, const AttnPlan& p) {
    if (p.fwd != TDX_ATTN_VECTOR) return TDX_EINVAL;
    TDX_DISPATCH_DTYPE(c.dtype, hipLaunchKernelGGL((attn_fwd_kernel<T, FA_D>), dim3(p.bwd_gx, p.bwd_gy), dim3(64), 0, c.st,
                                                    (const T*)c.qkv, (T*)c.out, c.lse, c.N, c.H));
    return tdx_launch_status();
}

static int attn_bwd_vector_launch(const AttnBwdCall& c, const AttnPlan& p) {
    if (p.bwd != TDX_ATTN_VECTOR) return TDX_EINVAL;
    const dim3 grid(p.bwd_gx, p.bwd_gy);
    TDX_DISPATCH_DTYPE(c.dtype, {
        hipLaunchKernelGGL((attn_bwd_dq_kernel<T, FA_D>), grid, dim3(64), 0, c.st, (const T*)c.qkv, (const T*)c.dout, c.lse,
                           c.delta, (T*)c.dqkv, c.N, c.H);
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, FA_D>), grid, dim3(64), 0, c.st, (const T*)c.qkv, (const T*)c.dout, c.lse,
                           c.delta, (T*)c.dqkv, c.N, c.H);
    });
    return tdx_launch_status();
}

extern "C" int tdx_attn_plan(int B, int N, int H, int D, int dtype, int* plan) {
    TDX_CHECK_ARG(plan && B > 0 && N > 0 && H > 0);
    const AttnPlan p = attn_plan(B, N, H, D, dtype);
    for (int i = 0; i < TDX_ATTN_PLAN_INTS; ++i) plan[i] = 0;
    if (p.status != TDX_OK) return p.status;
    plan[TDX_ATTN_PLAN_FWD] = p.fwd;
    plan[TDX_ATTN_PLAN_BWD] = p.bwd;
    plan[TDX_ATTN_PLAN_NQB] = p.nqb;
    plan[TDX_ATTN_PLAN_NTILE] = p.ntile;
    plan[TDX_ATTN_PLAN_NWG] = p.nwg;
    plan[TDX_ATTN_PLAN_CHUNK] = p.chunk;
    plan[TDX_ATTN_PLAN_STREAMK] = p.streamk;
    plan[TDX_ATTN_PLAN_BOUND] = p.bound;
    plan[TDX_ATTN_PLAN_TW_DQ] = p.twq;
    plan[TDX_ATTN_PLAN_TW_DKV] = p.twk;
    plan[TDX_ATTN_PLAN_BWD_GX] = p.bwd_gx;
    plan[TDX_ATTN_PLAN_BWD_GY] = p.bwd_gy;
    plan[TDX_ATTN_PLAN_WORKSPACE] = p.workspace > 0x7fffffffu ? 0x7fffffff : (int)p.workspace;
    return TDX_OK;
}

extern "C" int tdx_attn_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, int D, int dtype,
                            void* stream) {
    TDX_CHECK_ARG(qkv && out && lse && B > 0 && N > 0 && H > 0);
    const AttnPlan p = attn_plan(B, N, H, D, dtype);
    if (p.status != TDX_OK) return p.status;
    const AttnFwdCall c = {qkv, out, lse, B, N, H, dtype, as_stream(stream)};
    return p.fwd == TDX_ATTN_MFMA ? attn_fwd_mfma_launch(c, p) : attn_fwd_vector_launch(c, p);
}

extern "C" size_t tdx_attn_bwd_workspace_bytes(int B, int N, int H, int D) {
    return attn_plan(B, N, H, D, TDX_F32).workspace;  // (the figure depends on neither D nor the dtype)
}

extern "C" int tdx_attn_bwd(const void* qkv, const void* out, const float* lse, const void* dout, void* dqkv, int B,
                            int N, int H, int D, int dtype, void* workspace, void* stream) {
    TDX_CHECK_ARG(qkv && out && lse && dout && dqkv && workspace && B > 0 && N > 0 && H > 0);
    const AttnPlan p = attn_plan(B, N, H, D, dtype);
    if (p.status != TDX_OK) return p.status;
    float* delta = (float*)workspace;
    const AttnBwdCall c = {qkv, dout, lse, delta, dqkv, B, N, H, dtype, as_stream(stream)};
    const int64_t total = (int64_t)B * N * H;
    TDX_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((attn_delta_kernel<T, FA_D>), dim3(ceil_div(total, 256)), dim3(256), 0, c.st,
                                                  (const T*)out, (const T*)dout, delta, N, H, total));
    return p.bwd == TDX_ATTN_MFMA ? attn_bwd_mfma_launch(c, p) : attn_bwd_vector_launch(c, p);
}
