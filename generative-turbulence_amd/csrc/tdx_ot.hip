// Batched exact W2^2 between equally sized, uniformly weighted point sets (the inner problems of
// WassersteinMetric, turbdiff/models/metrics.py:520-567): with uniform weights the optimum of ot.emd2 is reached
// at a permutation (Birkhoff), so each job is a linear assignment problem, solved here by the epsilon-scaling
// auction (Bertsekas) with Jacobi bidding.
//
// Job (i, j, k): persons p are the cells idx[offsets[k] + p] of feature set A[i], objects q the same cells of B[j];
// c_pq = ||A_i[p] - B_j[q]||^2 in fp32, computed on the fly (never materialised).  Layout: one workgroup of four
// waves per job, a persistent grid of `slots` workgroups walking the job list, each with its own slice of the
// workspace.  In a round every unassigned person (one wave each) scans all objects for its best and second-best
// reduced cost c_pq + price_q and bids price_q1 + (r2 - r1) + eps on its best object.  Bids are resolved without
// any order dependence: a vector 64-bit atomic max of the (positive) bid's bits per object, then a vector atomic
// min of the person index among the bids equal to that maximum -- the higher bid wins, on equal bids the lower
// person; prices and bids are fp64.  Every phase starts from an empty assignment with the previous prices and
// eps divided by 8, from eps = S down to eps_final = rel_eps * S, where S (computed per job on the device) is
// (1/n) sum ||x - m||^2 over both sets around their pooled mean m -- for any coupling of the two sets the mean
// cost is at most 2 S, and the independent coupling's is S plus half the squared distance of the set means.
//
// Output per job: the primal (1/n) sum_p c_{p, sigma(p)}, the dual bound (1/n)[sum_p min_q (c_pq + pi_q) - sum_q pi_q]
// (<= the optimum), eps_final and the number of bids.  epsilon-complementary slackness of the final phase gives
// 0 <= primal - dual <= eps_final: the optimality certificate is computed by the kernel itself.
// Every loop is bounded: a phase stops after max_rounds rounds, a job after max_bids bids, with an error status
// (the job's values are NaN); nothing spins.  Sums are formed in a fixed order, so results are bit-reproducible.
#include "tdx_common.h"

#include <climits>

namespace {

constexpr int OT_THREADS = 256;
constexpr int OT_WAVES = OT_THREADS / 64;
constexpr int OT_MAX_PHASES = 64;

__host__ __device__ inline size_t ot_align(size_t b) { return (b + 255) & ~(size_t)255; }

__host__ __device__ inline size_t ot_slot_bytes(int max_n) {
    const size_t n = (size_t)max_n;
    return 2 * ot_align(n * 32) + 3 * ot_align(n * 8) + 6 * ot_align(n * 4);
}

struct Slot {
    float* a;                  // persons' features, (n, 8)
    float* b;                  // objects' features, (n, 8)
    double* price;             // (n)
    unsigned long long* bmax;  // highest bid on each object this round, fp64 bits (0 = none)
    double* bid_val;           // bid of the t-th bidder of the round
    int* winner;               // lowest person index among the highest bids (INT_MAX = none)
    int* owner;                // object -> person (-1 = free)
    int* assigned;             // person -> object (-1 = unassigned)
    int* list[2];              // unassigned persons: this round's, next round's
    int* bid_obj;              // object of the t-th bidder's bid
};

__device__ Slot slot_at(void* ws, int max_n, int s) {
    char* p = (char*)ws + (size_t)s * ot_slot_bytes(max_n);
    const size_t n = (size_t)max_n;
    Slot sl;
    sl.a = (float*)p;                  p += ot_align(n * 32);
    sl.b = (float*)p;                  p += ot_align(n * 32);
    sl.price = (double*)p;             p += ot_align(n * 8);
    sl.bmax = (unsigned long long*)p;  p += ot_align(n * 8);
    sl.bid_val = (double*)p;           p += ot_align(n * 8);
    sl.winner = (int*)p;               p += ot_align(n * 4);
    sl.owner = (int*)p;                p += ot_align(n * 4);
    sl.assigned = (int*)p;             p += ot_align(n * 4);
    sl.list[0] = (int*)p;              p += ot_align(n * 4);
    sl.list[1] = (int*)p;              p += ot_align(n * 4);
    sl.bid_obj = (int*)p;
    return sl;
}

__device__ __forceinline__ float cost8(const float a[8], const float* __restrict__ b) {
    const float4 b0 = reinterpret_cast<const float4*>(b)[0], b1 = reinterpret_cast<const float4*>(b)[1];
    const float d[8] = {a[0] - b0.x, a[1] - b0.y, a[2] - b0.z, a[3] - b0.w, a[4] - b1.x, a[5] - b1.y, a[6] - b1.z, a[7] - b1.w};
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(d[e], d[e], s);
    return s;
}

__device__ __forceinline__ void load8(const float* __restrict__ p, float a[8]) {
    const float4 a0 = reinterpret_cast<const float4*>(p)[0], a1 = reinterpret_cast<const float4*>(p)[1];
    a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w;
    a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
}

// deterministic sum over the workgroup (xor butterfly in each wave, the four wave sums in order); result in all threads
__device__ double block_sum(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// best (lowest reduced cost, lower object on ties) and second-best value of person a against all objects; wave-uniform
__device__ void scan_best(const float a[8], const Slot& sl, int n, double& r1, int& q1, double& r2) {
    const int lane = threadIdx.x & 63;
    r1 = INFINITY; r2 = INFINITY; q1 = INT_MAX;
    for (int q = lane; q < n; q += 64) {
        const double r = (double)cost8(a, sl.b + (size_t)q * 8) + sl.price[q];
        if (r < r1) { r2 = r1; r1 = r; q1 = q; }
        else if (r < r2) r2 = r;
    }
    if (q1 >= n) q1 = 0;  // no finite candidate in this lane (the host refuses non-finite features; never an index past n)
    for (int off = 32; off > 0; off >>= 1) {
        const double o1 = __shfl_xor(r1, off, 64), o2 = __shfl_xor(r2, off, 64);
        const int oq = __shfl_xor(q1, off, 64);
        const double second = fmin(fmax(r1, o1), fmin(r2, o2));
        if (o1 < r1 || (o1 == r1 && oq < q1)) { r1 = o1; q1 = oq; }
        r2 = second;
    }
}

__device__ double scan_min(const float a[8], const Slot& sl, int n) {
    const int lane = threadIdx.x & 63;
    double r1 = INFINITY;
    for (int q = lane; q < n; q += 64) r1 = fmin(r1, (double)cost8(a, sl.b + (size_t)q * 8) + sl.price[q]);
    for (int off = 32; off > 0; off >>= 1) r1 = fmin(r1, __shfl_xor(r1, off, 64));
    return r1;
}

__global__ void __launch_bounds__(OT_THREADS)
ot_auction_kernel(const float* __restrict__ fa, const float* __restrict__ fb, int64_t n_cells, const int* __restrict__ idx,
                  const int* __restrict__ offsets, int K, const int* __restrict__ jobs, int J, int Sa, int Sb, double rel_eps,
                  int max_rounds, int64_t max_bids, void* ws, int max_n, double* __restrict__ out, int* __restrict__ status) {
    __shared__ double red[OT_WAVES];
    __shared__ int next_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Slot sl = slot_at(ws, max_n, blockIdx.x);

    for (int job = blockIdx.x; job < J; job += gridDim.x) {
        const int i = jobs[3 * job], j = jobs[3 * job + 1], k = jobs[3 * job + 2];
        double* o = out + 4 * (size_t)job;
        if (i < 0 || i >= Sa || j < 0 || j >= Sb || k < 0 || k >= K || offsets[k + 1] - offsets[k] > max_n ||
            offsets[k + 1] < offsets[k]) {
            if (tid == 0) { o[0] = o[1] = o[2] = NAN; o[3] = 0.0; status[job] = TDX_OT_BAD_JOB; }
            continue;
        }
        const int off = offsets[k], n = offsets[k + 1] - offsets[k];
        if (n == 0) {  // a region of weight 0
            if (tid == 0) { o[0] = o[1] = o[2] = o[3] = 0.0; status[job] = TDX_OT_OK; }
            continue;
        }
        // gather both point sets; empty bid state
        const float* A = fa + (size_t)i * n_cells * 8;
        const float* B = fb + (size_t)j * n_cells * 8;
        for (int p = tid; p < n; p += OT_THREADS) {
            const int64_t c = idx[off + p];
            const float4* sa = reinterpret_cast<const float4*>(A + c * 8);
            const float4* sb = reinterpret_cast<const float4*>(B + c * 8);
            float4* da = reinterpret_cast<float4*>(sl.a + (size_t)p * 8);
            float4* db = reinterpret_cast<float4*>(sl.b + (size_t)p * 8);
            da[0] = sa[0]; da[1] = sa[1];
            db[0] = sb[0]; db[1] = sb[1];
            sl.price[p] = 0.0;
            sl.bmax[p] = 0ull;
            sl.winner[p] = INT_MAX;
        }
        __syncthreads();

        // cost scale S = (1/n) sum over both sets of ||x - m||^2, m the pooled mean
        double m[8], S = 0.0;
        for (int e = 0; e < 8; ++e) {
            double v = 0.0;
            for (int p = tid; p < n; p += OT_THREADS) v += (double)sl.a[(size_t)p * 8 + e] + (double)sl.b[(size_t)p * 8 + e];
            m[e] = block_sum(v, red) / (2.0 * n);
        }
        {
            double v = 0.0;
            for (int p = tid; p < n; p += OT_THREADS)
                for (int e = 0; e < 8; ++e) {
                    const double da = (double)sl.a[(size_t)p * 8 + e] - m[e], db = (double)sl.b[(size_t)p * 8 + e] - m[e];
                    v += da * da + db * db;
                }
            S = block_sum(v, red) / n;
        }
        const double eps_final = rel_eps * S;

        int st = (S < 1e300) ? TDX_OT_OK : TDX_OT_NONFINITE;  // S is NaN or inf: no finite scale to work at
        int64_t bids = 0;
        if (st != TDX_OT_OK) {
        } else if (n == 1 || S == 0.0) {
            // a single pair, or all points equal (every cost 0): the identity is optimal
            for (int p = tid; p < n; p += OT_THREADS) sl.assigned[p] = p;
            __syncthreads();
        } else {
            double eps = S;
            for (int phase = 0; phase < OT_MAX_PHASES && st == TDX_OT_OK; ++phase) {
                eps = fmax(eps, eps_final);
                for (int p = tid; p < n; p += OT_THREADS) {
                    sl.assigned[p] = -1;
                    sl.owner[p] = -1;
                    sl.list[0][p] = p;
                }
                __syncthreads();
                int cnt = n, cur = 0;
                for (int round = 0; cnt > 0; ++round) {
                    if (round >= max_rounds) { st = TDX_OT_ROUND_CAP; break; }
                    if (bids + cnt > max_bids) { st = TDX_OT_BID_CAP; break; }
                    bids += cnt;
                    const int* L = sl.list[cur];
                    int* Ln = sl.list[cur ^ 1];
                    // bidding: one wave per unassigned person
                    for (int t = wave; t < cnt; t += OT_WAVES) {
                        float a[8];
                        load8(sl.a + (size_t)L[t] * 8, a);
                        double r1, r2;
                        int q1;
                        scan_best(a, sl, n, r1, q1, r2);
                        if (lane == 0) {
                            const double bid = sl.price[q1] + (r2 - r1) + eps;
                            sl.bid_obj[t] = q1;
                            sl.bid_val[t] = bid;
                            atomicMax(&sl.bmax[q1], (unsigned long long)__double_as_longlong(bid));
                        }
                    }
                    if (tid == 0) next_cnt = 0;
                    __syncthreads();
                    // among the highest bids on an object, the lowest person index wins
                    for (int t = tid; t < cnt; t += OT_THREADS) {
                        const int q = sl.bid_obj[t];
                        if ((unsigned long long)__double_as_longlong(sl.bid_val[t]) == atomicAdd(&sl.bmax[q], 0ull))
                            atomicMin(&sl.winner[q], L[t]);
                    }
                    __syncthreads();
                    // winners take their objects (and displace the previous owners); losers stay unassigned
                    for (int t = tid; t < cnt; t += OT_THREADS) {
                        const int p = L[t], q = sl.bid_obj[t];
                        if (atomicAdd(&sl.winner[q], 0) == p) {
                            const int prev = sl.owner[q];
                            sl.owner[q] = p;
                            sl.assigned[p] = q;
                            sl.price[q] = sl.bid_val[t];
                            if (prev >= 0) {
                                sl.assigned[prev] = -1;
                                Ln[atomicAdd(&next_cnt, 1)] = prev;
                            }
                        } else {
                            Ln[atomicAdd(&next_cnt, 1)] = p;
                        }
                    }
                    __syncthreads();
                    for (int t = tid; t < cnt; t += OT_THREADS) {
                        const int q = sl.bid_obj[t];
                        atomicExch(&sl.bmax[q], 0ull);
                        atomicExch(&sl.winner[q], INT_MAX);
                    }
                    cnt = next_cnt;
                    cur ^= 1;
                    __syncthreads();
                }
                if (eps <= eps_final) break;
                eps = eps / 8.0;
            }
        }
        if (st != TDX_OT_OK) {
            if (tid == 0) { o[0] = o[1] = NAN; o[2] = eps_final; o[3] = (double)bids; status[job] = st; }
            __syncthreads();
            continue;
        }
        // certificate: primal, sum of prices, sum_p min_q (c_pq + pi_q)
        double vp = 0.0, vpi = 0.0;
        for (int p = tid; p < n; p += OT_THREADS) {
            float a[8];
            load8(sl.a + (size_t)p * 8, a);
            vp += (double)cost8(a, sl.b + (size_t)sl.assigned[p] * 8);
            vpi += sl.price[p];
        }
        const double primal = block_sum(vp, red), sum_pi = block_sum(vpi, red);
        double vd = 0.0;
        for (int p = wave; p < n; p += OT_WAVES) {
            float a[8];
            load8(sl.a + (size_t)p * 8, a);
            vd += scan_min(a, sl, n);
        }
        if (lane != 0) vd = 0.0;  // the wave-uniform partial counts once
        const double dual = block_sum(vd, red);
        if (tid == 0) {
            o[0] = primal / n;
            o[1] = (dual - sum_pi) / n;
            o[2] = eps_final;
            o[3] = (double)bids;
            status[job] = TDX_OT_OK;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" size_t tdx_ot_workspace_bytes(int max_n, int slots) {
    if (max_n <= 0 || slots <= 0) return 0;
    return ot_slot_bytes(max_n) * (size_t)slots;
}

extern "C" int tdx_ot_auction(const float* fa, const float* fb, int64_t n_cells, const int* idx, const int* offsets, int K,
                              const int* jobs, int J, int Sa, int Sb, double rel_eps, int max_rounds, int64_t max_bids,
                              void* workspace, int max_n, int slots, double* out, int* status, void* stream) {
    TDX_CHECK_ARG(fa && fb && idx && offsets && jobs && workspace && out && status);
    TDX_CHECK_ARG(n_cells > 0 && K > 0 && J > 0 && Sa > 0 && Sb > 0 && max_n > 0 && slots > 0);
    TDX_CHECK_ARG(rel_eps > 0.0 && max_rounds > 0 && max_bids > 0);
    hipLaunchKernelGGL(ot_auction_kernel, dim3(slots < J ? slots : J), dim3(OT_THREADS), 0, as_stream(stream), fa, fb, n_cells,
                       idx, offsets, K, jobs, J, Sa, Sb, rel_eps, max_rounds, max_bids, workspace, max_n, out, status);
    return tdx_launch_status();
}
