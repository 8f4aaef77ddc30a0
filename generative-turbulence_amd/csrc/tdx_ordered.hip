// TDX_DETERMINISTIC=1: run-to-run reproducible parameter gradients.
//
// By default the cross-workgroup merges of the small parameter gradients are fp32 atomics (bias gradients of the 3x3x3 convs,
// weight / bias gradients of the 1x1 convs, of the encoders / decoder and of the first conv): their sums depend on arrival
// order in the last bits (4e-7 relative, profiles/r13_determinism_probe.txt).  With the switch every such merge goes through
// per-split partials that are added in a FIXED order by the two kernels below, and the halo shell takes its ordered route
// (TDX_SHELL_DETERMINISTIC): a training step then produces the same bits every run.  The reference sets no determinism flag
// of its own; under torch the counterpart would be torch.use_deterministic_algorithms.
//
// The f64 atomics of the forward go as well: tdx_conv3_fwd_gn takes the conv and then the statistics pass over its result
// (no moments from the conv epilogues), whose blocks store their own f64 tables for an ordered merge (tdx_groupnorm.hip);
// the loss adds block partials rounded to a 2^-20 grid, on which f64 additions are exact -- order-independent -- up to 2^33.
// tdx_conv3_fwd_partial (the sampler's first conv) does the same: a sampling run is bit-reproducible too.
//
// The other library-wide host services of tdx_runtime.h live here too: the environment switches, the CU budget of the
// persistent kernels, the scratch arena, and the zero fills.
#include "tdx_common.h"
#include "tdx_runtime.h"
#include <errno.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

// ---- environment switches (rules: tdx_runtime.h) ---------------------------------------------------------------------------
enum SwitchKind { SW_RANGE, SW_CLAMP, SW_SET };
struct SwitchRow {
    TdxSwitchId id;
    const char* name;
    int def;
    SwitchKind kind;  // accepted integers: v[0] .. v[1] (SW_RANGE; SW_CLAMP: values outside move to the nearest end), or the four of v
    int v[4];
    const char* word;  // a string accepted beside the integers, or nullptr ...
    int word_value;    // ... and what it stands for
    const char* desc;
};
static constexpr SwitchRow g_switches[] = {
    {SW_ATTN_BOUND, "TDX_ATTN_BOUND", 1, SW_RANGE, {0, 1}, nullptr, 0,
     "0: attention forward checks every tile's maximum instead of skipping under the key-norm bound"},
    {SW_ATTN_BWD_TW, "TDX_ATTN_BWD_TW", 22, SW_SET, {11, 12, 21, 22}, nullptr, 0,
     "attention backward, tiles per wave: tens digit the dQ kernel's, ones digit the dK/dV kernel's"},
    {SW_ATTN_IMPL, "TDX_ATTN_IMPL", 0, SW_RANGE, {0, 1}, "vector", 1,
     "vector: row-wise attention kernels also for long sequences (cross-check)"},
    {SW_ATTN_STREAMK, "TDX_ATTN_STREAMK", 1, SW_RANGE, {0, 1}, nullptr, 0,
     "0: attention forward with one workgroup per query block instead of the stream-K schedule"},
    {SW_CONV1_IMPL, "TDX_CONV1_IMPL", 0, SW_RANGE, {0, 1}, "direct", 1, "direct: vector-ALU 1x1 convs (cross-check)"},
    {SW_CONV3_PERM, "TDX_CONV3_PERM", 1, SW_RANGE, {0, 1}, nullptr, 0,
     "0: main bricks of the 16-bit brick kernels (forward, data and weight gradient) in grid orientation"},
    {SW_CONV3_RING, "TDX_CONV3_RING", 1, SW_RANGE, {0, 2}, nullptr, 0, "ring conv kernel: 0 off, 1 where it pays, 2 wherever legal (tests)"},
    {SW_CONV3_SMALL, "TDX_CONV3_SMALL", 1, SW_RANGE, {0, 1}, nullptr, 0, "0: no small-grid conv kernel (brick kernels instead)"},
    {SW_CONV3_SMALL_ROWS, "TDX_CONV3_SMALL_ROWS", 6000, SW_RANGE, {0, INT_MAX}, nullptr, 0,
     "voxel rows up to which the small-grid conv kernel runs; when set, deep forwards get no larger gate of their own"},
    {SW_CONV3_THIN, "TDX_CONV3_THIN", 1, SW_RANGE, {0, 2}, nullptr, 0,
     "thin remainder bricks: 0 never, 1 on grids of 60000 voxels and more, 2 on every grid (tests)"},
    {SW_CONVG_MFMA, "TDX_CONVG_MFMA", 1, SW_RANGE, {0, 1}, nullptr, 0, "0: general convs of bf16 tensors on the vector-ALU kernels"},
    {SW_DETERMINISTIC, "TDX_DETERMINISTIC", 0, SW_RANGE, {0, 1}, nullptr, 0,
     "1: every merge of a training step in a fixed order (run-to-run reproducible bits)"},
    {SW_PERSISTENT_CUS, "TDX_PERSISTENT_CUS", 256, SW_CLAMP, {8, 256}, nullptr, 0,
     "CUs the persistent one-workgroup-per-CU kernels occupy (used rounded down to a multiple of 8)"},
    {SW_RING_LOADERS, "TDX_RING_LOADERS", 1, SW_RANGE, {0, 1}, nullptr, 0,
     "0: the ring kernel's computing waves issue the copies themselves (bf16; fp16 always has loader waves)"},
    {SW_RING_MIN_ITEMS, "TDX_RING_MIN_ITEMS", 768, SW_RANGE, {0, INT_MAX}, nullptr, 0,
     "(brick, N tile) pairs an 8-deep ring launch must have"},
    {SW_RING_RAGGED, "TDX_RING_RAGGED", 1, SW_RANGE, {0, 1}, nullptr, 0, "0: 8-deep ring kernel on grids of whole bricks only"},
    {SW_RING_Z4, "TDX_RING_Z4", 1, SW_RANGE, {0, 2}, nullptr, 0, "4-deep ring bricks: 0 never, 1 where 8-deep ones do not apply, 2 wherever legal (tests)"},
    {SW_SHELL_DETERMINISTIC, "TDX_SHELL_DETERMINISTIC", 0, SW_RANGE, {0, 1}, nullptr, 0,
     "1: halo-shell term of the data gradient through a fixed-order fold instead of atomics"},
    {SW_SKIP_DGRAD_FUSE, "TDX_SKIP_DGRAD_FUSE", 1, SW_RANGE, {0, 1}, nullptr, 0,
     "0: a projected-skip block's 1x1 input gradient as two launches behind the data gradient, not inside the ring launch"},
    {SW_SMALL_ZPAD, "TDX_SMALL_ZPAD", 1, SW_RANGE, {0, 1}, nullptr, 0, "0: small-grid conv kernel without the padded image stride"},
    {SW_WGRAD_RING, "TDX_WGRAD_RING", 1, SW_RANGE, {0, 2}, nullptr, 0,
     "producer / consumer weight gradient (16-bit): 0 off, 1 on, 2 only its 64-wide form"},
    {SW_WGRAD_SMALL, "TDX_WGRAD_SMALL", 1, SW_RANGE, {0, 1}, nullptr, 0, "0: no packed-K weight gradient on small grids (brick kernel instead)"},
    {SW_WGRAD_SMALL_ROWS, "TDX_WGRAD_SMALL_ROWS", 8000, SW_RANGE, {0, INT_MAX}, nullptr, 0,
     "voxel rows up to which the packed-K weight gradient runs"},
    {SW_WGRAD_SPLIT_RING, "TDX_WGRAD_SPLIT_RING", 1, SW_RANGE, {0, 1}, nullptr, 0,
     "0: no producer / consumer weight gradient for split-precision fp32 (single-role kernel instead)"},
};

static constexpr bool switch_accepts(const SwitchRow& r, long v) {
    if (r.kind == SW_SET) return v == r.v[0] || v == r.v[1] || v == r.v[2] || v == r.v[3];
    return v >= r.v[0] && v <= r.v[1];
}
static constexpr bool switch_table_ok() {
    if (sizeof(g_switches) / sizeof(g_switches[0]) != SW_COUNT) return false;
    for (int i = 0; i < SW_COUNT; ++i) {
        const SwitchRow& r = g_switches[i];
        if (r.id != i || !switch_accepts(r, r.def) || (r.word != nullptr && !switch_accepts(r, r.word_value))) return false;
    }
    return true;
}
static_assert(switch_table_ok(), "a row per TdxSwitchId, in the enum's order, each default among the row's accepted values");

// the value the environment gives the switch; false if it gives none (unset, empty, unparsable, not accepted)
static bool switch_read(const SwitchRow& r, int& value) {
    const char* s = getenv(r.name);
    if (s == nullptr || s[0] == 0) return false;
    if (r.word != nullptr && strcmp(s, r.word) == 0) {
        value = r.word_value;
        return true;
    }
    char* end = nullptr;
    errno = 0;
    long v = strtol(s, &end, 10);
    if (end == s || *end != 0 || errno == ERANGE) return false;
    if (r.kind == SW_CLAMP) v = std::min<long>(std::max<long>(v, r.v[0]), r.v[1]);
    if (!switch_accepts(r, v)) return false;
    value = (int)v;
    return true;
}
int tdx_switch(TdxSwitchId id) {
    int v;
    return switch_read(g_switches[id], v) ? v : g_switches[id].def;
}
bool tdx_switch_is_set(TdxSwitchId id) {
    int v;
    return switch_read(g_switches[id], v);
}
extern "C" int tdx_switch_count(void) { return SW_COUNT; }
extern "C" const char* tdx_switch_name(int i) { return i >= 0 && i < SW_COUNT ? g_switches[i].name : nullptr; }
extern "C" int tdx_switch_default(int i) { return i >= 0 && i < SW_COUNT ? g_switches[i].def : 0; }
extern "C" int tdx_switch_value(int i) {
    if (i < 0 || i >= SW_COUNT) return 0;
    return i == SW_PERSISTENT_CUS ? tdx_persistent_cus() : tdx_switch((TdxSwitchId)i);
}

int tdx_persistent_cus() { return tdx_switch(SW_PERSISTENT_CUS) & ~7; }

// ---- scratch arena (layout and the rule of its reuse: tdx_runtime.h) ----------------------------------------------------
static void* g_scratch = nullptr;
static size_t g_scratch_bytes = 0;
void* tdx_scratch_ptr() { return g_scratch; }
size_t tdx_scratch_bytes() { return g_scratch_bytes; }
const void* tdx_scratch_zero() { return g_scratch; }
void* tdx_scratch_region(size_t offset, size_t bytes) {
    if (g_scratch == nullptr || offset > g_scratch_bytes || bytes > g_scratch_bytes - offset) return nullptr;
    return (char*)g_scratch + offset;
}
extern "C" int tdx_set_scratch(void* ptr, size_t bytes) {
    if (ptr != nullptr && bytes < TDX_SCRATCH_ZERO_BYTES) return TDX_EINVAL;  // at least the zero block
    g_scratch = ptr;
    g_scratch_bytes = ptr ? bytes : 0;
    return TDX_OK;
}

bool tdx_deterministic() { return tdx_switch(SW_DETERMINISTIC) != 0; }

// dst[r * ld + c] (+)= sum_k slabs[k * stride + r * cols + c], k ascending.  One element per 32 lanes when there are many
// slabs (lane l adds slabs l, l + 32, ... in order, then a fixed butterfly), else one element per thread.
template <int LPE>
__global__ void __launch_bounds__(256) ordered_sum_kernel(const float* __restrict__ slabs, int nslab, int64_t stride,
                                                         float* __restrict__ dst, int64_t n, int cols, int64_t ld, int add) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = gid / LPE;
    const int l = (int)(gid % LPE);
    float v = 0.f;
    if (e < n) {
        const float* p = slabs + e;
        int k = l;
        for (; k + 3 * LPE < nslab; k += 4 * LPE) {  // four loads in flight, added in slab order
            const float a = p[(int64_t)k * stride], b = p[(int64_t)(k + LPE) * stride], c = p[(int64_t)(k + 2 * LPE) * stride],
                        d = p[(int64_t)(k + 3 * LPE) * stride];
            v = (((v + a) + b) + c) + d;
        }
        for (; k < nslab; k += LPE) v += p[(int64_t)k * stride];
    }
    if (LPE > 1) {
#pragma unroll
        for (int o = LPE / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);  // same tree every run; all lanes end with the sum
    }
    if (e < n && l == 0) {
        float* d = dst + (e / cols) * ld + (e % cols);
        *d = add ? *d + v : v;
    }
}

int ordered_sum_launch(const float* slabs, int nslab, int64_t stride, float* dst, int rows, int cols, int64_t ld, bool add,
                       hipStream_t st) {
    const int64_t n = (int64_t)rows * cols;
    if (n <= 0 || nslab <= 0) return TDX_OK;
    if (nslab > 32)
        hipLaunchKernelGGL(ordered_sum_kernel<32>, dim3((unsigned)ceil_div(n * 32, (int64_t)256)), dim3(256), 0, st, slabs, nslab, stride,
                           dst, n, cols, ld, add ? 1 : 0);
    else
        hipLaunchKernelGGL(ordered_sum_kernel<1>, dim3((unsigned)ceil_div(n, (int64_t)256)), dim3(256), 0, st, slabs, nslab, stride, dst, n,
                           cols, ld, add ? 1 : 0);
    return tdx_launch_status();
}

// Bias gradient of a conv over an NDHWC gradient: dbias[c] = sum_v dy[v][c], in a fixed order.
// Pass 1: block b sums voxels [b * vpb, (b + 1) * vpb) -- a thread walks its voxels (v0 + r, v0 + r + rows, ...) for its 8
// channels, the block's rows are added in row order through LDS -> part[b][C].  Pass 2: ordered_sum over the blocks.
#define OB_THREADS 256
template <typename T>
__global__ void __launch_bounds__(OB_THREADS) bias_partial_kernel(const T* __restrict__ dy, int64_t nvox, int C, int64_t vpb,
                                                                  float* __restrict__ part) {
    __shared__ float red[OB_THREADS][9];
    const int L = C >> 3, rows = OB_THREADS / L;
    const int lc = threadIdx.x % L, r = threadIdx.x / L;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    const int64_t v0 = (int64_t)blockIdx.x * vpb, v1 = min(nvox, v0 + vpb);
    if (r < rows)
        for (int64_t v = v0 + r; v < v1; v += rows) {
            Vec8<T> g;
            g.load(dy + v * C + lc * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += g.v[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = r < rows ? s[j] : 0.f;
    __syncthreads();
    for (int o = threadIdx.x; o < C; o += OB_THREADS) {
        const int l = o >> 3, j = o & 7;
        float t = 0.f;
        for (int q = 0; q < rows; ++q) t += red[q * L + l][j];
        part[(int64_t)blockIdx.x * C + o] = t;
    }
}

size_t bias_grad_ordered_scratch_floats(int C) { return (size_t)256 * C; }

int bias_grad_ordered_launch(const void* dy, int64_t nvox, int C, int dtype, float* dbias, float* part, size_t part_floats,
                             hipStream_t st) {
    if ((C % 8) || C > 8 * OB_THREADS || part_floats < (size_t)C) return TDX_ESHAPE;
    int64_t nblk = std::min<int64_t>(256, (int64_t)(part_floats / C));
    int64_t vpb = ceil_div(nvox, nblk);
    vpb = vpb < 64 ? 64 : vpb;
    nblk = ceil_div(nvox, vpb);
    TDX_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((bias_partial_kernel<T>), dim3((unsigned)nblk), dim3(OB_THREADS), 0, st, (const T*)dy,
                                                  nvox, C, vpb, part));
    int rc = tdx_launch_status();
    if (rc != TDX_OK) return rc;
    return ordered_sum_launch(part, (int)nblk, C, dbias, 1, C, C, false, st);
}

// ---- zero fill as a KERNEL ------------------------------------------------------------------------------------------------
// hipMemsetAsync inside a captured hipGraph becomes a memset node, and on this runtime a small memset node is not ordered
// against EARLIER kernel nodes that still write the previous owner of the same (graph-pool) memory: replayed, the fill can land
// before such a late write, which then sits in the freshly "zeroed" accumulator -- one garbage element in the encoder / decoder
// gradients from the second replay of a captured training step on, found when the captured step stopped forking its weight
// gradients onto a side stream (which had hidden it: record_stream kept those blocks from being reused).  torch itself zeroes
// with fill kernels.  Every zero fill of the library goes through these two launches; a kernel node is ordered like any other.
__global__ void __launch_bounds__(256) zero_bytes_kernel(unsigned char* __restrict__ p, size_t bytes) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i >= bytes) return;
    if (i + 16 <= bytes && (reinterpret_cast<uintptr_t>(p + i) & 15) == 0) {
        *reinterpret_cast<uint4*>(p + i) = make_uint4(0, 0, 0, 0);
    } else {
        const size_t e = i + 16 < bytes ? i + 16 : bytes;
        for (size_t k = i; k < e; ++k) p[k] = 0;
    }
}
__global__ void __launch_bounds__(256) zero_rows_kernel(unsigned char* __restrict__ p, size_t pitch, size_t width, size_t rows) {
    const size_t per_row = (width + 3) / 4;  // 4-byte pieces (width and pitch are multiples of 4: fp32 matrices)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_row * rows) return;
    const size_t r = i / per_row, c = (i - r * per_row) * 4;
    *reinterpret_cast<unsigned*>(p + r * pitch + c) = 0u;
}
int tdx_zero_async(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return TDX_OK;
    hipLaunchKernelGGL(zero_bytes_kernel, dim3((unsigned)((bytes + 4095) / 4096)), dim3(256), 0, st, (unsigned char*)p, bytes);
    return tdx_launch_status();
}
int tdx_zero2d_async(void* p, size_t pitch, size_t width, size_t rows, hipStream_t st) {
    if (width == 0 || rows == 0) return TDX_OK;
    if ((pitch % 4) || (width % 4) || (reinterpret_cast<uintptr_t>(p) % 4)) return TDX_EINVAL;
    const size_t n = (width / 4) * rows;
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (unsigned char*)p, pitch, width, rows);
    return tdx_launch_status();
}
