// Library-wide host services (defined in tdx_ordered.hip): the environment switches, the ordered sums behind
// TDX_DETERMINISTIC, the CU budget of the persistent kernels, and the per-stream scratch arena.
#pragma once
#include "tdx_common.h"

// The library's environment switches: one row each in the table of tdx_ordered.hip (name, default, accepted values,
// description), in this order.  The only place the library reads the environment.
enum TdxSwitchId {
    SW_ATTN_BOUND,
    SW_ATTN_BWD_TW,
    SW_ATTN_IMPL,
    SW_ATTN_STREAMK,
    SW_CONV1_IMPL,
    SW_CONV3_PERM,
    SW_CONV3_RING,
    SW_CONV3_SMALL,
    SW_CONV3_SMALL_ROWS,
    SW_CONV3_THIN,
    SW_CONVG_MFMA,
    SW_DETERMINISTIC,
    SW_PERSISTENT_CUS,
    SW_RING_LOADERS,
    SW_RING_MIN_ITEMS,
    SW_RING_RAGGED,
    SW_RING_Z4,
    SW_SHELL_DETERMINISTIC,
    SW_SKIP_DGRAD_FUSE,
    SW_SMALL_ZPAD,
    SW_WGRAD_RING,
    SW_WGRAD_SMALL,
    SW_WGRAD_SMALL_ROWS,
    SW_WGRAD_SPLIT_RING,
    SW_COUNT
};
// The switch's value as of now: the environment is read on every call and nothing is cached, so a process may flip a switch
// between two launches.  The whole string must be a decimal integer the row accepts, or the row's word; a variable that is
// unset, empty, unparsable or out of the row's values yields the row's default (TDX_PERSISTENT_CUS alone clamps instead).
int tdx_switch(TdxSwitchId id);
// whether tdx_switch(id) comes from the environment rather than from the row's default
bool tdx_switch_is_set(TdxSwitchId id);

// TDX_DETERMINISTIC=1: the fp32 atomic merges of the backward's small parameter gradients are replaced by per-split partials
// added in a fixed order (tdx_ordered.hip), the halo shell takes its ordered route
bool tdx_deterministic();
// dst[r * ld + c] (+)= sum_{k < nslab} slabs[k * stride + r * cols + c], k ascending
int ordered_sum_launch(const float* slabs, int nslab, int64_t stride, float* dst, int rows, int cols, int64_t ld, bool add,
                       hipStream_t st);
// dbias[c] = sum over the nvox rows of dy[v][c] (NDHWC, C % 8 == 0) in a fixed order; part: >= C floats of scratch (256 C used if there)
size_t bias_grad_ordered_scratch_floats(int C);
int bias_grad_ordered_launch(const void* dy, int64_t nvox, int C, int dtype, float* dbias, float* part, size_t part_floats,
                             hipStream_t st);

// CUs the persistent one-workgroup-per-CU kernels (ring conv, producer / consumer weight gradient) may occupy:
// the TDX_PERSISTENT_CUS switch rounded down to a multiple of 8; [8, 256], default 256.  A data-parallel run
// sets it below 256 to leave CUs to RCCL's kernels.
int tdx_persistent_cus();

// The scratch arena: caller-provided transient workspace (tdx_set_scratch, include/tdx.h) of kernels whose entry points
// have no argument for one.  One arena serves one stream.  Layout:
//   [0, TDX_SCRATCH_ZERO_BYTES)   the zero block: the caller binds it zeroed and no kernel writes it.  The zero source of
//                                 the LDS-DMA kernels (ring conv data gradient, ring weight gradient, small-grid conv).
//   [TDX_SCRATCH_ZERO_BYTES, ..)  transient within ONE entry point's launches: everything past the zero block is dead once
//                                 the entry point's last launch is enqueued, and the next entry point on the stream may reuse
//                                 it from any offset.  Users today: the small-grid conv's K-split slabs and the attention
//                                 forward's key-norm table + stream-K partials start right behind the zero block; the ordered
//                                 (TDX_DETERMINISTIC) partials of GroupNorm, the codecs and the 1x1 weight gradient start at
//                                 TDX_SCRATCH_SLAB_OFFSET.
#define TDX_SCRATCH_ZERO_BYTES 64
#define TDX_SCRATCH_SLAB_OFFSET 256
// the bound arena; nullptr / 0 if none
void* tdx_scratch_ptr();
size_t tdx_scratch_bytes();
// the zero block; nullptr without an arena (tdx_set_scratch refuses one that is smaller than the block)
const void* tdx_scratch_zero();
// `bytes` of the arena from byte `offset` on; nullptr when there is no arena or offset + bytes does not fit
void* tdx_scratch_region(size_t offset, size_t bytes);
