// Device helpers shared by the matrix-core kernels (gfx950): the vector types of MFMA fragments, the transposed LDS
// fragment read, the swizzled LDS row layouts, the register <-> row map of a 32 x 32 accumulator tile and the fragments
// made from registers or global rows, the fp32 -> bf16 hi / lo split, one LDS-DMA instruction, and the workgroup barrier
// behind an LDS wait.  Everything here is __forceinline__ and format-agnostic: 16-bit operands travel as raw words in
// bf16x8, in the attention kernels too; H16<HF> (tdx_common.h) picks the MFMA opcode and the rounding, and its bit-cast
// of the words costs no instruction.
#pragma once
#include "tdx_common.h"

typedef bf16x8_t bf16x8;
typedef f32x16_t f32x16;
typedef f32x4_t f32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// Transposed fragment read of K-major 16-bit rows (ds_read_b64_tr_b16): each of the two reads takes 4 rows x 16 columns
// per 16-lane group and delivers them column-major, so the lane ends up with 8 consecutive k of its column: rows
// lo .. lo + 3 and hi .. hi + 3 (the callers pass hi = lo + 4 rows).
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* lo, const unsigned char* hi) {
    s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lo));
    s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(hi));
    s16x8 r = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, r);
}

// Swizzled LDS tiles whose 16-B chunks are read as ds_read_b128 fragments without bank conflicts: byte offset of chunk c of
// row r.  64-B rows (32 16-bit elements, 4 chunks): chunk position c ^ ((r >> 2) & 3)
__device__ __forceinline__ int sw64(int r, int c) { return r * 64 + ((c ^ ((r >> 2) & 3)) << 4); }
// 128-B rows (64 elements, 8 chunks): chunk position c ^ (r & 7)
__device__ __forceinline__ int sw128(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// Row of a 32 x 32 accumulator tile (v_mfma_f32_32x32x*) that register i of a lane in half hh = lane >> 5 holds; the
// column is lane & 31.  Registers 4 j .. 4 j + 3 are the consecutive rows 8 j + 4 hh .. + 3.  base: the tile's first row in
// whatever the caller counts (added first, as the kernels always wrote it: the sum's order decides the instructions).
template <typename B = int>
__device__ __forceinline__ B acc_row(int i, int hh, B base = 0) { return base + (i & 3) + 8 * (i >> 2) + 4 * hh; }

// Accumulator registers 8 s .. 8 s + 7 of a 32 x 32 tile, rounded to the format: the B operand of k step s of a product
// that sums over the tile's rows (by acc_row the lane's 8 registers are k = 16 s + 8 (j >> 2) + 4 hh + (j & 3): the A operand
// comes from tr_frag with the two reads 8 rows apart)
template <typename H>
__device__ __forceinline__ bf16x8 acc_as_b(const f32x16& t, int s) {
    return __builtin_bit_cast(bf16x8, make_uint4(H::pack2(t[8 * s], t[8 * s + 1]), H::pack2(t[8 * s + 2], t[8 * s + 3]),
                                                 H::pack2(t[8 * s + 4], t[8 * s + 5]), H::pack2(t[8 * s + 6], t[8 * s + 7])));
}

// 8 consecutive elements of a global row, times `scale`, rounded to the format again: a B operand (col = the lane's row,
// k = the 8 elements)
template <typename H>
__device__ __forceinline__ bf16x8 row_frag(const typename H::T* row, float scale) {
    Vec8<typename H::T> v;
    v.load(row);
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = H::pack2(v.v[2 * e] * scale, v.v[2 * e + 1] * scale);
    return __builtin_bit_cast(bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
}

// Split precision: 8 fp32 -> 8 bf16 hi (= bf16(v)) and 8 bf16 lo (= bf16(v - hi)), packed two per word
__device__ __forceinline__ void split8(const float4& a, const float4& b, uint4& hi, uint4& lo) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
        const float r0 = v[2 * i] - __uint_as_float(h[i] << 16), r1 = v[2 * i + 1] - __uint_as_float(h[i] & 0xffff0000u);
        l[i] = pack_bf16x2(r0, r1);
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}

// LDS byte address of a pointer into shared memory
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p;
}

// One LDS-DMA instruction (global_load_lds_dwordx4): every lane copies 16 B from its own global address to LDS byte
// address lds + 16 * lane (lds is made wave-uniform here).  Inline assembly, not the builtin: the compiler treats the
// builtin as a store to LDS that any later ds_read might alias and puts s_waitcnt vmcnt(0) in front of the NEXT fragment
// read, which serialises the copy of buffer i + 1 with the MFMAs of buffer i, the opposite of double buffering.  The
// kernels order the copies themselves (s_waitcnt vmcnt(0) + barrier before a buffer is read).  The instruction takes its
// LDS base from M0, which is compiler-reserved: it is saved and restored inside the statement, instead of an "m0" clobber
// that the compiler does not honour.
__device__ __forceinline__ void lds_dma16(const void* gsrc, unsigned lds) {
    lds = __builtin_amdgcn_readfirstlane(lds);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds) : "memory");
}

// Workgroup barrier that this wave's LDS stores (and reads) have been performed before: what a producer / consumer
// kernel puts between "buffer written" and "buffer read" when the compiler does not know the two are related
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// the same, and this wave's global loads have landed too (loader waves that stage through registers)
__device__ __forceinline__ void vmem_lds_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
