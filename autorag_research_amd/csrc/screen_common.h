// screen_common.h -- what all four screen kernels (k_screen, k_screen_stream, k_screen256c, k_screen_rq) share: the operand
// and accumulator register types, the staged-row geometry, the launch arguments, the LDS-DMA and MFMA primitives and the
// per-block constants of the int8 screen.  The hit paths (what a kernel does with a value that passes its threshold) are in
// screen_hits.h; the kernels in their own headers.
#pragma once
#include "dev_common.h"

namespace mi355 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileM = 128;  // corpus rows per workgroup tile (k_screen, k_screen_stream)
constexpr int kTileN = 128;  // queries per workgroup tile (k_screen)
constexpr int kStepK = 64;   // bf16 elements per K step (128 B)
constexpr int kRowB = 128;   // bytes per staged row

struct ScreenArgs {
    const void* shadow;      // [rows_pad, row_bytes]  bf16 (2 B/element) or int8 shadow rows
    const void* qhat;        // [Bpad, row_bytes]      same element type
    const float* thr;        // [Bpad]  emit iff v >= thr  (bf16: v = t; int8: v = S_q S_g acc + e_g kq, dev_common.h)
    const float* sc;         // [Bpad]  int8 screen: the query's step S_q
    const float* kq;         // [Bpad]  int8 screen: factor on the row group's residual norm
    const I8Group* grp;      // [rows_pad / 32]  int8 screen: step and residual norm of every group of 32 rows
    const uint8_t* flag8;    // [rows]  int8 screen: 1 = row is not in the int8 shadow (read by the emit-all epilogue only)
    int* cnt;                // [Bpad]
    int32_t* cand_row;       // [Bpad, cap]
    float* cand_val;         // [Bpad, cap]
    int row_bytes;           // bytes per shadow row (a multiple of 128)
    int ksteps;              // row_bytes / 128: K steps of 64 bf16 or 128 int8
    int cap;
    int ct0;        // first corpus tile of this chunk
    int n_ctiles;   // corpus tiles in this chunk
    int n_qtiles;   // query tiles
    int64_t row_end;  // rows >= row_end are not part of this chunk (tile padding)
    int64_t row0;     // first row of this chunk
    int emit_all;     // 1 = first chunk: every (query,row) is a candidate -> direct store at slot row-row0, no atomics;
                      // 2 = starter (k_screen only): per query and 64-row slab ONLY the largest value, at slot (slab index)
    float* moments;   // starter of a speculative pass (else nullptr): [Bpad, moment_slabs, 2] sum and sum of squares of the
    int moment_slabs; // slab's screen values, per query -- the sample the model threshold is predicted from (k_select.h)
};
constexpr int kEmitAll = 1, kEmitSlabMax = 2;
constexpr int kSlabRows = 64;  // rows of one wave's sub-tile in k_screen: the starter keeps one candidate per slab and query

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// one 32x32 MFMA step on 16-byte operand fragments (carried as bf16x8 registers): 16 bf16 k-values (I8 = false)
// or 32 int8 k-values (I8 = true).
// The int8 form accumulates exact int32; its accumulator travels in the same f32x16 registers (bit pattern).
template <bool I8>
__device__ __forceinline__ f32x16 screen_mfma(bf16x8 fa, bf16x8 fb, f32x16 acc) {
    if constexpr (I8) {
        return __builtin_bit_cast(f32x16, __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, fa),
                                                                                __builtin_bit_cast(i32x4, fb),
                                                                                __builtin_bit_cast(i32x16, acc), 0, 0, 0));
    } else {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
    }
}

// int8 screen: the two per-lane constants of one 32x32 accumulator block (32 rows = one I8Group, 32 queries = the lanes):
// v = fma((float)acc, m, ek).  `g` is wave-uniform (a scalar load), sq / kq are the lane's query.
struct I8Blk {
    float m, ek;
};
__device__ __forceinline__ I8Blk i8_blk(const I8Group g, float sq, float kq) { return I8Blk{g.step * sq, g.err * kq}; }
__device__ __forceinline__ float i8_value(int acc, const I8Blk& b) { return __builtin_fmaf((float)acc, b.m, b.ek); }
// the group record of the block whose first row is row0 (a multiple of 32), through the scalar data cache: the address is
// wave-uniform, and the constant address space tells the compiler that nothing in this kernel writes it
__device__ __forceinline__ I8Group i8_group_of(const I8Group* grp, int64_t row0) {
    typedef const __attribute__((address_space(4))) float cfloat;
    cfloat* p = (cfloat*)(const float*)(grp + (row0 >> 5));
    return I8Group{p[0], p[1]};
}

// 32-bit LDS address of a pointer into dynamic shared memory
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long)((const __attribute__((address_space(3))) char*)p);
}

}  // namespace mi355
