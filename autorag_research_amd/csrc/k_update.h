// k_update.h -- in-place mutation of the single-vector corpus (mi355dr_update_rows / mi355dr_remove_rows).
//   k_update_rows         scatter n new fp32 rows to their slots
//   k_mark_dead           give the removed rows the dead sentinel in nrm2
//   k_rebuild_side_lists  irr_rows / irr8_rows and the count of dead rows, from nrm2 and flag8 over the whole index
// The derived data of the touched rows is rebuilt by the builders add_rows uses, through their id-list forms (k_prep.h):
// k_row_nrm2 (the same k-ascending chain: the bits of an add_rows of the same vector), k_build_shadow (bf16 image; NaN for
// a dead row) and k_build_shadow8 (every touched group of 32 rows whole; a dead row is out of the peak, all-zero, flag 1).
// Reference: the second UPDATE of a chunk's `embedding` (orm/service/base_ingestion.py:199-247) and a row that leaves
// `WHERE embedding IS NOT NULL` (orm/repository/base.py:409-415).
#pragma once
#include "dev_common.h"

namespace mi355 {

// grid: n blocks of 256 threads; row j of src [n, d] -> slot ids[j] of rows (ids are distinct and inside the index: checked
// by the host).  Whole float4 when rows are 16-byte aligned (d % 4 == 0; both bases come from hipMalloc or are checked).
__global__ __launch_bounds__(256) void k_update_rows(const float* __restrict__ src, const int64_t* __restrict__ ids, int64_t n,
                                                      int d, int vec4, float* __restrict__ rows) {
    const int64_t j = blockIdx.x;
    if (j >= n) return;
    const float* s = src + j * (int64_t)d;
    float* t = rows + ids[j] * (int64_t)d;
    if (vec4) {
        const float4* s4 = (const float4*)s;
        float4* t4 = (float4*)t;
        for (int k = threadIdx.x; k < d / 4; k += blockDim.x) t4[k] = s4[k];
    } else {
        for (int k = threadIdx.x; k < d; k += blockDim.x) t[k] = s[k];
    }
}

// grid: ceil(n / 256) blocks of 256 threads
__global__ __launch_bounds__(256) void k_mark_dead(const int64_t* __restrict__ ids, int64_t n, float* __restrict__ nrm2) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) nrm2[ids[j]] = kDeadNrm2;
}

// grid: ceil(n / 256) blocks of 256 threads over rows [row0, row0 + n).  The two side lists hold LIVE rows only:
//   irr_rows   rows whose norm the screens cannot normalise (zero / non-finite / extreme)
//   irr8_rows  rows outside the int8 shadow (flag8: irregular or loose)
// counts keep counting past kIrrCap (the host compares them with the capacity); counts[2] += dead rows.
// The caller zeroes the three counters first.  List order is immaterial: the lists feed candidate lists that are sorted.
__global__ __launch_bounds__(256) void k_rebuild_side_lists(const float* __restrict__ nrm2, const uint8_t* __restrict__ flag8,
                                                             int64_t row0, int64_t n, int32_t* __restrict__ irr_rows,
                                                             int* __restrict__ irr_count, int32_t* __restrict__ irr8_rows,
                                                             int* __restrict__ irr8_count, int* __restrict__ dead_count) {
    __shared__ int s_dead;
    if (threadIdx.x == 0) s_dead = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool dead = false;
    if (j < n) {
        const int64_t i = row0 + j;
        const float n2 = nrm2[i];
        dead = row_is_dead(n2);
        if (!dead) {
            if (!norm_is_regular(n2)) {
                const int slot = atomicAdd(irr_count, 1);
                if (slot < kIrrCap) irr_rows[slot] = (int32_t)i;
            }
            if (flag8[i]) {
                const int slot = atomicAdd(irr8_count, 1);
                if (slot < kIrrCap) irr8_rows[slot] = (int32_t)i;
            }
        }
    }
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(dead));
    if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(&s_dead, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_dead > 0) atomicAdd(dead_count, s_dead);
}

}  // namespace mi355
