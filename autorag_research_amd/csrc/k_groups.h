// k_groups.h -- several top-k lists fused into one per group: every row once, at its best value.
//
// One workgroup of 256 threads per group walks the rule in include/mi355dr.h ("grouped search") literally: the group's
// s_g x width (value, row) entries go into LDS as (order key, row) -- the key is dist_to_key of dev_common.h, NaN last; an
// entry without a row is padding -- and are sorted twice.  The first sort, by (row asc, key asc), puts the occurrences of a
// row side by side with its smallest key in front, so "the predecessor has my row" marks every other occurrence; those
// become padding.  The second sort, by (key asc, row asc) with padding last, is the library's total order, and its first
// k_out entries are the result.  Rows stay int64 throughout (row_offset can lift them above 2^31).  Plain sort kernel: no
// communication between workgroups, no global atomics, every loop bounded by the group's padded size np <= kSortMax.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kGroupsThreads = 256;
constexpr int64_t kGroupsNoRow = 0x7FFFFFFFFFFFFFFFll;  // the row of a padding entry: behind every real row in both sorts

inline int groups_pow2(int64_t n) {  // next_pow2 for the host's sizing
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// key[np] | row[np] | the distinct-row counter (16 bytes keep the block a multiple of 16)
__host__ __device__ inline size_t groups_lds_bytes(int np) { return (size_t)np * (sizeof(uint64_t) + sizeof(int64_t)) + 16; }

// The int64-row variant of bitonic_asc_key_row.  BY_ROW: order (row asc, key asc); else (key asc, row asc).  Padding is
// (kKeyNaN, kGroupsNoRow): last under both, and two entries that compare equal are identical, so no swap order matters.
template <bool BY_ROW>
__device__ __forceinline__ bool groups_before(uint64_t k1, int64_t r1, uint64_t k2, int64_t r2) {
    if (BY_ROW) return r1 < r2 || (r1 == r2 && k1 < k2);
    return k1 < k2 || (k1 == k2 && r1 < r2);
}
template <bool BY_ROW>
__device__ __forceinline__ void bitonic_asc_groups(uint64_t* key, int64_t* row, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int p = i ^ j;
                if (p > i) {
                    const bool asc = ((i & k) == 0);
                    const uint64_t ka = key[i], kb = key[p];
                    const int64_t ra = row[i], rb = row[p];
                    if (asc ? groups_before<BY_ROW>(kb, rb, ka, ra) : groups_before<BY_ROW>(ka, ra, kb, rb)) {
                        key[i] = kb;
                        key[p] = ka;
                        row[i] = rb;
                        row[p] = ra;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// grid: one workgroup per group.  vals / rows: [S, width]; group g owns lists offs[g] .. offs[g + 1] - 1.  np_max: the padded
// size the launch's LDS was sized for (the host refuses a call whose largest group exceeds kSortMax).  out_vals / out_rows:
// [G, k_out]; out_count: [G] or null.
__global__ __launch_bounds__(kGroupsThreads) void k_merge_groups(const double* __restrict__ vals, const int64_t* __restrict__ rows,
                                                                 int width, const int32_t* __restrict__ offs, int np_max,
                                                                 int k_out, double* __restrict__ out_vals,
                                                                 int64_t* __restrict__ out_rows, int32_t* __restrict__ out_count) {
    extern __shared__ __align__(16) unsigned char groups_smem[];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x;
    const int l0 = offs[g], l1 = offs[g + 1];
    const int64_t n64 = (int64_t)(l1 - l0) * width;
    double* ov = out_vals + g * k_out;
    int64_t* orow = out_rows + g * k_out;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    // (block-uniform) an empty group; a group the LDS was not sized for never gets past the host's checks
    if (n64 <= 0 || n64 > (int64_t)np_max) {
        for (int t = tid; t < k_out; t += kGroupsThreads) {
            ov[t] = nan;
            orow[t] = -1;
        }
        if (tid == 0 && out_count) out_count[g] = 0;
        return;
    }
    const int n = (int)n64, np = next_pow2(n);  // np <= np_max: np_max is a power of two >= n
    uint64_t* key = (uint64_t*)groups_smem;
    int64_t* row = (int64_t*)(key + np_max);
    int* distinct = (int*)(row + np_max);
    const double* gv = vals + (int64_t)l0 * width;
    const int64_t* gr = rows + (int64_t)l0 * width;

    // ---- 1: (order key, row); an entry without a row is padding, a NaN with a row stays (an irregular row's result)
    if (tid == 0) *distinct = 0;
    for (int i = tid; i < np; i += kGroupsThreads) {
        const int64_t r = i < n ? gr[i] : -1;
        const bool has = r >= 0;
        key[i] = has ? dist_to_key(gv[i]) : kKeyNaN;
        row[i] = has ? r : kGroupsNoRow;
    }
    __syncthreads();
    // ---- 2: occurrences of a row side by side, the smallest key first
    bitonic_asc_groups<true>(key, row, np);
    // ---- 3: every occurrence behind the first becomes padding (np / 256 <= 16 entries per thread: one flag bit each)
    unsigned dup = 0;
    int mine = 0;
    for (int i = tid, j = 0; i < np; i += kGroupsThreads, ++j) {
        const int64_t r = row[i];
        if (r == kGroupsNoRow) continue;
        if (i > 0 && row[i - 1] == r) dup |= 1u << j;
        else ++mine;
    }
    __syncthreads();
    for (int i = tid, j = 0; i < np; i += kGroupsThreads, ++j) {
        if (dup >> j & 1u) {
            key[i] = kKeyNaN;
            row[i] = kGroupsNoRow;
        }
    }
    if (mine) atomicAdd(distinct, mine);  // (LDS)
    __syncthreads();
    // ---- 4: the library's total order, padding last
    bitonic_asc_groups<false>(key, row, np);
    // ---- 5: the first k_out entries; key_to_dist gives a number its own bits back and a NaN the library's NaN
    for (int t = tid; t < k_out; t += kGroupsThreads) {
        const bool has = t < np && row[t] != kGroupsNoRow;
        ov[t] = has ? key_to_dist(key[t]) : nan;
        orow[t] = has ? row[t] : -1;
    }
    if (tid == 0 && out_count) out_count[g] = *distinct;
}

}  // namespace mi355
