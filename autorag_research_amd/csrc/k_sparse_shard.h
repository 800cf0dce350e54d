// k_sparse_shard.h -- the device side of the row-sharded sparse searches.  Each kernel sits on one
// side of an all-gather, like those of k_shard.h:
//   k_sparse_stats_fold    the ranks' statistics payloads [world][words] summed into one row (exact: they are integers)
//   k_sparse_final_packed  k_sparse_final's lines written as this rank's packed [2][nb][k] int64 block (plane 0 the
//                          distance bits, plane 1 the global ids): what mi355dr_merge_topk_packed_device reads
//   k_sparse_fold_scores   the score forms: per position the value of the lowest rank whose value is not NaN
// One thread per word, consecutive threads on consecutive words: every load and store is a coalesced 8-byte vector access.
#pragma once
#include "k_sparse.h"

namespace mi355 {

constexpr long long kSparseNaNBits = 0x7FF8000000000000ll;

// grid: ceil(words / kSparseThreads).  all: [world][words]
__global__ __launch_bounds__(kSparseThreads) void k_sparse_stats_fold(const int64_t* __restrict__ all, int64_t words, int world,
                                                                      int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
    if (i >= words) return;
    int64_t sum = 0;
    for (int r = 0; r < world; ++r) sum += all[(int64_t)r * words + i];
    out[i] = sum;
}

// grid: ceil(n / kSparseThreads), n = nb * k.  packed: [2][n]
__global__ __launch_bounds__(kSparseThreads) void k_sparse_final_packed(const uint64_t* __restrict__ best_key,
                                                                        const int32_t* __restrict__ best_doc, int64_t n,
                                                                        int64_t row_offset, int64_t* __restrict__ packed) {
    const int64_t i = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t r = best_doc[i];
    const bool has = r != kRowNone;
    packed[i] = has ? __double_as_longlong(key_to_dist(best_key[i])) : kSparseNaNBits;
    packed[n + i] = has ? (int64_t)r + row_offset : -1;
}

// grid: ceil(n / kSparseThreads).  all: [world][n] distances as their bit patterns; at most one rank owns a document, so the
// lowest rank whose value is not NaN is the owner
__global__ __launch_bounds__(kSparseThreads) void k_sparse_fold_scores(const int64_t* __restrict__ all, int64_t n, int world,
                                                                       int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
    if (i >= n) return;
    int64_t v = kSparseNaNBits;
    for (int r = 0; r < world; ++r) {
        const int64_t x = all[(int64_t)r * n + i];
        if ((x & 0x7FFFFFFFFFFFFFFFll) <= 0x7FF0000000000000ll) {  // not a NaN
            v = x;
            break;
        }
    }
    out[i] = v;
}

}  // namespace mi355
