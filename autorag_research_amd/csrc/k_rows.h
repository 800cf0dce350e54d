// k_rows.h -- search by stored row: the two kernels around the ordinary pass and the range pass.
//   k_rows_gather   per slot: the caller's global id checked against the shard and the removed-row mark, the row's fp32
//                   vector copied into the query buffer (an invalid slot: a zero vector, valid = 0, counted), and the slot's
//                   (query, row) pair for k_rescore_pairs (the range form's row-with-itself distance)
//   k_rows_drop     per slot: the row itself found in the inner pass's list and left out -- out[j] = cand[j + (j >= p)] --,
//                   an invalid slot blanked to NaN / -1 and count 0; the range form also takes the row itself off the count
//                   when its own distance is in range
// Plain HIP C++: vector loads and stores, one atomicAdd per invalid slot.  Input and output are different buffers.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kRowsThreads = 256;

// grid: one workgroup per slot.  ids: [nb] GLOBAL rows; q_out: [nb, d]; valid: [nb]; pair_q / pair_row: [nb] (an invalid slot
// names row 0: the pair is scored and never read); skipped: one counter
__global__ __launch_bounds__(kRowsThreads) void k_rows_gather(const int64_t* __restrict__ ids, int64_t row_offset, int64_t n_rows,
                                                               const float* __restrict__ rows, const float* __restrict__ nrm2,
                                                               int d, float* __restrict__ q_out, int* __restrict__ valid,
                                                               int32_t* __restrict__ pair_q, int64_t* __restrict__ pair_row,
                                                               unsigned long long* __restrict__ skipped) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t id = ids[b];
    // the shard test of subset_local_row (subset_ids.h): no signed overflow whatever the id
    const uint64_t local = (uint64_t)id - (uint64_t)row_offset;
    const int64_t r = id >= row_offset && local < (uint64_t)n_rows ? (int64_t)local : -1;
    bool ok = r >= 0;  // block-uniform
    if (ok) ok = !row_is_dead(nrm2[r]);
    float* dst = q_out + (int64_t)b * d;
    if (ok) {
        const float* src = rows + r * (int64_t)d;
        if (d % 4 == 0) {  // (rows and the query buffer are 256-B aligned allocations: 16-B aligned rows)
            const float4* s4 = (const float4*)src;
            float4* d4 = (float4*)dst;
            for (int c = tid; c < d / 4; c += kRowsThreads) d4[c] = s4[c];
        } else {
            for (int c = tid; c < d; c += kRowsThreads) dst[c] = src[c];
        }
    } else {
        for (int c = tid; c < d; c += kRowsThreads) dst[c] = 0.0f;
    }
    if (tid == 0) {
        valid[b] = ok ? 1 : 0;
        pair_q[b] = b;
        pair_row[b] = ok ? r : 0;
        if (!ok) atomicAdd(skipped, 1ull);
    }
}

// grid: one workgroup per slot.  cand_dist / cand_rows: [nb, stride] the inner pass's lists (global rows, total order), stride
// = k + 1 (k with include_self); out_dist / out_rows: [nb, k].  Range form (cand_count != nullptr): cand_count [nb] the inner
// pass's exact counts, self_dist [nb] the row-with-itself distances, radius [nb], out_count [nb].
__global__ __launch_bounds__(kRowsThreads) void k_rows_drop(const double* __restrict__ cand_dist,
                                                             const int64_t* __restrict__ cand_rows, int stride,
                                                             const int64_t* __restrict__ ids, const int* __restrict__ valid, int k,
                                                             int include_self, const int64_t* __restrict__ cand_count,
                                                             const double* __restrict__ self_dist,
                                                             const double* __restrict__ radius, double* __restrict__ out_dist,
                                                             int64_t* __restrict__ out_rows, int64_t* __restrict__ out_count) {
    __shared__ int s_min[kRowsThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    double* od = out_dist + (int64_t)b * k;
    int64_t* orow = out_rows + (int64_t)b * k;
    if (!valid[b]) {  // block-uniform
        for (int j = tid; j < k; j += kRowsThreads) {
            od[j] = __longlong_as_double(0x7FF8000000000000ll);
            orow[j] = -1;
        }
        if (tid == 0 && cand_count) out_count[b] = 0;
        return;
    }
    const double* cd = cand_dist + (int64_t)b * stride;
    const int64_t* cr = cand_rows + (int64_t)b * stride;
    // position of the row itself in the list (it is there at most once); stride: not there, the list is cut to k
    int p = stride;
    if (!include_self) {
        const int64_t self = ids[b];
        for (int j = tid; j < stride; j += kRowsThreads)
            if (cr[j] == self) p = min(p, j);
        s_min[tid] = p;
        __syncthreads();
        for (int w = kRowsThreads / 2; w > 0; w >>= 1) {
            if (tid < w) s_min[tid] = min(s_min[tid], s_min[tid + w]);
            __syncthreads();
        }
        p = s_min[0];
    }
    for (int j = tid; j < k; j += kRowsThreads) {
        const int from = j + (j >= p ? 1 : 0);  // (< stride: p < stride only where stride = k + 1)
        od[j] = cd[from];
        orow[j] = cr[from];
    }
    if (tid == 0 && cand_count) {
        // in range: not NaN and <= radius, as doubles (decided from the distance, not from the truncated list)
        const bool self_in = !include_self && self_dist[b] <= radius[b];
        out_count[b] = cand_count[b] - (self_in ? 1 : 0);
    }
}

}  // namespace mi355
