// k_combine.h -- search by examples / Rocchio feedback: the two kernels around the ordinary pass.
//   k_combine_rows     per slot: the listed positives and negatives made local, tested (shard, removed-row mark, stored norm
//                      finite and > 0) and scaled once, then every coordinate's IEEE-double chain in LIST order:
//                        acc = alpha * (s(q) * q_i);  acc = acc + cp * (s_j * c_ji) ...;  acc = acc - cn * (s_j * c_ji) ...
//                      rounded to fp32 once.  No value ever crosses a lane: a thread owns its coordinates from first to last
//                      example, so the order of every chain is the rule's (include/mi355dr.h "search by examples / feedback").
//                      The feedback form reads the positives from a search's own lists: entries with row >= 0 and a non-NaN
//                      distance (pos_dist != nullptr).
//   k_examples_strike  per slot: every entry of the inner pass's list whose row is listed in the slot is left out, the first k
//                      survivors written in list order with NaN / -1 behind; an invalid slot is blanked
// Plain HIP C++: vector loads and stores, one atomicAdd per skipped position or slot.  Input and output are different buffers.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kCombineThreads = 256;
constexpr int kCombineMaxExamples = 1024;  // positives + negatives of one slot (LDS: a double and an int32 each)

// one coordinate's chain, from the base term to the last negative (contraction off: one rounding per operation)
__device__ __forceinline__ double combine_term(double scale, float c) {
#pragma clang fp contract(off)
    return scale * (double)c;
}

// grid: one workgroup per slot.  queries: [nb, d] the base vectors or nullptr; pos_ids: [nb, mp], neg_ids: [nb, mn] GLOBAL
// rows; pos_dist: nullptr, or [nb, mp] the distances of the search whose rows pos_ids are; q_out: [nb, d]; valid: [nb];
// counters: [0] skipped example positions, [1] invalid slots.  mp + mn <= kCombineMaxExamples (the host checks)
__global__ __launch_bounds__(kCombineThreads) void k_combine_rows(
    const float* __restrict__ queries, const int64_t* __restrict__ pos_ids, int mp, const int64_t* __restrict__ neg_ids, int mn,
    const double* __restrict__ pos_dist, int64_t row_offset, int64_t n_rows, const float* __restrict__ rows,
    const float* __restrict__ nrm2, int d, int metric, double alpha, double beta, double gamma, float* __restrict__ q_out,
    int* __restrict__ valid, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
    __shared__ double s_scale[kCombineMaxExamples];
    __shared__ int32_t s_row[kCombineMaxExamples];  // local row, -1: the position is skipped
    __shared__ int s_cnt[2][kCombineThreads];
    __shared__ double s_base_scale;
    __shared__ int s_base_ok;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = mp + mn;
    const float* q = queries ? queries + (int64_t)b * d : nullptr;
    // ---- phase 1: the examples, once
    int my_pos = 0, my_neg = 0;
    for (int j = tid; j < m; j += kCombineThreads) {
        const bool is_pos = j < mp;
        const int64_t id = is_pos ? pos_ids[(int64_t)b * mp + j] : neg_ids[(int64_t)b * mn + (j - mp)];
        bool listed = true;  // (the feedback form: a list's padding and its NaN entries are no positives at all)
        if (pos_dist) {
            const double dj = pos_dist[(int64_t)b * mp + j];
            listed = id >= 0 && dj == dj;
        }
        // the shard test of subset_local_row (subset_ids.h): no signed overflow whatever the id
        const uint64_t local = (uint64_t)id - (uint64_t)row_offset;
        const int64_t r = listed && id >= row_offset && local < (uint64_t)n_rows ? (int64_t)local : -1;
        bool ok = r >= 0;
        float n2 = 0.0f;
        if (ok) {
            n2 = nrm2[r];
            ok = !row_is_dead(n2) && n2 > 0.0f && n2 < __builtin_inff();  // (NaN fails both compares)
        }
        s_row[j] = ok ? (int32_t)r : -1;
        s_scale[j] = ok ? (metric == 0 ? 1.0 / sqrt((double)n2) : 1.0) : 0.0;
        if (ok) {
            if (is_pos) ++my_pos;
            else ++my_neg;
        } else if (listed) {
            atomicAdd(&counters[0], 1ull);
        }
    }
    s_cnt[0][tid] = my_pos;
    s_cnt[1][tid] = my_neg;
    if (tid == 0) {
        // the base vector's squared norm: the k-ascending fp32 chain of k_row_nrm2, on one lane
        float acc = 0.0f;
        if (q)
            for (int c = 0; c < d; ++c) acc = __builtin_fmaf(q[c], q[c], acc);
        const bool ok = q && acc > 0.0f && acc < __builtin_inff();
        s_base_ok = ok ? 1 : 0;
        s_base_scale = ok ? (metric == 0 ? 1.0 / sqrt((double)acc) : 1.0) : 0.0;
    }
    __syncthreads();
    for (int w = kCombineThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_cnt[0][tid] += s_cnt[0][tid + w];
            s_cnt[1][tid] += s_cnt[1][tid + w];
        }
        __syncthreads();
    }
    const int n_pos = s_cnt[0][0], n_neg = s_cnt[1][0];
    const bool has_base = q != nullptr;
    const bool slot_ok = has_base ? s_base_ok != 0 : (n_pos > 0 || n_neg > 0);  // block-uniform
    float* dst = q_out + (int64_t)b * d;
    if (tid == 0) {
        valid[b] = slot_ok ? 1 : 0;
        if (!slot_ok) atomicAdd(&counters[1], 1ull);
    }
    if (!slot_ok) {
        for (int c = tid; c < d; c += kCombineThreads) dst[c] = 0.0f;
        return;
    }
    // ---- phase 2: every coordinate's chain, the examples walked in list order
    const double base_w = s_base_scale;
    const double cp = n_pos > 0 ? beta / (double)n_pos : 0.0;
    const double cn = n_neg > 0 ? gamma / (double)n_neg : 0.0;
    if (d % 4 == 0) {  // (rows and the query buffers are 256-B aligned allocations: 16-B aligned rows)
        for (int c = tid; c < d / 4; c += kCombineThreads) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            if (has_base) {
                const float4 v = ((const float4*)q)[c];
                a0 = alpha * combine_term(base_w, v.x);
                a1 = alpha * combine_term(base_w, v.y);
                a2 = alpha * combine_term(base_w, v.z);
                a3 = alpha * combine_term(base_w, v.w);
            }
            for (int j = 0; j < mp; ++j) {
                const int32_t r = s_row[j];
                if (r < 0) continue;  // block-uniform
                const double s = s_scale[j];
                const float4 v = ((const float4*)(rows + (int64_t)r * d))[c];
                a0 = a0 + cp * combine_term(s, v.x);
                a1 = a1 + cp * combine_term(s, v.y);
                a2 = a2 + cp * combine_term(s, v.z);
                a3 = a3 + cp * combine_term(s, v.w);
            }
            for (int j = mp; j < m; ++j) {
                const int32_t r = s_row[j];
                if (r < 0) continue;
                const double s = s_scale[j];
                const float4 v = ((const float4*)(rows + (int64_t)r * d))[c];
                a0 = a0 - cn * combine_term(s, v.x);
                a1 = a1 - cn * combine_term(s, v.y);
                a2 = a2 - cn * combine_term(s, v.z);
                a3 = a3 - cn * combine_term(s, v.w);
            }
            ((float4*)dst)[c] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
        }
    } else {
        for (int c = tid; c < d; c += kCombineThreads) {
            double a = has_base ? alpha * combine_term(base_w, q[c]) : 0.0;
            for (int j = 0; j < mp; ++j) {
                const int32_t r = s_row[j];
                if (r < 0) continue;
                a = a + cp * combine_term(s_scale[j], rows[(int64_t)r * d + c]);
            }
            for (int j = mp; j < m; ++j) {
                const int32_t r = s_row[j];
                if (r < 0) continue;
                a = a - cn * combine_term(s_scale[j], rows[(int64_t)r * d + c]);
            }
            dst[c] = (float)a;
        }
    }
}

// grid: one workgroup per slot.  cand_dist / cand_rows: [nb, stride] the inner pass's lists (global rows, total order), stride
// <= 1024; pos_ids: [nb, mp] / neg_ids: [nb, mn] the slot's listed ids (strike == 0: not read); valid: [nb] (blank_all != 0:
// not read, every slot is blanked -- an empty index); out_dist / out_rows: [nb, k], k <= stride
__global__ __launch_bounds__(kCombineThreads) void k_examples_strike(
    const double* __restrict__ cand_dist, const int64_t* __restrict__ cand_rows, int stride, const int64_t* __restrict__ pos_ids,
    int mp, const int64_t* __restrict__ neg_ids, int mn, int strike, const int* __restrict__ valid, int blank_all, int k,
    double* __restrict__ out_dist, int64_t* __restrict__ out_rows) {
    __shared__ int64_t s_ids[kCombineMaxExamples];
    __shared__ int s_scan[kCombineThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    double* od = out_dist + (int64_t)b * k;
    int64_t* orow = out_rows + (int64_t)b * k;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (blank_all || !valid[b]) {  // block-uniform
        for (int j = tid; j < k; j += kCombineThreads) {
            od[j] = nan;
            orow[j] = -1;
        }
        return;
    }
    const int m = strike ? mp + mn : 0;
    for (int j = tid; j < m; j += kCombineThreads)
        s_ids[j] = j < mp ? pos_ids[(int64_t)b * mp + j] : neg_ids[(int64_t)b * mn + (j - mp)];
    __syncthreads();
    const double* cd = cand_dist + (int64_t)b * stride;
    const int64_t* cr = cand_rows + (int64_t)b * stride;
    // a thread owns `per` consecutive entries (<= 4), so ranks follow list order
    const int per = (stride + kCombineThreads - 1) / kCombineThreads;
    const int j0 = tid * per, j1 = min(stride, j0 + per);
    unsigned keep = 0;  // bit i: entry j0 + i stays
    int kept = 0;
    for (int j = j0; j < j1; ++j) {
        const int64_t row = cr[j];
        bool hit = false;
        for (int e = 0; e < m; ++e) hit |= s_ids[e] == row;
        if (!hit) {
            keep |= 1u << (j - j0);
            ++kept;
        }
    }
    // inclusive prefix count over the workgroup (Hillis-Steele in LDS)
    s_scan[tid] = kept;
    __syncthreads();
    for (int w = 1; w < kCombineThreads; w <<= 1) {
        const int add = tid >= w ? s_scan[tid - w] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const int total = s_scan[kCombineThreads - 1];
    int rank = s_scan[tid] - kept;
    for (int j = j0; j < j1; ++j) {
        if (!(keep >> (j - j0) & 1u)) continue;
        if (rank < k) {
            od[rank] = cd[j];
            orow[rank] = cr[j];
        }
        ++rank;
    }
    for (int j = total + tid; j < k; j += kCombineThreads) {
        od[j] = nan;
        orow[j] = -1;
    }
}

}  // namespace mi355
