// k_range.h -- range search: every row within a distance, counted and listed on the device.
//   k_range_prep     per query: the radius as an order key, the exact path's fixed threshold (thr_key, thr_row) and -- for a
//                    query that screens -- the fixed screen threshold the radius allows (screen_threshold, k_select.h)
//   k_range_collect  per query, after a chunk: the chunk's candidates become (key, row) entries of the query's result buffer
//                    and are counted.  Screen form: every candidate is re-scored by the exact chain first (staged_dot, the
//                    re-score device code of k_prune) and kept iff its key is within the radius.  Exact form: the candidates
//                    come from k_scan / k_scan32 and are all within the radius by the scan's own test.  A list that
//                    overflowed is not committed: the (query, chunk) pair is recorded for the host, which runs it again on
//                    the exact path.
//   k_range_finish   per query: the buffer sorted by the total order (key asc, row asc), its first max_results entries and
//                    the count written out; a query with more rows in range than the buffer holds is flagged instead.
// Plain HIP C++: vector stores, atomicAdd, the LDS bitonic sort of dev_common.h.  No workgroup waits for another one.
#pragma once
#include "dev_common.h"
#include "k_select.h"

namespace mi355 {

constexpr int kRangeThreads = 256;
constexpr int32_t kRangeScreens = 0x7FFFFFFF;  // RangeState::xfrom of a query whose chunks are screened

// device arrays the index owns, one slot per query of the block (mi355dr.hip: ensure_range)
struct RangeState {
    uint64_t* key;              // [B, R] result buffer: exact keys ...
    int32_t* row;               // [B, R] ... and local rows, in arrival order
    unsigned long long* count;  // [B] rows in range so far (slots used = min(count, R))
    uint64_t* rkey;             // [B] dist_to_key(radius)
    int32_t* xfrom;             // [B] rows from this one on are served by the exact path; kRangeScreens: none
    // [0]: pairs recorded, [1]: pairs that found the list full (the host then fails the call), then the pairs: (query,
    // 2 * span + came_from_the_exact_form)
    int* redo;
    int redo_cap;               // pairs the list holds
    unsigned long long* stat;   // [2] candidates taken from the screens, of them re-scored
    int* flag;                  // [B] k_range_finish: more than R rows are in range
    int R;
};

__device__ __forceinline__ void range_record(const RangeState& rs, int q, int code) {
    const int i = atomicAdd(&rs.redo[0], 1);
    if (i < rs.redo_cap) {
        rs.redo[2 + 2 * i] = q;
        rs.redo[3 + 2 * i] = code;
    } else {
        atomicAdd(&rs.redo[1], 1);
    }
}

// grid: ceil(B / 256) blocks of 256 threads, behind k_prep_queries.  screen != 0: regular queries get the threshold their
// radius allows -- the function the prunes publish thresholds with, so no row at or below the radius is lost; a threshold
// that admits every row (-inf; below -1 under cosine) or is no number sends the query to the exact path at once, and so does
// an irregular query (parked at +inf by k_prep_queries).  One so high that no stored row reaches it is parked at +inf.
__global__ __launch_bounds__(kRangeThreads) void k_range_prep(const double* __restrict__ radius, int B, int metric, int screen,
                                                               QueryState st, RangeState rs) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    // (distances are compared as doubles, where -0.0 == +0.0; the order keys tell them apart: a zero radius is +0.0)
    const double r = radius[b] == 0.0 ? 0.0 : radius[b];
    const uint64_t rk = dist_to_key(r);
    rs.rkey[b] = rk;
    rs.count[b] = 0ull;
    rs.flag[b] = 0;
    st.thr_key[b] = rk;  // k_scan appends iff key < rk || (key == rk && row < INT32_MAX): distance <= radius, NaN excluded
    st.thr_row[b] = 0x7FFFFFFF;
    int32_t xfrom = 0;
    float thr = __builtin_inff();
    if (screen && !(st.status[b] & kStIrregular)) {
        float t = screen_threshold(metric, r, st.E[b], st.qn[b]);
        if (t > -__builtin_inff() && (metric != 0 || t >= -1.0f)) {  // (NaN compares false)
            if (t > 1e30f) t = __builtin_inff();  // (regular rows have |c| <= 1e15: none reaches it)
            thr = t;
            xfrom = kRangeScreens;
        }
    }
    st.thr[b] = thr;
    rs.xfrom[b] = xfrom;
}

// dynamic LDS: one stage tile per wave | qs[d] | two counters
__host__ __device__ inline size_t range_collect_lds(int d) {
    return (size_t)(kRangeThreads / kWave) * kStageFloats * sizeof(float) + prune_qs_floats(d) * sizeof(float);
}

enum { kRangeFormScreen = 0, kRangeFormSide = 1, kRangeFormExact = 2 };

struct RangeCollectArgs {
    const float* rows;     // [n, d]
    const float* nrm2;     // [n]
    const float* q;        // [B, d]
    QueryState st;
    RangeState rs;
    const int32_t* cand_row;  // [Bpad, cap]
    const float* cand_val;    // screen / side form: the screen value (NaN: no bound); exact form: the fp32 dot
    const int* qlist;         // exact form: the launch's queries (else nullptr: blockIdx.x)
    const uint8_t* flag8;     // int8 screen: rows outside the int8 shadow (their finite screen values are stale zeros)
    int cap, d, metric, form;
    int span;                 // what an overflow is recorded under
    int64_t row0;             // screen form: first row of the chunk
    int64_t n_rows;           // rows of the index (candidate rows are checked against it)
};

// grid: one workgroup per query (exact form: per listed query)
__global__ __launch_bounds__(kRangeThreads) void k_range_collect(RangeCollectArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tiles = (float*)smem;
    float* qs = tiles + (kRangeThreads / kWave) * kStageFloats;
    int* s_ctr = (int*)(qs + prune_qs_floats(a.d) - 16);  // [0]: appended, [1]: re-scored
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = a.qlist ? a.qlist[blockIdx.x] : blockIdx.x;
    // thread 0 reads the words it rewrites below and hands them round through LDS: the branches that follow are block-uniform
    if (tid == 0) {
        s_ctr[0] = s_ctr[1] = 0;
        s_ctr[2] = a.st.cnt[q];
        s_ctr[3] = a.rs.xfrom[q];
        s_ctr[4] = a.st.status[q];
        *(unsigned long long*)(s_ctr + 6) = a.rs.count[q];
    }
    __syncthreads();
    const int cnt = s_ctr[2];
    const int32_t xfrom = s_ctr[3];
    const int status = s_ctr[4];
    const unsigned long long base = *(const unsigned long long*)(s_ctr + 6);
    const int R = a.rs.R;
    if (a.form == kRangeFormScreen) {
        const bool over = cnt > a.cap || (status & kStOverflow);
        if (xfrom != kRangeScreens || over) {
            // served by the exact path from here on: nothing of this chunk is committed, the host runs it again exactly
            if (tid == 0) {
                range_record(a.rs, q, 2 * a.span);
                if (xfrom == kRangeScreens) {
                    a.rs.xfrom[q] = (int32_t)a.row0;
                    a.st.thr[q] = __builtin_inff();  // (later chunks' screens emit nothing for it)
                }
                a.st.cnt[q] = 0;
                a.st.status[q] &= ~kStOverflow;
            }
            return;
        }
    } else if (a.form == kRangeFormExact && cnt > a.cap) {
        // the scan counted every in-range row of the piece although the list kept only its first `cap`: when that count
        // already puts the query beyond the buffer its entries no longer matter (k_range_finish flags it); else the piece is
        // run again in list-sized pieces
        if (tid == 0) {
            if (base + (unsigned long long)cnt > (unsigned long long)R) a.rs.count[q] = base + (unsigned long long)cnt;
            else range_record(a.rs, q, 2 * a.span + 1);
            a.st.cnt[q] = 0;
        }
        return;
    }
    if (cnt <= 0) return;
    const int n = min(cnt, a.cap);
    const int32_t* crow = a.cand_row + (int64_t)q * a.cap;
    const float* cval = a.cand_val + (int64_t)q * a.cap;
    const uint64_t rk = a.rs.rkey[q];
    const float nq = a.st.qn[q];
    uint64_t* okey = a.rs.key + (int64_t)q * R;
    int32_t* orow = a.rs.row + (int64_t)q * R;
    auto append = [&](uint64_t key, int32_t row) {
        const unsigned long long slot = base + (unsigned long long)atomicAdd(&s_ctr[0], 1);  // (LDS)
        if (slot < (unsigned long long)R) {
            okey[slot] = key;
            orow[slot] = row;
        }
    };
    if (a.form == kRangeFormExact) {
        for (int e = tid; e < n; e += kRangeThreads) {
            int32_t row = crow[e];
            if (row < 0 || row >= a.n_rows) continue;
            const uint64_t key = exact_key_of(a.metric, cval[e], nq, a.nrm2[row], row);
            if (key <= rk && key != kKeyNaN) append(key, row);
        }
    } else {
        for (int k = tid; k < a.d; k += kRangeThreads) qs[k] = a.q[(int64_t)q * a.d + k];
        __syncthreads();
        float* tile = tiles + wave * kStageFloats;
        for (int b0 = 0; b0 < n; b0 += kRangeThreads) {
            const int e = b0 + tid;
            bool live = e < n;
            const int32_t row = live ? crow[e] : 0;
            const float v = live ? cval[e] : 0.0f;
            if (live && (row < 0 || row >= a.n_rows)) live = false;
            // side rows at or behind xfrom are rows of the chunks the exact path serves for this query
            if (live && a.form == kRangeFormSide && row >= xfrom) live = false;
            // a finite value on a row outside the int8 shadow is a stale zero: that row comes through the side list (NaN)
            if (live && a.flag8 != nullptr && v == v && a.flag8[row]) live = false;
            const float* rp = live ? a.rows + (int64_t)row * a.d : nullptr;
            float acc = 0.0f;
            if (b0 + wave * kWave < n) acc = staged_dot(tile, rp, qs, a.d, lane);  // wave-uniform condition
            if (live) {
                int32_t kept = row;  // (a dead row: the padding entry, never within a radius)
                const uint64_t key = exact_key_of(a.metric, acc, nq, a.nrm2[row], kept);
                atomicAdd(&s_ctr[1], 1);
                if (key <= rk && key != kKeyNaN) append(key, kept);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.rs.count[q] = base + (unsigned long long)s_ctr[0];
        a.st.cnt[q] = 0;
        if (a.form != kRangeFormExact) {
            atomicAdd(&a.rs.stat[0], (unsigned long long)n);
            atomicAdd(&a.rs.stat[1], (unsigned long long)s_ctr[1]);
        }
    }
}

// key[np] | row[np]
__host__ __device__ inline size_t range_finish_lds(int np) { return (size_t)np * (sizeof(uint64_t) + sizeof(int32_t)); }

// grid: B blocks of 256 threads; np_max: the power of two >= R the launch's LDS was sized for.  row_map (a view) names the
// global id of every stored row; else it is row + row_offset.
__global__ __launch_bounds__(kRangeThreads) void k_range_finish(RangeState rs, int np_max, int max_results, int64_t row_offset,
                                                                 const int64_t* __restrict__ row_map, double* __restrict__ out_dist,
                                                                 int64_t* __restrict__ out_rows, int64_t* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* SK = (uint64_t*)smem;
    int32_t* SR = (int32_t*)(smem + (size_t)np_max * sizeof(uint64_t));
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned long long c = rs.count[q];
    double* od = out_dist + (int64_t)q * max_results;
    int64_t* orow = out_rows + (int64_t)q * max_results;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (tid == 0) out_count[q] = (int64_t)c;
    if (c > (unsigned long long)rs.R) {  // (block-uniform) the host serves the list by the ordinary search; the count stands
        for (int t = tid; t < max_results; t += kRangeThreads) {
            od[t] = nan;
            orow[t] = -1;
        }
        if (tid == 0) rs.flag[q] = 1;
        return;
    }
    const int n = (int)c, np = next_pow2(max(n, 1));  // np <= np_max: n <= R <= np_max
    for (int i = tid; i < np; i += kRangeThreads) {
        SK[i] = i < n ? rs.key[(int64_t)q * rs.R + i] : kKeyNaN;
        SR[i] = i < n ? rs.row[(int64_t)q * rs.R + i] : kRowNone;
    }
    __syncthreads();
    bitonic_asc_key_row(SK, SR, np);
    for (int t = tid; t < max_results; t += kRangeThreads) {
        if (t < n) {
            od[t] = key_to_dist(SK[t]);
            orow[t] = row_map ? row_map[SR[t]] : (int64_t)SR[t] + row_offset;
        } else {
            od[t] = nan;
            orow[t] = -1;
        }
    }
}

}  // namespace mi355
