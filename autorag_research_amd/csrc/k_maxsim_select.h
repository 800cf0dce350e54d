// k_maxsim_select.h -- selection kernels of the MaxSim search (host side: mi355dr_maxsim.hip).
//   k_topk_segments    segment-wise exact top-k by (distance, doc): full scans, and the path of k > kMsFastK
//   k_ms_candidates    candidates of one query (k > kMsFastK)
//   k_ms_select, k_ms_candidates_y, k_ms_tighten, k_ms_final    the fast path: every query of a pass at once (grid.y)
//   k_ms_membership    a listed subset as the table the kernels above take in place of blk_off
//   k_ms_write_out, k_ms_fill_empty    results to the caller's layout
#pragma once
#include "maxsim_common.h"

namespace mi355 {

// fp32 -> sortable key (distance asc, NaN last)
__device__ __forceinline__ uint64_t f32_to_key(float f) {
    if (f != f) return kKeyNaN;
    uint32_t b = __float_as_uint(f);
    b = (b >> 31) ? ~b : (b | 0x80000000u);
    return (uint64_t)b;
}
__device__ __forceinline__ float key_to_f32(uint64_t k) {
    if (k == kKeyNaN) return __uint_as_float(0x7FC00000u);
    uint32_t b = (uint32_t)k;
    b = (b >> 31) ? (b & 0x7FFFFFFFu) : ~b;
    return __uint_as_float(b);
}

// one workgroup per segment of kSegSort entries: sort by (key,row), write the first k.
// first stage reads distances (and skips empty docs), later stages read (key,row) partials.
// row_map / n_in_dev (first stage only): entry g is doc row_map[g], and only the first *n_in_dev entries exist.
__global__ __launch_bounds__(256) void k_topk_segments(const float* dist, const int64_t* blk_off,
                                                        const uint64_t* key_in, const int32_t* row_in, int64_t n_in,
                                                        int k, int seg, uint64_t* key_out, int32_t* row_out,
                                                        const int32_t* row_map, const int* n_in_dev) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* SK = (uint64_t*)smem;
    int32_t* SR = (int32_t*)(smem + (size_t)kSegSort * 8);
    const int64_t base = (int64_t)blockIdx.x * seg;
    if (dist && n_in_dev) n_in = min(n_in, (int64_t)*n_in_dev);
    for (int i = threadIdx.x; i < seg; i += blockDim.x) {
        const int64_t g = base + i;
        uint64_t key = kKeyNaN;
        int32_t row = 0x7FFFFFFF;
        if (g < n_in) {
            if (dist) {
                const int64_t doc = row_map ? (int64_t)row_map[g] : g;
                if (blk_off[doc + 1] > blk_off[doc]) {  // docs without vectors are not rows of the result
                    key = f32_to_key(dist[g]);
                    row = (int32_t)doc;
                }
            } else {
                key = key_in[g];
                row = row_in[g];
            }
        }
        SK[i] = key;
        SR[i] = row;
    }
    __syncthreads();
    bitonic_asc_key_row(SK, SR, seg);
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        key_out[(int64_t)blockIdx.x * k + i] = SK[i];
        row_out[(int64_t)blockIdx.x * k + i] = SR[i];
    }
}

// candidates of one query: every doc whose screen distance is within 2E of the k-th best screen distance
// (kth_key = last entry of the screen's top-k; NaN key = fewer than k docs with vectors -> every doc is a candidate)
__global__ void k_ms_candidates(const float* dist16, const int64_t* blk_off, int64_t n_docs, const uint64_t* topk_keys, int k,
                                float two_e, int32_t* list, int cap, int* ctl) {
    const int64_t doc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (doc >= n_docs || blk_off[doc + 1] <= blk_off[doc]) return;
    const uint64_t kth = topk_keys[k - 1];
    float thr = __builtin_inff();
    if (kth != kKeyNaN) {
        thr = key_to_f32(kth) + two_e;
        thr += fabsf(thr) * 1.2e-7f + 1e-30f;  // round the sum up
    }
    if (!(dist16[doc] > thr)) {  // (a NaN screen value stays a candidate)
        const int slot = atomicAdd(&ctl[0], 1);
        if (slot < cap) list[slot] = (int32_t)doc;
        else ctl[1] = 1;
    }
}

// ---- fast selection path of the screened search (k <= kMsFastK): all queries of a launch at once (grid.y) ----
constexpr int kMsFastK = 64;
constexpr int kMsSelSeg = kWave * kSelPerLane;  // 1024 entries per wave

// One wave per segment of 1024 entries: the k smallest distances of the segment, as order keys (unsorted, padded
// with 0xFFFFFFFF).  First stage reads screen distances (docs without vectors / NaN rank last), later stages keys.
// Only VALUES travel: the stages exist to find the k-th best screen distance.
__global__ __launch_bounds__(kWave) void k_ms_select(const float* dist, const int64_t* blk_off, const uint32_t* key_in,
                                                     int64_t n_in, int64_t in_stride, int k, uint32_t* key_out,
                                                     int64_t out_stride) {
    const int lane = threadIdx.x, y = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * kMsSelSeg;
    uint32_t inv[kSelPerLane];  // inverted key: the smallest distance has the largest inv; 0 = absent
#pragma unroll
    for (int j = 0; j < kSelPerLane; ++j) {
        const int64_t g = base + j * kWave + lane;
        uint32_t key = 0xFFFFFFFFu;
        if (g < n_in) {
            if (dist) {
                const float v = dist[(int64_t)y * in_stride + g];
                if (blk_off[g + 1] > blk_off[g] && v == v) key = f32_order_key(v);
            } else {
                key = key_in[(int64_t)y * in_stride + g];
            }
        }
        inv[j] = ~key;
    }
    uint32_t* out = key_out + (int64_t)y * out_stride + (int64_t)blockIdx.x * k;
    for (int i = lane; i < k; i += kWave) out[i] = 0xFFFFFFFFu;
    const int n_valid = wave_count_ge(inv, 1u);
    const int kk = min(k, n_valid);
    if (kk == 0) return;
    const uint32_t x = wave_nth_largest(inv, kk);
    int n = 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {  // strictly better than the k-th first, then ties up to k
#pragma unroll
        for (int j = 0; j < kSelPerLane; ++j) {
            const bool want = pass == 0 ? inv[j] > x : inv[j] == x;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(want);
            const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
            if (want && pos < kk) out[pos] = ~inv[j];
            n += __builtin_popcountll(bal);
        }
    }
}

// candidates of every query of the launch (grid.y): docs whose screen distance is within 2E of the k-th best one -> the WIDE
// list (+ each entry's screen distance, when sd_out is given); the docs AT OR ABOVE the k-th best screen distance -> the STARTER
// list (when list_a is given): k_ms_tighten narrows the wide list with the starter's exact distances
constexpr int kMsCandPerThread = 4;  // a workgroup of 256 threads looks at 1024 docs
__global__ __launch_bounds__(256) void k_ms_candidates_y(const float* dist16, int64_t dist_stride, const int64_t* blk_off,
                                                          int64_t n_docs, const uint32_t* topk_keys, int64_t key_stride, int k,
                                                          const float* two_e, int32_t* list, int cap, int* ctl, float* sd_out,
                                                          int32_t* list_a, int* ctl_a) {
    __shared__ uint32_t kth_s;
    const int y = blockIdx.y;
    if (threadIdx.x < kWave) {  // k <= kMsFastK = 64: one key per lane of the first wave
        uint32_t key = threadIdx.x < k ? topk_keys[(int64_t)y * key_stride + threadIdx.x] : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, kWave));
        if (threadIdx.x == 0) kth_s = key;
    }
    __syncthreads();
    const uint32_t kth = kth_s;
    float thr = __builtin_inff();
    if (kth != 0xFFFFFFFFu) {
        const uint32_t ub = (kth & 0x80000000u) ? (kth & 0x7FFFFFFFu) : ~kth;
        thr = __uint_as_float(ub) + two_e[y];
        thr += fabsf(thr) * 1.2e-7f + 1e-30f;
    }
#pragma unroll
    for (int u = 0; u < kMsCandPerThread; ++u) {
        const int64_t doc = ((int64_t)blockIdx.x * kMsCandPerThread + u) * blockDim.x + threadIdx.x;
        if (doc >= n_docs || blk_off[doc + 1] <= blk_off[doc]) continue;
        const float v = dist16[(int64_t)y * dist_stride + doc];
        if (!(v > thr)) {
            const int slot = atomicAdd(&ctl[2 * y], 1);
            if (slot < cap) {
                list[(int64_t)y * cap + slot] = (int32_t)doc;
                if (sd_out) sd_out[(int64_t)y * cap + slot] = v;
            } else {
                ctl[2 * y + 1] = 1;
            }
            if (list_a && v == v && f32_order_key(v) <= kth) {  // (the select ranks exactly these keys)
                const int sa = atomicAdd(&ctl_a[2 * y], 1);
                if (sa < cap) list_a[(int64_t)y * cap + sa] = (int32_t)doc;
                else ctl_a[2 * y + 1] = 1;
            }
        }
    }
}

// The wide list -> the final list (grid.y = query, one workgroup).  The starter docs (>= k of them: the screen's top-k and its
// ties) carry their EXACT distances: their k-th smallest, D, is an upper bound of the true k-th best exact distance, and a doc
// of the exact top-k (ties included) has exact <= D, hence screen <= exact + E <= D + E.  The wide list's threshold is
// x_k + 2E with x_k the k-th best SCREEN distance; D <= x_k + E always (every starter doc has exact <= screen + E), and
// D ~ x_k in practice: the band halves and the docs to re-score drop by ~6 x (the band sits in the tail of the score
// distribution).  The starter is part of the final list (screen <= x_k <= D + E).  Without a usable starter (fewer than k docs
// with vectors, a starter list beyond kMsTightenMax entries or overflown) the final list is the wide list.
constexpr int kMsTightenMax = 1024;
__global__ __launch_bounds__(256) void k_ms_tighten(const float* dist_a, const int* ctl_a, const int32_t* list_c, const float* sd_c,
                                                     const int* ctl_c, int cap, int k, const float* two_e, int32_t* list_b, int* ctl_b) {
    __shared__ uint32_t key_a[kMsTightenMax];
    __shared__ float thr_s;
    __shared__ int n_b;
    const int y = blockIdx.y, tid = threadIdx.x;
    const int n_c = min(ctl_c[2 * y], cap);
    if (ctl_c[2 * y + 1] != 0) {  // the wide list overflowed: the caller's exact full scan
        if (tid == 0) {
            ctl_b[2 * y] = 0;
            ctl_b[2 * y + 1] = 1;
        }
        return;
    }
    const int n_a = ctl_a[2 * y];
    const bool usable = ctl_a[2 * y + 1] == 0 && n_a >= k && n_a <= kMsTightenMax;  // workgroup-uniform
    if (tid == 0) {
        thr_s = __builtin_inff();
        n_b = 0;
    }
    if (usable) {
        for (int i = tid; i < n_a; i += blockDim.x) key_a[i] = f32_order_key(dist_a[(int64_t)y * cap + i]);
        __syncthreads();
        for (int i = tid; i < n_a; i += blockDim.x) {  // rank under the strict order (key, position): exactly one entry has rank k - 1
            const uint32_t ki = key_a[i];
            int rank = 0;
            for (int j = 0; j < n_a; ++j) rank += (key_a[j] < ki || (key_a[j] == ki && j < i)) ? 1 : 0;
            if (rank == k - 1) {
                const uint32_t ub = (ki & 0x80000000u) ? (ki & 0x7FFFFFFFu) : ~ki;
                // D + E rounded UP (two_e holds 2E rounded up); a NaN here keeps every entry (the comparison below)
                thr_s = __double2float_ru((double)__uint_as_float(ub) + 0.5 * (double)two_e[y]);
            }
        }
    }
    __syncthreads();
    const float thr = thr_s;
    for (int i = tid; i < n_c; i += blockDim.x) {
        if (!(sd_c[(int64_t)y * cap + i] > thr)) list_b[(int64_t)y * cap + atomicAdd(&n_b, 1)] = list_c[(int64_t)y * cap + i];
    }
    __syncthreads();
    if (tid == 0) {
        ctl_b[2 * y] = n_b;
        ctl_b[2 * y + 1] = 0;
    }
}

// exact top-k of one query's re-scored candidates (grid.y = query): sort by (distance, doc) in LDS, write the result.
// doc_map (a view: mi355dr_view_create) names the global id of every stored document; else it is doc + row_offset
__global__ __launch_bounds__(256) void k_ms_final(const float* cand_dist, const int32_t* cand_list, const int* ctl, int cap,
                                                   int k, int64_t row_offset, const int64_t* __restrict__ doc_map, float* out_d,
                                                   int64_t* out_r) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int y = blockIdx.y;
    const int n = min(ctl[2 * y], cap);
    const int np = next_pow2(max(n, 1));
    uint64_t* SK = (uint64_t*)smem;
    int32_t* SR = (int32_t*)(smem + (size_t)np * 8);
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        uint64_t key = kKeyNaN;
        int32_t row = 0x7FFFFFFF;
        if (i < n) {
            key = f32_to_key(cand_dist[(int64_t)y * cap + i]);
            row = cand_list[(int64_t)y * cap + i];
        }
        SK[i] = key;
        SR[i] = row;
    }
    __syncthreads();
    bitonic_asc_key_row(SK, SR, np);
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const bool ok = i < n && SR[i] != 0x7FFFFFFF;
        out_d[(int64_t)y * k + i] = ok ? key_to_f32(SK[i]) : __uint_as_float(0x7FC00000u);
        out_r[(int64_t)y * k + i] = !ok ? -1 : doc_map ? doc_map[SR[i]] : (int64_t)SR[i] + row_offset;
    }
}

// The membership table of a listed subset (mi355dr_search_maxsim_subset): T[d] = listed documents below d, d = 0 .. n_docs, by a
// lower bound in the sorted, unique list of documents with vectors.  T[d + 1] > T[d] holds exactly for the listed documents:
// k_topk_segments, k_ms_select and the two candidate kernels read T where they read blk_off ("this document has vectors"), and
// never look at the positions of the dense screen distances that the list screen did not write.
__global__ void k_ms_membership(const int32_t* __restrict__ list, int64_t n_list, int64_t n_docs, int64_t* __restrict__ T) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_docs) return;
    int64_t lo = 0, hi = n_list;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)list[mid] < d) lo = mid + 1;
        else hi = mid;
    }
    T[d] = lo;
}

__global__ void k_ms_write_out(const uint64_t* key, const int32_t* row, int k, int64_t row_offset,
                               const int64_t* __restrict__ doc_map, float* out_d, int64_t* out_r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const bool ok = row[i] != 0x7FFFFFFF;
    out_d[i] = ok ? key_to_f32(key[i]) : __uint_as_float(0x7FC00000u);
    out_r[i] = !ok ? -1 : doc_map ? doc_map[row[i]] : (int64_t)row[i] + row_offset;
}

}  // namespace mi355

namespace {

__global__ void k_ms_fill_empty(float* d, int64_t* r, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        d[i] = __uint_as_float(0x7FC00000u);
        r[i] = -1;
    }
}

}  // namespace
