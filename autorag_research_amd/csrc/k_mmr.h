// k_mmr.h -- Maximal Marginal Relevance over a candidate list, selected on the device.
//
// One workgroup of 4 waves per query walks the definition in include/mi355dr.h ("MMR search") literally: the candidates
// arrive in the library's total order (distance asc, NaN last, row asc), the eligible ones are the leading entries with a
// row and a non-NaN distance, pick 0 is candidate 0, and after every pick but the last the picked row is scored against
// every unselected candidate through staged_dot -- the k-ascending fp32 fmaf chain of dev_common.h, 64 rows per wave
// against the ONE LDS-resident vector -- with the stored norms of both rows and distance_from in double.  Everything
// else is IEEE double with separate operations (the unit is compiled with -ffp-contract=off).
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kMmrThreads = 256;
constexpr int kMmrWaves = kMmrThreads / kWave;
constexpr int kMmrMax = 1024;  // longest candidate list (fetch_k of mi355dr_search_mmr, m of mi355dr_mmr_select)
constexpr int kMmrNone = 0x7FFFFFFF;

// per-candidate arrays are sized by the list (rounded up to 4 entries so that every array stays 16-B aligned)
__host__ __device__ inline int mmr_cap(int stride) { return (stride + 3) & ~3; }
__host__ __device__ inline int mmr_dq(int d) { return (d + 3) & ~3; }
// tiles | qv | sq | ms | reduction scores | local rows | reduction positions, first-unselected, eligible count | flags
__host__ __device__ inline size_t mmr_lds_bytes(int d, int stride) {
    const size_t cap = (size_t)mmr_cap(stride);
    return (size_t)kMmrWaves * kStageFloats * sizeof(float) + (size_t)mmr_dq(d) * sizeof(float) + 2 * cap * sizeof(double) +
           kMmrWaves * sizeof(double) + cap * sizeof(int32_t) + (2 * kMmrWaves + 4) * sizeof(int) + cap;
}

// "higher is better" image of a distance, in double: 1 - distance for cosine, -distance for inner product
__device__ __forceinline__ double mmr_sim(int metric, double dist) { return metric == 0 ? 1.0 - dist : -dist; }

// Where the selection reads a candidate's fp32 vector and stored norm from.  locate(): is candidate i (global row r) a row the
// source holds, and under which locator (kept in LDS, one int32 per candidate); vec() / nrm(): its vector and |row|^2.
// This one: the index's own rows -- the locator is the local row.  k_shard.h has the other: the gathered stage of a row-sharded
// index.  Both run mmr_select_body, so argmax, tie rule, staged_dot and distance_from cannot drift apart.
struct MmrLocalRows {
    const float* rows;
    const float* nrm2;
    int64_t n_rows, row_offset;
    int d;
    __device__ __forceinline__ bool locate(int, int64_t r, int32_t* loc) const {
        if (r >= row_offset && r - row_offset < n_rows) {
            *loc = (int32_t)(r - row_offset);
            return true;
        }
        return false;
    }
    __device__ __forceinline__ const float* vec(int, int32_t loc) const { return rows + (int64_t)loc * d; }
    __device__ __forceinline__ float nrm(int, int32_t loc) const { return nrm2[loc]; }
};

// one workgroup of kMmrThreads per query.  crow / cdist: this query's [stride] list, GLOBAL rows (-1 = none); od / orow: its
// [k] picks.  pairs_scored: one counter, += the (picked, candidate) dots of this query.
template <class Src>
__device__ __forceinline__ void mmr_select_body(const Src& src, const int64_t* __restrict__ crow, const double* __restrict__ cdist,
                                                int stride, int d, int metric, int k, double lambda, double* __restrict__ od,
                                                int64_t* __restrict__ orow, unsigned long long* __restrict__ pairs_scored) {
    extern __shared__ __align__(16) unsigned char mmr_smem[];
    const int cap = mmr_cap(stride), dq = mmr_dq(d);
    float* tiles = (float*)mmr_smem;
    float* qv = tiles + kMmrWaves * kStageFloats;
    double* sq = (double*)(qv + dq);
    double* ms = sq + cap;
    double* red_s = ms + cap;
    int32_t* lrow = (int32_t*)(red_s + kMmrWaves);
    int* red_p = (int*)(lrow + cap);
    int* red_f = red_p + kMmrWaves;
    int* n_elig = red_f + kMmrWaves;  // (4 ints: the first one is used)
    unsigned char* sel = (unsigned char*)(n_elig + 4);

    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;

    // ---- the eligible prefix: a row the source holds and a distance that is a number
    if (tid == 0) n_elig[0] = stride;
    __syncthreads();
    for (int i = tid; i < stride; i += kMmrThreads) {
        const int64_t r = crow[i];
        const double dist = cdist[i];
        int32_t loc = 0;
        if (src.locate(i, r, &loc) && dist == dist) {
            lrow[i] = loc;
            sq[i] = mmr_sim(metric, dist);
            sel[i] = 0;
        } else {
            atomicMin(&n_elig[0], i);
        }
    }
    __syncthreads();
    const int n = n_elig[0], picks = min(k, n);  // (uniform: every loop bound below depends on n and k only)
    for (int t = picks + tid; t < k; t += kMmrThreads) {
        od[t] = __longlong_as_double(0x7FF8000000000000ll);
        orow[t] = -1;
    }
    if (picks == 0) return;
    const double one_m = 1.0 - lambda;
    const int rounds = (n + kMmrThreads - 1) / kMmrThreads;
    int cur = 0;  // pick 0 = candidate 0
    for (int t = 0; t < picks; ++t) {
        if (t > 0) {
            // ---- argmax of lambda * sq - (1 - lambda) * ms over the unselected: the lowest position wins a tie, a NaN score
            //      never wins, and without a winner the first unselected candidate is taken
            double bs = 0.0;
            int bp = kMmrNone, fp = kMmrNone;
            for (int i = tid; i < n; i += kMmrThreads) {
                if (sel[i]) continue;
                fp = min(fp, i);
                const double a = lambda * sq[i], b = one_m * ms[i];
                const double sc = a - b;
                if (sc == sc && (bp == kMmrNone || sc > bs)) {
                    bs = sc;
                    bp = i;
                }
            }
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const double os = __shfl_xor(bs, off, kWave);
                const int op = __shfl_xor(bp, off, kWave), of = __shfl_xor(fp, off, kWave);
                if (op != kMmrNone && (bp == kMmrNone || os > bs || (os == bs && op < bp))) {
                    bs = os;
                    bp = op;
                }
                fp = min(fp, of);
            }
            if (lane == 0) {
                red_s[w] = bs;
                red_p[w] = bp;
                red_f[w] = fp;
            }
            __syncthreads();
            bs = red_s[0];
            bp = red_p[0];
            fp = red_f[0];
            for (int j = 1; j < kMmrWaves; ++j) {
                const double os = red_s[j];
                const int op = red_p[j];
                if (op != kMmrNone && (bp == kMmrNone || os > bs || (os == bs && op < bp))) {
                    bs = os;
                    bp = op;
                }
                fp = min(fp, red_f[j]);
            }
            cur = bp != kMmrNone ? bp : fp;  // (t < picks <= n: an unselected candidate exists)
        }
        if (tid == 0) {
            sel[cur] = 1;
            od[t] = cdist[cur];  // the query distance with the bits the search returned
            orow[t] = crow[cur];
        }
        if (t == picks - 1) break;  // no update after the last pick
        // ---- the picked row becomes the LDS-resident vector
        const int32_t pr = lrow[cur];
        const float* prow = src.vec(cur, pr);
        for (int c = tid; c < dq; c += kMmrThreads) qv[c] = c < d ? prow[c] : 0.0f;
        const float np = src.nrm(cur, pr);
        __syncthreads();
        // ---- wave w scores candidates 64 (w + 4 round) + lane against it
        for (int r = 0; r < rounds; ++r) {
            const int i = kWave * (w + kMmrWaves * r) + lane;
            const bool live = i < n && !sel[i];
            const float* rp = live ? src.vec(i, lrow[i]) : nullptr;
            if (__builtin_amdgcn_ballot_w64(live) == 0) continue;  // (wave-uniform; staged_dot synchronises the wave only)
            const float dot = staged_dot(tiles + w * kStageFloats, rp, qv, d, lane);
            if (live) {
                const double s = mmr_sim(metric, distance_from(metric, dot, np, src.nrm(i, lrow[i])));
                if (t == 0) ms[i] = s;
                else if (s > ms[i]) ms[i] = s;  // (a NaN s is ignored)
            }
        }
        __syncthreads();
    }
    if (tid == 0 && picks > 1) {
        const unsigned long long p1 = (unsigned long long)(picks - 1);
        atomicAdd(pairs_scored, p1 * (unsigned long long)n - p1 * (unsigned long long)picks / 2);
    }
}

// grid: one workgroup per query.  cand_rows / cand_dist: [B, stride], GLOBAL rows (row_offset is subtracted here; -1 = none).
// out_dist / out_rows: [B, k].
__global__ __launch_bounds__(kMmrThreads) void k_mmr_select(const int64_t* __restrict__ cand_rows,
                                                            const double* __restrict__ cand_dist, int stride,
                                                            const float* __restrict__ rows, const float* __restrict__ nrm2,
                                                            int64_t n_rows, int64_t row_offset, int d, int metric, int k,
                                                            double lambda, double* __restrict__ out_dist,
                                                            int64_t* __restrict__ out_rows,
                                                            unsigned long long* __restrict__ pairs_scored) {
    const int64_t qb = (int64_t)blockIdx.x;
    const MmrLocalRows src{rows, nrm2, n_rows, row_offset, d};
    mmr_select_body(src, cand_rows + qb * stride, cand_dist + qb * stride, stride, d, metric, k, lambda, out_dist + qb * k,
                    out_rows + qb * k, pairs_scored);
}

}  // namespace mi355
