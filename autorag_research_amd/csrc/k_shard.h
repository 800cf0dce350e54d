// k_shard.h -- the device side of the row-sharded derived searches (range, by stored row, MMR).
// Every kernel here sits on one side of an all-gather: it fills this rank's payload or folds the gathered payloads of all
// ranks into what ONE index holding every row would have had.
//   k_shard_fill_lists   an empty shard's contribution: NaN / -1 lists and zero counts
//   k_shard_rows_fold    by-row search: per slot the query vector, valid_any and self distance of the lowest rank that owns it
//   k_shard_count_fold   range search: out_count[b] = sum over the ranks of count_r[b]
//   k_shard_mmr_stage    MMR: per (query, candidate) of the merged list the owner's fp32 vector, stored |row|^2 and owned flag
//   k_shard_mmr_select   MMR: mmr_select_body (k_mmr.h) reading candidate i from stage[owner(i)]
// Plain HIP C++: vector loads and stores, one atomicAdd per slot no rank owns.
#pragma once
#include "dev_common.h"
#include "k_mmr.h"

namespace mi355 {

constexpr int kShardThreads = 256;

// ---- payload layouts (int64 words / floats per rank; every payload is a multiple of 8 bytes: RCCL moves ncclInt64) ----------
// by-row search, one block of nb slots: [nb * d floats, padded to a word][nb int32 valid, padded to a word][nb double self_dist]
__host__ __device__ inline int64_t shard_rows_qwords(int nb, int d) { return ((int64_t)nb * d + 1) / 2; }
__host__ __device__ inline int64_t shard_rows_vwords(int nb) { return ((int64_t)nb + 1) / 2; }
__host__ __device__ inline int64_t shard_rows_words(int nb, int d) { return shard_rows_qwords(nb, d) + shard_rows_vwords(nb) + nb; }
// MMR stage, one sub-block of cnt = queries x stride candidates: [cnt * d floats][cnt floats |row|^2][cnt int32 owned], padded
// to 4 floats (a rank's stage starts 16-B aligned, as staged_dot's float4 loads need when d % 4 == 0)
__host__ __device__ inline int64_t shard_stage_floats(int64_t cnt, int d) { return (cnt * (d + 2) + 3) & ~(int64_t)3; }

// grid: enough workgroups for n_entries (and nb).  dist / rows: n_entries entries; count: [nb] or null
__global__ __launch_bounds__(kShardThreads) void k_shard_fill_lists(double* __restrict__ dist, int64_t* __restrict__ rows,
                                                                     int64_t n_entries, int64_t* __restrict__ count, int nb) {
    const int64_t i = (int64_t)blockIdx.x * kShardThreads + threadIdx.x;
    if (i < n_entries) {
        dist[i] = __longlong_as_double(0x7FF8000000000000ll);
        rows[i] = -1;
    }
    if (count && i < nb) count[i] = 0;
}

// grid: one workgroup per slot.  all: [world][rank_words] the gathered payloads; q_out: [nb, d]; valid_any / self_dist: [nb]
// (no owner: a zero vector, 0 and NaN, counted in `skipped`).  Shards are disjoint; the LOWEST rank whose valid is set wins.
__global__ __launch_bounds__(kShardThreads) void k_shard_rows_fold(const int64_t* __restrict__ all, int64_t rank_words, int world,
                                                                    int nb, int d, float* __restrict__ q_out,
                                                                    int* __restrict__ valid_any, double* __restrict__ self_dist,
                                                                    unsigned long long* __restrict__ skipped) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t qw = shard_rows_qwords(nb, d), vw = shard_rows_vwords(nb);
    int owner = -1;  // block-uniform
    for (int r = 0; r < world && owner < 0; ++r)
        if (((const int*)(all + r * rank_words + qw))[b]) owner = r;
    float* dst = q_out + (int64_t)b * d;
    if (owner >= 0) {
        const float* src = (const float*)(all + owner * rank_words) + (int64_t)b * d;
        if (d % 4 == 0 && ((uintptr_t)src & 15) == 0) {  // (a rank's payload starts 8-B aligned only; block-uniform)
            const float4* s4 = (const float4*)src;
            float4* d4 = (float4*)dst;
            for (int c = tid; c < d / 4; c += kShardThreads) d4[c] = s4[c];
        } else {
            for (int c = tid; c < d; c += kShardThreads) dst[c] = src[c];
        }
    } else {
        for (int c = tid; c < d; c += kShardThreads) dst[c] = 0.0f;
    }
    if (tid == 0) {
        valid_any[b] = owner >= 0 ? 1 : 0;
        self_dist[b] = owner >= 0 ? ((const double*)(all + owner * rank_words + qw + vw))[b]
                                  : __longlong_as_double(0x7FF8000000000000ll);
        if (owner < 0) atomicAdd(skipped, 1ull);
    }
}

// grid: ceil(nb / kShardThreads).  rank r's counts: all + r * rank_stride + count_off, [nb] int64
__global__ __launch_bounds__(kShardThreads) void k_shard_count_fold(const int64_t* __restrict__ all, int64_t rank_stride,
                                                                     int64_t count_off, int world, int nb,
                                                                     int64_t* __restrict__ out_count) {
    const int b = blockIdx.x * kShardThreads + threadIdx.x;
    if (b >= nb) return;
    int64_t sum = 0;
    for (int r = 0; r < world; ++r) sum += all[r * rank_stride + count_off + b];
    out_count[b] = sum;
}

// grid: one wave per (query, candidate) entry e < cnt of the sub-block.  cand_rows: [cnt] GLOBAL rows of the merged lists.
// stage: this rank's [shard_stage_floats(cnt, d)].  An entry this shard does not hold gets flag 0 and nothing else.
__global__ __launch_bounds__(kWave) void k_shard_mmr_stage(const int64_t* __restrict__ cand_rows, int64_t cnt,
                                                            const float* __restrict__ rows, const float* __restrict__ nrm2,
                                                            int64_t n_rows, int64_t row_offset, int d,
                                                            float* __restrict__ stage) {
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t id = cand_rows[e];
    const uint64_t local = (uint64_t)id - (uint64_t)row_offset;
    const bool mine = id >= row_offset && local < (uint64_t)n_rows;  // wave-uniform
    float* nrm_out = stage + cnt * d;
    int32_t* flag_out = (int32_t*)(nrm_out + cnt);
    if (mine) {
        const float* src = rows + (int64_t)local * d;
        float* dst = stage + e * d;
        if (d % 4 == 0) {
            const float4* s4 = (const float4*)src;
            float4* d4 = (float4*)dst;
            for (int c = lane; c < d / 4; c += kWave) d4[c] = s4[c];
        } else {
            for (int c = lane; c < d; c += kWave) dst[c] = src[c];
        }
    }
    if (lane == 0) {
        flag_out[e] = mine ? 1 : 0;
        nrm_out[e] = mine ? nrm2[local] : 0.0f;
    }
}

// the gathered stage as mmr_select_body's source: candidate i of this query is entry e0 + i of every rank's stage; its
// locator is the owning rank (the lowest one whose flag is set), resolved once in the body's prologue
struct MmrStagedRows {
    const float* stage;     // [world][rank_floats]
    int64_t rank_floats;
    int world;
    int64_t cnt, e0;
    int d;
    __device__ __forceinline__ bool locate(int i, int64_t r, int32_t* loc) const {
        if (r < 0) return false;
        for (int rk = 0; rk < world; ++rk) {
            const int32_t* flags = (const int32_t*)(stage + rk * rank_floats + cnt * d + cnt);
            if (flags[e0 + i]) {
                *loc = rk;
                return true;
            }
        }
        return false;
    }
    __device__ __forceinline__ const float* vec(int i, int32_t loc) const { return stage + loc * rank_floats + (e0 + i) * d; }
    __device__ __forceinline__ float nrm(int i, int32_t loc) const { return stage[loc * rank_floats + cnt * d + e0 + i]; }
};

// grid: one workgroup per query of the sub-block (its lists and outputs start at the sub-block's first query); dynamic LDS:
// mmr_lds_bytes(d, stride), as k_mmr_select
__global__ __launch_bounds__(kMmrThreads) void k_shard_mmr_select(const int64_t* __restrict__ cand_rows,
                                                                  const double* __restrict__ cand_dist, int stride,
                                                                  const float* __restrict__ stage_all, int64_t rank_floats,
                                                                  int world, int64_t cnt, int d, int metric, int k, double lambda,
                                                                  double* __restrict__ out_dist, int64_t* __restrict__ out_rows,
                                                                  unsigned long long* __restrict__ pairs_scored) {
    const int64_t qb = (int64_t)blockIdx.x;
    const MmrStagedRows src{stage_all, rank_floats, world, cnt, qb * stride, d};
    mmr_select_body(src, cand_rows + qb * stride, cand_dist + qb * stride, stride, d, metric, k, lambda, out_dist + qb * k,
                    out_rows + qb * k, pairs_scored);
}

}  // namespace mi355
