// k_compact.h -- compaction of the single-vector corpus (mi355dr_compact; DESIGN.md "Compaction").
//   k_compact_gather  pull the source rows of one slice of destination rows (fp32 row + nrm2) into a staging buffer
// The host copies the staging buffer to rows[dst0 ...] / nrm2[dst0 ...] behind the kernel, on the same stream: dst <= src for
// every row and the slices ascend, so a slice's writes land below every source a later slice reads, and inside a slice nothing
// of the index is written before all of it is read.  Derived data (both shadows, the group records, the side lists) is not
// moved: the builders add_rows uses rebuild it over the moved range, so it has the bits an add would have written.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kCompactWaves = 4;     // rows per workgroup: one wave each
// independent 16-byte loads per lane before the first store; what is left of a count that is no multiple goes in a pair and
// singly.  (Whole rounds without bounds tests: a round whose loads are each guarded has its register array promoted to LDS.)
constexpr int kCompactInflight = 4;

// grid: ceil(m / kCompactWaves) blocks of 64 * kCompactWaves threads.  Row j of the slice = index row src_of_dst[j] (int32,
// strictly ascending, inside the index: built by the host from nrm2) -> stage_rows[j], its nrm2 -> stage_nrm2[j].
// vec4: d % 4 == 0 and both bases 16-byte aligned -- whole float4, kCompactInflight loads in flight per lane; else scalar.
__global__ __launch_bounds__(64 * kCompactWaves) void k_compact_gather(const float* __restrict__ rows, const float* __restrict__ nrm2,
                                                                        const int32_t* __restrict__ src_of_dst, int64_t m, int d,
                                                                        int vec4, float* __restrict__ stage_rows,
                                                                        float* __restrict__ stage_nrm2) {
    const int64_t j = (int64_t)blockIdx.x * kCompactWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= m) return;
    const int64_t src = src_of_dst[j];
    const float* s = rows + src * (int64_t)d;
    float* t = stage_rows + j * (int64_t)d;
    if (lane == 0) stage_nrm2[j] = nrm2[src];
    if (vec4) {
        const float4* s4 = (const float4*)s;
        float4* t4 = (float4*)t;
        const int n4 = d / 4, count = lane < n4 ? (n4 - lane + kWave - 1) / kWave : 0;  // this lane's words: lane, lane + 64, ...
        int i = 0;
        for (; i + kCompactInflight <= count; i += kCompactInflight) {
            float4 v[kCompactInflight];
#pragma unroll
            for (int u = 0; u < kCompactInflight; ++u) v[u] = s4[lane + (i + u) * kWave];
#pragma unroll
            for (int u = 0; u < kCompactInflight; ++u) t4[lane + (i + u) * kWave] = v[u];
        }
        if (i + 2 <= count) {  // (d = 768: three words per lane -- two together, one singly)
            const float4 v0 = s4[lane + i * kWave], v1 = s4[lane + (i + 1) * kWave];
            t4[lane + i * kWave] = v0;
            t4[lane + (i + 1) * kWave] = v1;
            i += 2;
        }
        for (; i < count; ++i) t4[lane + i * kWave] = s4[lane + i * kWave];
    } else {
        for (int k = lane; k < d; k += kWave) t[k] = s[k];
    }
}

}  // namespace mi355
