// k_block.h -- the small kernels the block schedule of mi355dr.hip puts between the screens, the prunes and the scans.
//   k_set_counts       every list of a block holds the same number of candidates (behind an emit-all chunk)
//   k_reset_queries    empty lists and kept sets for the queries the exact scan recomputes
//   k_gather_queries, k_scatter_results    a fix-up's sub-block: its queries out of the block, its results back into it
#pragma once
#include "dev_common.h"

namespace mi355 {

__global__ void k_set_counts(int* cnt, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cnt[i] = v;
}

__global__ void k_reset_queries(QueryState st, const int* qlist, int nq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int q = qlist[i];
    st.cnt[q] = 0;
    st.carry[q] = 0;
    st.best_n[q] = 0;
    st.thr_key[q] = kKeyNaN;
    st.thr_row[q] = 0x7FFFFFFF;
    st.status[q] &= ~kStOverflow;
}

// rows `map[j]` of src -> row j of dst (d floats each)
__global__ void k_gather_queries(const float* src, const int* map, int d, float* dst) {
    const int j = blockIdx.x;
    for (int c = threadIdx.x; c < d; c += blockDim.x) dst[(int64_t)j * d + c] = src[(int64_t)map[j] * d + c];
}
// result j of the re-screened sub-block -> slot map[j] of the block's outputs
__global__ void k_scatter_results(const double* sd, const int64_t* sr, const int* map, int k, double* od, int64_t* orow) {
    const int j = blockIdx.x;
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        od[(int64_t)map[j] * k + i] = sd[(int64_t)j * k + i];
        orow[(int64_t)map[j] * k + i] = sr[(int64_t)j * k + i];
    }
}

}  // namespace mi355
