// k_view.h -- the gathers behind mi355dr_view_create (DESIGN.md "Views"): the listed rows / documents of a parent index,
// pulled slice by slice into a staging buffer that the view's own add paths then read.
//   k_view_gather_nrm2  nrm2 of the listed rows -> [m]: the host reads these m words back and drops the removed rows
//                       (kDeadNrm2) from the list before any row is gathered
//   k_view_gather_rows  rows ids[j] of the parent's fp32 corpus -> stage[j]        (sorted ids: ascending addresses)
//   k_view_gather_toks  32-token blocks of the parent's padded, column-permuted MaxSim image -> [sum_T, dim] fp32 tokens in
//                       the caller's column order and without the padding: what mi355dr_add_multivec_device takes
// Only derived data's SOURCE is gathered: shadows, group records, side lists and the bound maxima are rebuilt by the view's
// add paths, so they have the bits an add of exactly these rows would have written.
#pragma once
#include "dev_common.h"
#include "index.h"  // ms_perm
#include "maxsim_common.h"

namespace mi355 {

constexpr int kViewWaves = 4;     // rows per workgroup: one wave each
// independent 16-byte loads per lane before the first store (d = 768: three words per lane, one round)
constexpr int kViewInflight = 4;

// grid: ceil(m / 256) blocks of 256 threads
__global__ __launch_bounds__(256) void k_view_gather_nrm2(const float* __restrict__ nrm2, const int32_t* __restrict__ ids,
                                                           int64_t m, float* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = nrm2[ids[j]];
}

// grid: ceil(m / kViewWaves) blocks of 64 * kViewWaves threads; one wave per row, lanes side by side along the row.
// ids: int32, strictly ascending, every one inside the parent (the host built them from the caller's list and the norms).
// vec4: d % 4 == 0 and both bases 16-byte aligned -- whole float4 words, up to kViewInflight loads in flight per lane
// (whole rounds without bounds tests, so the register array stays in registers); else one float per lane and access.
__global__ __launch_bounds__(64 * kViewWaves) void k_view_gather_rows(const float* __restrict__ rows, const int32_t* __restrict__ ids,
                                                                       int64_t m, int d, int vec4, float* __restrict__ stage) {
    const int64_t j = (int64_t)blockIdx.x * kViewWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= m) return;
    const float* s = rows + (int64_t)ids[j] * d;
    float* t = stage + j * (int64_t)d;
    if (vec4) {
        const float4* s4 = (const float4*)s;
        float4* t4 = (float4*)t;
        const int n4 = d / 4, count = lane < n4 ? (n4 - lane + kWave - 1) / kWave : 0;  // this lane's words: lane, lane + 64, ...
        int i = 0;
        for (; i + kViewInflight <= count; i += kViewInflight) {
            float4 v[kViewInflight];
#pragma unroll
            for (int u = 0; u < kViewInflight; ++u) v[u] = s4[lane + (i + u) * kWave];
#pragma unroll
            for (int u = 0; u < kViewInflight; ++u) t4[lane + (i + u) * kWave] = v[u];
        }
        if (i + 2 <= count) {
            const float4 v0 = s4[lane + i * kWave], v1 = s4[lane + (i + 1) * kWave];
            t4[lane + i * kWave] = v0;
            t4[lane + (i + 1) * kWave] = v1;
            i += 2;
        }
        for (; i < count; ++i) t4[lane + i * kWave] = s4[lane + i * kWave];
    } else {
        for (int c = lane; c < d; c += kWave) t[c] = s[c];
    }
}

// One 32-token block of a listed document: block `src_blk` of the parent's image holds `cnt` (1 ... 32) real tokens in front of
// its padding; they become tokens dst_tok ... dst_tok + cnt of the staging buffer.
struct ViewTokBlock {
    int64_t src_blk, dst_tok;
    int32_t cnt, pad_;
};

// grid: one workgroup of 64 * kViewWaves threads per block of `blocks`; wave w moves tokens w, w + kViewWaves, ...
// Stored position p of a token row holds column ms_perm(p), and ms_perm is its own inverse inside every group of 8: column c
// is read from position ms_perm(c) -- a lane's 4-byte load stays inside the 32-byte group its neighbours read, the stores are
// consecutive.  Columns >= d (the image's zero padding to dpad) are not read.
__global__ __launch_bounds__(64 * kViewWaves) void k_view_gather_toks(const float* __restrict__ tok, const ViewTokBlock* __restrict__ blocks,
                                                                       int d, int dpad, float* __restrict__ stage) {
    const ViewTokBlock b = blocks[blockIdx.x];
    const int lane = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < b.cnt; r += kViewWaves) {
        const float* s = tok + (b.src_blk * kMsBlkRows + r) * (int64_t)dpad;
        float* t = stage + (b.dst_tok + r) * (int64_t)d;
        for (int c = lane; c < d; c += kWave) t[c] = s[ms_perm(c)];
    }
}

}  // namespace mi355
