// k_maxsim_build.h -- builders of the multi-vector store's device images (host side: mi355dr_maxsim.hip).
//   k_ms_build     padded fp32 image, bf16 fragment image and the bound maxima of new documents (every add goes through it)
//   k_ms_build_at  the same block body with an explicit destination block per workgroup (mi355dr_set_multivec)
//   k_ms_relayout  moves the blocks of untouched documents into a store laid out anew (mi355dr_set_multivec, block counts changed)
//   k_ms_pack8     the granule-packed bf16 copy (k_maxsim_wg8.h) from the padded one
#pragma once
#include "maxsim_common.h"

namespace mi355 {

__device__ __forceinline__ uint16_t dev_bf16_rn(float f) {  // same rounding as host_bf16_rn
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// one 32-row block of document i (slice-local), block `bi` of the document, written as block `dst_blk` of the store: the padded
// fp32 image (columns permuted: ms_perm, index.h), the bf16 fragment image, and the store-wide maxima of the screen bound
// (non-negative doubles order like their bit patterns).  The ONE body behind every image the store holds: an image written by
// a set has the bits an add would have written.
__device__ __forceinline__ void ms_build_block(const float* __restrict__ vecs, int64_t tok0, int64_t T, int64_t bi, int64_t dst_blk,
                                               int d, int dp, int nkk, float* tok, uint16_t* tok16, unsigned long long* stats,
                                               int* not_finite) {
    const int lane = threadIdx.x;
    for (int r = 0; r < kMsBlkRows; ++r) {
        const float* sv = vecs + (tok0 + min(bi * kMsBlkRows + r, T - 1)) * (int64_t)d;
        float* dst = tok + (dst_blk * kMsBlkRows + r) * (int64_t)dp;
        for (int j = lane; j < dp; j += 64) {
            const int c = ms_perm(j);
            dst[j] = c < d ? sv[c] : 0.0f;
        }
    }
    {
        const int r = lane & 31, hf = lane >> 5;
        const float* sv = vecs + (tok0 + min(bi * kMsBlkRows + r, T - 1)) * (int64_t)d;
        for (int kk = 0; kk < nkk; ++kk) {
            uint16_t* dst = tok16 + (((dst_blk * nkk + kk) * 64 + lane) * (int64_t)8);
            for (int j = 0; j < 8; ++j) {
                const int c = kk * 16 + hf * 8 + j;
                dst[j] = c < d ? dev_bf16_rn(sv[c]) : (uint16_t)0;
            }
        }
    }
    if (lane < kMsBlkRows && bi * kMsBlkRows + lane < T) {  // the real tokens of this block: norms, residual, finiteness
        const float* sv = vecs + (tok0 + bi * kMsBlkRows + lane) * (int64_t)d;
        double n2 = 0.0, n16 = 0.0, r2 = 0.0;
        bool fin = true;
        for (int c = 0; c < d; ++c) {
            const float f = sv[c];
            fin = fin && (fabsf(f) <= 3.402823466e38f);
            const double x = f, x16 = __uint_as_float((uint32_t)dev_bf16_rn(f) << 16);
            n2 += x * x;
            n16 += x16 * x16;
            r2 += (x - x16) * (x - x16);
        }
        if (!fin) atomicExch(not_finite, 1);
        if (n2 == n2 && n2 <= 1.7976931348623157e308) {
            atomicMax(&stats[0], (unsigned long long)__double_as_longlong(sqrt(n2)));
            atomicMax(&stats[1], (unsigned long long)__double_as_longlong(sqrt(n16)));
            atomicMax(&stats[2], (unsigned long long)__double_as_longlong(sqrt(r2)));
        }
    }
}

// one workgroup (64 lanes) per NEW 32-row block, the blocks of a slice's documents one after the other from blk_base on
__global__ __launch_bounds__(64) void k_ms_build(const float* __restrict__ vecs, const int64_t* __restrict__ doc_tok0,
                                                  const int64_t* __restrict__ doc_T, const int32_t* __restrict__ blk_doc,
                                                  const int64_t* __restrict__ doc_blk0, int d, int dp, int nkk, int64_t blk_base,
                                                  float* tok, uint16_t* tok16, unsigned long long* stats, int* not_finite) {
    const int64_t b = blockIdx.x;
    const int i = blk_doc[b];
    ms_build_block(vecs, doc_tok0[i], doc_T[i], b - doc_blk0[i], blk_base + b, d, dp, nkk, tok, tok16, stats, not_finite);
}

// the same with the destination named per document: block bi of document i goes to block doc_dst0[i] + bi of the store
__global__ __launch_bounds__(64) void k_ms_build_at(const float* __restrict__ vecs, const int64_t* __restrict__ doc_tok0,
                                                     const int64_t* __restrict__ doc_T, const int32_t* __restrict__ blk_doc,
                                                     const int64_t* __restrict__ doc_blk0, const int64_t* __restrict__ doc_dst0,
                                                     int d, int dp, int nkk, float* tok, uint16_t* tok16, unsigned long long* stats,
                                                     int* not_finite) {
    const int64_t b = blockIdx.x;
    const int i = blk_doc[b];
    const int64_t bi = b - doc_blk0[i];
    ms_build_block(vecs, doc_tok0[i], doc_T[i], bi, doc_dst0[i] + bi, d, dp, nkk, tok, tok16, stats, not_finite);
}

// ---- relayout (mi355dr_set_multivec when a document's block count changes) ----
// A run = a maximal stretch of untouched documents: its n blocks move from src0 to dst0 by one constant shift.  Runs are sorted by
// dst0 and do not overlap; the blocks between them belong to the touched documents (k_ms_build_at writes those).
struct MsRun {
    int64_t dst0, src0, n;
};
constexpr int kMsRelayoutWaves = 4;  // destination blocks per workgroup

// count 16-byte words per lane, 64 lanes side by side (1 KiB per word): eight loads in flight per lane, then their stores (d = 128:
// two such rounds for a block of the fp32 image, one for the bf16 image); what is left of a count that is no multiple goes singly
__device__ __forceinline__ void ms_copy_block(const uint4* __restrict__ src, uint4* __restrict__ dst, int count) {
    int i = 0;
    for (; i + 8 <= count; i += 8) {
        uint4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)(i + j) * 64];
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[(int64_t)(i + j) * 64] = v[j];
    }
    for (; i < count; ++i) dst[(int64_t)i * 64] = src[(int64_t)i * 64];
}

// one wave per DESTINATION block: finds its run by binary search (a block of a touched document finds none and leaves) and
// copies that block of both images, 16 bytes per lane and access.  tok_words = dpad / 8: the fp32 image's 16-byte words per
// lane and block (32 rows x dpad floats = 64 lanes x dpad / 8 words); the bf16 image's are nkk.
__global__ __launch_bounds__(64 * kMsRelayoutWaves) void k_ms_relayout(const uint4* __restrict__ tok_src, const uint4* __restrict__ tok16_src,
                                                                        const MsRun* __restrict__ runs, int n_runs, int64_t n_blocks,
                                                                        int tok_words, int nkk, uint4* __restrict__ tok_dst,
                                                                        uint4* __restrict__ tok16_dst) {
    const int64_t b = (int64_t)blockIdx.x * kMsRelayoutWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= n_blocks) return;
    int lo = 0, hi = n_runs - 1;  // the last run with dst0 <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (runs[mid].dst0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const MsRun r = runs[lo];
    if (b < r.dst0 || b >= r.dst0 + r.n) return;
    const int64_t sb = r.src0 + (b - r.dst0);
    ms_copy_block(tok_src + sb * tok_words * 64 + lane, tok_dst + b * tok_words * 64 + lane, tok_words);
    ms_copy_block(tok16_src + sb * nkk * 64 + lane, tok16_dst + b * nkk * 64 + lane, nkk);
}

// ---- the granule-packed bf16 copy (k_maxsim_wg8.h) ----
// one wave per PACKED block: lane = (row = lane & 31, half = lane >> 5) copies its 16-byte fragment of every k-group from the padded
// copy -- same bf16 values, so the two copies screen to bit-identical distances.  Row r of packed block p is token
// min(8 (granule - goff[doc]) + r % 8, T - 1) of the doc that owns granule 4 p + r / 8; rows past the last granule repeat the
// stream's last token (no workgroup ever folds them).
__global__ __launch_bounds__(64) void k_ms_pack8(const uint4* __restrict__ tok16, const int64_t* __restrict__ blk_off,
                                                 const int32_t* __restrict__ tok_cnt, const int64_t* __restrict__ goff,
                                                 int64_t n_docs, int64_t n_gran, int nkk, uint4* __restrict__ out, int64_t p0) {
    const int64_t p = p0 + blockIdx.x;
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    int64_t gi = p * 4 + (r >> 3);
    int rr = r & 7;
    if (gi >= n_gran) {
        gi = n_gran - 1;
        rr = 7;
    }
    int64_t lo = 0, hi = n_docs - 1;  // the doc with goff[doc] <= gi < goff[doc + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (goff[mid + 1] > gi) hi = mid;
        else lo = mid + 1;
    }
    const int64_t t = min((gi - goff[lo]) * 8 + rr, (int64_t)tok_cnt[lo] - 1);
    const uint4* src = tok16 + ((blk_off[lo] + (t >> 5)) * nkk) * 64 + (int)(t & 31) + 32 * hf;
    uint4* dst = out + (p * nkk) * 64 + lane;
    for (int kk = 0; kk < nkk; ++kk) dst[(int64_t)kk * 64] = src[(int64_t)kk * 64];
}

}  // namespace mi355
