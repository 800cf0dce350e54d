// k_maxsim_exact.h -- the exact fp32 MaxSim kernel (k_maxsim) and its argument block.  Walk, layout and the bit-exactness
// argument: the head of mi355dr_maxsim.hip; column order of the stored rows and of the staged query rows: ms_perm (index.h).
#pragma once
#include "maxsim_common.h"

namespace mi355 {

struct MsArgs {
    const float* tok;
    const int64_t* blk_off;
    const float* qtok;      // [kMsCols, dpad] zero-padded
    float* dist;            // [nq_launch, n_items]
    const int32_t* doc_list;  // optional [n_items]: the docs to score (nullptr: item i = doc i); < 0 or >= n_docs: NaN
    int64_t n_items;        // work items (= n_docs without a list)
    const int* n_items_dev; // optional: the real number of items (<= n_items, which then only sizes the grid / dist rows)
    int64_t list_stride;    // > 0: grid.y = query of the launch, each with its own doc_list / dist row (stride) and
                            //      n_items_dev pair (stride 2); the workgroup scores that query only
    int64_t n_docs;
    int dpad;
    int nq_launch;          // queries in this launch (<= 4 scored together; list mode with list_stride: <= kMsPassQueries, one per grid.y)
    int q_col0[kMsPassQueries];  // first column of each query in the staged image (any column)
    int q_len[kMsPassQueries];   // real token count of each query
    int clamp0;             // 1: every query token contributes max(0, max_j <q_i, d_j>)  (ColBERT reranker, rerankers/colbert.py:79)
    // a query with more vectors than one launch stages (ms_cols_for(dpad) <= 128 columns) is scored in TILES of its vectors:
    // the launch of tile t starts every item's sum from the value tile t-1 left (same layout as `dist`; may be `dist` itself),
    // so the fp32 sum still runs over the query's vectors in order -- bit for bit the one-launch chain
    const float* dist_in;
    // list mode, long documents (ColPali pages: 33 blocks): the four waves of a workgroup share ONE item -- wave w multiplies
    // blocks w, w + 4, ... -- and their per-column maxima meet in LDS (byte offset red_off of the dynamic segment, 2 KiB) before
    // wave 0 adds them up in token order.  A maximum does not depend on the order: the same bits as one wave per item.  With a
    // whole page per wave a 570-candidate list kept 570 of the chip's 1024 SIMDs busy for 33 blocks each, two deep where two
    // workgroups shared a CU: 0.5 ms per launch against 0.13 ms of fp32 MFMA work.
    int coop;
    int red_off;
};

// query-token columns one launch of k_maxsim stages: whole 32-column blocks, at most kMsCols, inside the 160 KiB of LDS
// (d = 128: 128 columns; d = 768, the hidden size the ColBERT reranker scores with: 32)
inline int ms_cols_for(int dpad) {
    const int c = (int)(((size_t)160 * 1024 - kMsRedBytes) / ((size_t)(dpad + 4) * sizeof(float))) / 32 * 32;
    return c < kMsCols ? c : kMsCols;
}

__device__ __forceinline__ void ms_load_piece(float4 (&a)[16], const float* row, int chunk, int dpad) {
    // this lane's 4 floats of every 8-dim group of dims [128*chunk, +128); groups past dpad read as zero
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int k0 = chunk * 128 + i * 8;
        a[i] = k0 < dpad ? load_gmem_f4(row + k0) : make_float4(0.f, 0.f, 0.f, 0.f);  // (global, not FLAT: dev_common.h)
    }
}

__device__ __forceinline__ void ms_compute_piece(f32x16 (&acc)[4], const float4 (&a)[16], const float* qs, int ld, int ncb,
                                                 int col, int half, int chunk, int dpad) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        if (cb >= ncb) break;
        const float* brow = qs + (cb * 32 + col) * ld + 4 * half + chunk * 128;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (chunk * 128 + i * 8 >= dpad) break;
            const float4 bv = *(const float4*)(brow + i * 8);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, bv.x, acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, bv.z, acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, bv.y, acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, bv.w, acc[cb], 0, 0, 0);
        }
    }
}

// B fragments: LDS image [col][dpad + 4] floats (the +4 pad makes the 16-lane groups of ds_read_b128 hit 16
// distinct 16-B slots).  The doc-token piece (32 rows x 128 dims = 16 float4 per lane) is register-resident
// and reused for every query column block; the next piece is prefetched while the current one is consumed.
__global__ __launch_bounds__(kMsThreads, 2) void k_maxsim(const MsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qs = (float*)smem;
    const int ld = a.dpad + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The argument block is read-only and its two small arrays are only ever indexed at compile time (unrolled selects):
    // a kernel that writes its by-value arguments, or indexes them with a run-time value, gets the whole block copied to the
    // stack first (65 scratch instructions in the round-4 build; pinned by tests/test_build_pipeline.py).
    const int32_t* doc_list = a.doc_list;
    float* dist = a.dist;
    const float* dist_in = a.dist_in;
    const int* n_items_dev = a.n_items_dev;
    const float* qtok = a.qtok;
    int nql = a.nq_launch;           // queries scored together by this workgroup: <= 4 (list mode: the one of blockIdx.y)
    int qc0[4], qln[4];              // their first column / token count (registers: every index below is a constant)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qc0[i] = a.q_col0[i];
        qln[i] = a.q_len[i];
    }
    if (a.list_stride > 0) {  // per-query candidate lists
        const int y = blockIdx.y;
        doc_list += (int64_t)y * a.list_stride;
        dist += (int64_t)y * a.list_stride;
        if (dist_in) dist_in += (int64_t)y * a.list_stride;
        n_items_dev += 2 * y;
        int c0 = a.q_col0[0], ln = a.q_len[0];
#pragma unroll
        for (int i = 1; i < kMsPassQueries; ++i)
            if (i == y) {
                c0 = a.q_col0[i];
                ln = a.q_len[i];
            }
        qtok += (int64_t)c0 * a.dpad;  // this query's columns become columns 0.. of the staged image (any c0)
        qc0[0] = 0;
        qln[0] = ln;
        nql = 1;
    }
    const int64_t n_items = n_items_dev ? min((int64_t)*n_items_dev, a.n_items) : a.n_items;
    const bool coop = a.coop != 0;
    if ((int64_t)blockIdx.x * (coop ? 1 : 4) >= n_items) return;  // nothing for this workgroup: skip staging the query block
    float* red = (float*)(smem + a.red_off);
    int ncb = 0;   // column blocks in use
#pragma unroll
    for (int qi = 0; qi < 4; ++qi)
        if (qi < nql) ncb = max(ncb, (qc0[qi] + qln[qi] + 31) / 32);
    for (int i = tid; i < ncb * 32 * (a.dpad / 4); i += kMsThreads) {
        const int c = i / (a.dpad / 4), k4 = i - c * (a.dpad / 4);
        *(float4*)(qs + c * ld + k4 * 4) = *(const float4*)(qtok + (int64_t)c * a.dpad + k4 * 4);
    }
    __syncthreads();
    const int half = lane >> 5, col = lane & 31;
    const int nchunk = (a.dpad + 127) / 128;
    // docs are dealt round-robin to the waves of the grid so long and short docs mix
    // (with a doc list the grid is small and fixed -- the real list length is only known on the device -- and the
    // waves stride over the list until it ends)
    for (int dw = 0; doc_list || dw < kMsDocsPerWave; ++dw) {
    const int64_t item = coop ? (int64_t)dw * gridDim.x + blockIdx.x : ((int64_t)dw * gridDim.x + blockIdx.x) * 4 + wave;
    if (item >= n_items) break;  // (cooperative: the same item in all four waves -- every branch on it is workgroup-uniform)
    const int64_t doc = doc_list ? (int64_t)doc_list[item] : item;
    if (doc < 0 || doc >= a.n_docs) {  // (subset scoring) not a stored doc
        if (lane == 0 && (!coop || wave == 0))
            for (int qi = 0; qi < nql; ++qi) dist[(int64_t)qi * a.n_items + item] = __uint_as_float(0x7FC00000u);
        continue;
    }
    const int64_t b0 = a.blk_off[doc], b1 = a.blk_off[doc + 1];
    const int bfirst = coop ? wave : 0, bstep = coop ? 4 : 1;  // this wave's blocks of the document: b0 + bfirst + bstep * i
    const int64_t nb_w = b1 - b0 > bfirst ? (b1 - b0 - bfirst + bstep - 1) / bstep : 0;
    float run[4];  // running max per column block (this lane's column)
#pragma unroll
    for (int c = 0; c < 4; ++c) run[c] = -__builtin_inff();

    const int64_t npieces = nb_w * nchunk;
    f32x16 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
    float4 pa[16], pb[16];
    auto row_of = [&](int64_t p) { return a.tok + ((b0 + bfirst + bstep * (p / nchunk)) * kMsBlkRows + col) * (int64_t)a.dpad + 4 * half; };
    auto finish_block = [&]() {  // block max per column: 16 rows in this lane, the other 16 in lane^32
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            if (cb >= ncb) break;
            float m = acc[cb][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[cb][r]);
            m = fmaxf(m, __shfl_xor(m, 32, kWave));
            run[cb] = fmaxf(run[cb], m);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
        }
    };
    if (npieces > 0) ms_load_piece(pa, row_of(0), 0, a.dpad);
    for (int64_t p = 0; p < npieces; p += 2) {
        if (p + 1 < npieces) ms_load_piece(pb, row_of(p + 1), (int)((p + 1) % nchunk), a.dpad);
        ms_compute_piece(acc, pa, qs, ld, ncb, col, half, (int)(p % nchunk), a.dpad);
        if ((p + 1) % nchunk == 0) finish_block();
        if (p + 1 < npieces) {
            if (p + 2 < npieces) ms_load_piece(pa, row_of(p + 2), (int)((p + 2) % nchunk), a.dpad);
            ms_compute_piece(acc, pb, qs, ld, ncb, col, half, (int)((p + 1) % nchunk), a.dpad);
            if ((p + 2) % nchunk == 0) finish_block();
        }
    }
    if (coop) {  // the four waves' column maxima -> wave 0
        if (lane < 32) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (cb < ncb) red[(wave * 4 + cb) * 32 + lane] = run[cb];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                if (cb >= ncb) break;
                float m = red[cb * 32 + col];
#pragma unroll
                for (int w = 1; w < 4; ++w) m = fmaxf(m, red[(w * 4 + cb) * 32 + col]);
                run[cb] = m;
            }
        }
        __syncthreads();  // (red is rewritten by the next item)
        if (wave != 0) continue;
    }
    // per query: distance = sum over its tokens (in order) of -(max dot); empty docs are skipped by the select
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
        if (qi >= nql) break;
        float accd = dist_in ? dist_in[(int64_t)qi * a.n_items + item] : 0.0f;  // (wave-uniform address)
        for (int j = 0; j < qln[qi]; ++j) {
            const int c = qc0[qi] + j;
            float v = 0.0f;
#pragma unroll
            for (int cbi = 0; cbi < 4; ++cbi)
                if (cbi == (c >> 5)) v = run[cbi];
            v = __shfl(v, c & 31, kWave);
            if (a.clamp0) v = fmaxf(v, 0.0f);
            accd = accd + (-v);
        }
        if (lane == 0) dist[(int64_t)qi * a.n_items + item] = b1 > b0 ? accd : __uint_as_float(0x7FC00000u);
    }
    }  // docs of this wave
}

}  // namespace mi355
