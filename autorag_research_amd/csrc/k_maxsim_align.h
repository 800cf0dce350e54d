// k_maxsim_align.h -- MaxSim explained: the terms of k_maxsim's sum instead of the sum.
//   k_maxsim_align       per (query vector, candidate): the maximum dot and the lowest token index that reaches it
//   k_maxsim_align_dist  the distances from the finished values: k_maxsim's tail, one fp32 add per vector in vector order
//   k_maxsim_map         every dot of listed (query, document) pairs, written out instead of folded
// Operands, walk and arithmetic are k_maxsim's (k_maxsim_exact.h: ms_load_piece / ms_compute_piece, the staged query image
// [col][dpad + 4], 32-token blocks ascending), so every dot is the same k-ascending fp32 fmaf chain.  Work comes as a table of
// TILES in device memory -- one workgroup row (blockIdx.y) per tile of at most ms_cols_for(dpad) vectors of one query -- and
// not as by-value arrays: nothing here indexes an argument array, nothing goes to the stack.
#pragma once
#include "k_maxsim_exact.h"

namespace mi355 {

// a tile: `len` consecutive query vectors from global vector `g0` on (rows of the packed query image [V][dpad])
struct MsAlignTile {
    int g0, len;
    int query;    // align: the query b whose candidate row the tile is scored against
    int doc;      // map: the local document (always one with vectors)
    int T;        // map: its token count
    int pad;
    int64_t out;  // map: element offset of vector g0's row in the output (row stride T)
};

struct MsAlignArgs {
    const float* tok;
    const int64_t* blk_off;
    const float* qtok;          // [V, dpad] every query vector of the call, packed (multivec_pack_query_row)
    const MsAlignTile* tiles;   // [gridDim.y]
    const int32_t* doc_list;    // align: [B, m] local documents; < 0 or >= n_docs: skipped
    float* out_val;             // align: [V, m]; map: the slots, one after the other
    int32_t* out_tok;           // align: [V, m]
    int m;                      // align: candidates per query
    int64_t n_docs;
    int dpad;
    int clamp0;
};

// the tile's query vectors -> the staged image, whole 32-column blocks (columns past the tile are zero: their results are dropped)
__device__ __forceinline__ void ms_align_stage(float* qs, const float* qtok, int len, int dpad, int tid) {
    const int ld = dpad + 4, ncb = (len + 31) / 32, w = dpad / 4;
    for (int i = tid; i < ncb * 32 * w; i += kMsThreads) {
        const int c = i / w, k4 = i - c * w;
        *(float4*)(qs + c * ld + k4 * 4) =
            c < len ? *(const float4*)(qtok + (int64_t)c * dpad + k4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// One wave per (tile, candidate).  Per block and column the maximum is found as k_maxsim finds it; the lowest row of the block
// that holds it follows from the C/D layout of the 32x32 MFMA: register r of lane l is token row (r & 3) + 8 (r >> 2) + 4 (l >> 5)
// of query column l & 31.  The running (maximum, token) moves only on a strictly greater block maximum -- blocks ascend, so the
// lowest index stays -- or when there is no token yet (a first maximum of -inf).  NaN dots never win: fmaxf drops them and
// equality fails on them.  The padded rows of a document's last block repeat its last token, so they tie with row T - 1 and lose
// to it: no index >= T can come out.
__global__ __launch_bounds__(kMsThreads, 2) void k_maxsim_align(const MsAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qs = (float*)smem;
    const int ld = a.dpad + 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the candidate, its document and its blocks stay out of the VGPRs)
    const MsAlignTile t = a.tiles[blockIdx.y];
    if ((int)blockIdx.x * 4 >= a.m) return;
    const int32_t* doc_list = a.doc_list + (int64_t)t.query * a.m;
    float* out_val = a.out_val + (int64_t)t.g0 * a.m;
    int32_t* out_tok = a.out_tok + (int64_t)t.g0 * a.m;
    const int ncb = (t.len + 31) / 32;
    ms_align_stage(qs, a.qtok + (int64_t)t.g0 * a.dpad, t.len, a.dpad, tid);
    __syncthreads();
    const int half = lane >> 5, col = lane & 31;
    const int nchunk = (a.dpad + 127) / 128;
    for (int item = (int)blockIdx.x * 4 + wave; item < a.m; item += (int)gridDim.x * 4) {
        const int64_t doc = doc_list[item];
        int64_t b0 = 0, b1 = 0;
        if (doc >= 0 && doc < a.n_docs) {
            b0 = a.blk_off[doc];
            b1 = a.blk_off[doc + 1];
        }
        if (b1 <= b0) {  // a skipped id or a document without vectors
            for (int c = lane; c < t.len; c += 64) {
                out_val[(int64_t)c * a.m + item] = __uint_as_float(0x7FC00000u);
                out_tok[(int64_t)c * a.m + item] = -1;
            }
            continue;
        }
        float run[4];
        int rtok[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            run[c] = -__builtin_inff();
            rtok[c] = -1;
        }
        const int npieces = (int)(b1 - b0) * nchunk;
        f32x16 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
        float4 pa[16], pb[16];
        auto row_of = [&](int p) { return a.tok + ((b0 + p / nchunk) * kMsBlkRows + col) * (int64_t)a.dpad + 4 * half; };
        auto finish_block = [&](int blk) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                if (cb >= ncb) break;
                float mx = acc[cb][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[cb][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
                int row = 64;  // (none: the block's maximum is NaN)
#pragma unroll
                for (int r = 15; r >= 0; --r)  // rows ascend with r inside a lane
                    if (acc[cb][r] == mx) row = (r & 3) + 8 * (r >> 2) + 4 * half;
                row = min(row, __shfl_xor(row, 32, kWave));
                if (row < 64 && (mx > run[cb] || rtok[cb] < 0)) {
                    run[cb] = mx;
                    rtok[cb] = blk * kMsBlkRows + row;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
            }
        };
        ms_load_piece(pa, row_of(0), 0, a.dpad);
        for (int p = 0; p < npieces; p += 2) {
            if (p + 1 < npieces) ms_load_piece(pb, row_of(p + 1), (p + 1) % nchunk, a.dpad);
            ms_compute_piece(acc, pa, qs, ld, ncb, col, half, p % nchunk, a.dpad);
            if ((p + 1) % nchunk == 0) finish_block(p / nchunk);
            if (p + 1 < npieces) {
                if (p + 2 < npieces) ms_load_piece(pa, row_of(p + 2), (p + 2) % nchunk, a.dpad);
                ms_compute_piece(acc, pb, qs, ld, ncb, col, half, (p + 1) % nchunk, a.dpad);
                if ((p + 2) % nchunk == 0) finish_block((p + 1) / nchunk);
            }
        }
        if (lane < 32) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int c = cb * 32 + lane;
                if (cb < ncb && c < t.len) {
                    const float v = run[cb];
                    out_val[(int64_t)c * a.m + item] = a.clamp0 ? fmaxf(v, 0.0f) : v;
                    out_tok[(int64_t)c * a.m + item] = rtok[cb];
                }
            }
        }
    }
}

// out_dist[b, p] from the finished values: acc = 0.0f; acc = acc + (-val) over the query's vectors in order -- the chain of
// k_maxsim's tail (its tiles carry the same sum through dist_in).  A candidate without values (NaN in its first row: a maximum
// taken by fmaxf from -inf is never NaN) and a query without vectors get the NaN k_maxsim writes.
__global__ __launch_bounds__(256) void k_maxsim_align_dist(const float* __restrict__ val, const int32_t* __restrict__ q_off, int B,
                                                           int64_t m, float* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * m) return;
    const int b = (int)(i / m);
    const int64_t p = i - (int64_t)b * m;
    const int g0 = q_off[b], g1 = q_off[b + 1];
    float accd = 0.0f;
    bool none = g1 <= g0;
    if (!none) none = val[(int64_t)g0 * m + p] != val[(int64_t)g0 * m + p];
    for (int g = g0; g < g1 && !none; ++g) accd = accd + (-val[(int64_t)g * m + p]);
    dist[i] = none ? __uint_as_float(0x7FC00000u) : accd;
}

// One workgroup per tile of a (query, document) pair; its four waves take the document's blocks w, w + 4, ...  The accumulators
// go straight to memory: a lane holds 16 tokens of ONE query vector, four runs of four consecutive tokens, so each of the 16
// stores of a block and column block writes 4-byte words that are consecutive in groups of four lanes' worth only (the strided
// form; no LDS transpose -- the image of a 768-dim tile leaves no room for four waves' 32x32 tiles).  Rows >= T are not written.
__global__ __launch_bounds__(kMsThreads, 2) void k_maxsim_map(const MsAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qs = (float*)smem;
    const int ld = a.dpad + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MsAlignTile t = a.tiles[blockIdx.x];
    const int ncb = (t.len + 31) / 32;
    ms_align_stage(qs, a.qtok + (int64_t)t.g0 * a.dpad, t.len, a.dpad, tid);
    __syncthreads();
    const int half = lane >> 5, col = lane & 31;
    const int nchunk = (a.dpad + 127) / 128;
    const int64_t b0 = a.blk_off[t.doc];
    const int nb = (int)min(a.blk_off[t.doc + 1] - b0, (int64_t)(t.T + kMsBlkRows - 1) / kMsBlkRows);  // (never past the document)
    float* out = a.out_val + t.out;
    for (int blk = wave; blk < nb; blk += 4) {
        f32x16 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
        float4 pa[16];
        const float* row = a.tok + ((b0 + blk) * kMsBlkRows + col) * (int64_t)a.dpad + 4 * half;
        for (int ch = 0; ch < nchunk; ++ch) {
            ms_load_piece(pa, row, ch, a.dpad);
            ms_compute_piece(acc, pa, qs, ld, ncb, col, half, ch, a.dpad);
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int c = cb * 32 + col;
            if (cb < ncb && c < t.len) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = blk * kMsBlkRows + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (j < t.T) out[(int64_t)c * t.T + j] = acc[cb][r];
                }
            }
        }
    }
}

}  // namespace mi355
