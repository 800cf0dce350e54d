// k_scan_ids.h -- the exact scan over a LISTED subset of rows (mi355dr_search_subset): k_scan with one indirection.
// A wave owns 64 list POSITIONS instead of 64 consecutive rows: lane l stages the row `rows + ids[p] * d` of its position
// p, and everything between the staging and the epilogue is k_scan's, instruction for instruction -- the query piece, the
// padded LDS image, the v_mfma_f32_32x32x2_f32 chain (k ascending, one rounding per product, zero padding that adds
// fma(0, 0, acc) = acc).  The dot of a (query, row) pair therefore has the bits k_scan gives it, and so has its key.
// The epilogue names a pair by its TRUE row: accumulator element (rb, r) belongs to position wpos0 + local index, whose row
// is ids[position] -- every lane parks its id in a 1 KiB LDS strip behind the tiles when it loads it (one write) and reads
// the 32 it needs there at the end (one address per wave half: broadcasts).  Not kept in a register and not loaded twice:
// either way one more 64-bit value lives across the K loop, and at the kernel's 256-VGPR budget it is spilled to the stack.
// nrm2, the dead-row test, the (key, row) < (thr_key, thr_row) test and the candidate's cand_row all use that row, so exact
// ties break by row whatever the list looks like.  The host passes the list sorted ascending and unique (positions in row
// order: neighbouring lanes read neighbouring parts of HBM) with every id inside [0, n): the kernel does not range-check.
// Only this generic form exists (every d, d % 4 != 0 included).  An LDS-DMA form in k_scan32's manner is expressible --
// its eight-rows-per-instruction pieces take per-lane source addresses -- and was not built: see DESIGN.md section 4.5.
// Reference semantics: base.py:409-415 with `AND id = ANY(:ids)` (sequential scan + ORDER BY distance LIMIT k).
#pragma once
#include "k_scan.h"

namespace mi355 {

struct ScanIdsArgs {
    ScanArgs s;          // row0 / row1: the chunk in list POSITIONS [pos0, pos1)
    const int32_t* ids;  // [m] local rows, ascending, unique, each in [0, n)
};

// k_scan's tiles + the workgroup's 256 ids (77.5 KiB: still two workgroups per CU)
__host__ __device__ inline size_t scan_ids_lds_bytes(int d, int nq) { return scan_lds_bytes(d, nq) + kScanThreads * sizeof(int32_t); }

__global__ __launch_bounds__(kScanThreads, 2) void k_scan_ids(ScanIdsArgs ia) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ScanArgs& a = ia.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* tile = (float*)smem + wave * kStageFloats;
    float* qtile = (float*)smem + 4 * kStageFloats;  // shared by the four waves
    int32_t* wid = (int32_t*)((float*)smem + 4 * kStageFloats + kScanQTileFloats) + wave * kWave;  // this wave's 64 ids
    const int64_t wpos0 = a.row0 + (int64_t)blockIdx.x * kScanThreads + wave * kWave;
    // (a wave past the end of the chunk keeps walking with idle slots: the query piece is handed over at block barriers)
    const int64_t mypos = wpos0 + lane;
    const int32_t myid = mypos < a.row1 ? ia.ids[mypos] : -1;  // idle slot: no row
    wid[lane] = myid;  // (read by the wave's other lanes in the epilogue, behind the K loop's barriers)
    const float* rp = myid >= 0 ? a.rows + (int64_t)myid * a.d : nullptr;
    const int lq = lane & 31;
    const float* qp = (lane < 32 && lq < a.nq) ? a.q + (int64_t)a.qlist[lq] * a.d : nullptr;  // lanes 32..63: idle slots
    const int d = a.d;
    const bool vec = (d & 3) == 0;

    scan_f32x16 acc[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][r] = 0.0f;

    // this wave's quarter of the query piece: groups g = 2 wave, 2 wave + 1 (query rows 8 wave .. 8 wave + 7)
    struct QPiece {
        float4 v[2];
    };
    StageRows sr;
    StagePiece p0, p1;
    QPiece q0, q1;
    bool dense = false;  // (k_scan: idle slots read a live lane's row, pieces inside the rows need no per-load predicate)
    auto issue = [&](StagePiece& p, const StageRows& r, int k0) __attribute__((always_inline)) {
        if (dense && k0 + kStageCols <= d) stage_issue_dense(p, r, k0, lane);  // wave-uniform
        else stage_issue(p, r, k0, d, lane);
    };
    int qoff[2] = {-1, -1};  // this wave's two query rows as float offsets from a.q
    auto issue_q = [&](QPiece& p, int k0) __attribute__((always_inline)) {
        const int c4 = (lane & 15) * 4;
#pragma unroll
        for (int u = 0; u < 2; ++u)
            p.v[u] = (qoff[u] >= 0 && k0 + c4 < d) ? load_gmem_f4(a.q + qoff[u] + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    if (vec) {
        const bool dr = stage_rows_init_dense(sr, rp, lane);
        {
            StageRows sq;
            const bool dq = stage_rows_init_dense(sq, qp, lane);
            dense = dr && dq;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float* src = wave == 0 ? sq.r[u] : wave == 1 ? sq.r[2 + u] : wave == 2 ? sq.r[4 + u] : sq.r[6 + u];
                qoff[u] = src != nullptr ? (int)(src - a.q) : -1;  // (query blocks are far below 2^31 floats)
            }
        }
        issue(p0, sr, 0);
        issue_q(q0, 0);
        if (kStageCols < d) {
            issue(p1, sr, kStageCols);
            issue_q(q1, kStageCols);
        }
    }
    const int h = lane >> 5;
    const float* ta0 = tile + lq * kStageLd;
    const float* ta1 = tile + (32 + lq) * kStageLd;
    const float* tb = qtile + lq * kStageLd;
    auto mfma_piece = [&]() {
#pragma unroll 4
        for (int u = 0; u < kStageCols / 4; ++u) {
            const float4 a0 = *(const float4*)(ta0 + 4 * u), a1 = *(const float4*)(ta1 + 4 * u);
            const float4 b = *(const float4*)(tb + 4 * u);
            const float bx = h ? b.y : b.x, bz = h ? b.w : b.z;
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0.y : a0.x, bx, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1.y : a1.x, bx, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0.w : a0.z, bz, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1.w : a1.z, bz, acc[1], 0, 0, 0);
        }
    };
    auto commit_q = [&](const QPiece& p) {  // rows 4 g + (lane >> 4), g = 2 wave + u
        const int sub = lane >> 4, c4 = (lane & 15) * 4;
#pragma unroll
        for (int u = 0; u < 2; ++u) *(float4*)(qtile + ((2 * wave + u) * 4 + sub) * kStageLd + c4) = p.v[u];
    };
    if (vec) {
        for (int k0 = 0; k0 < d; k0 += 2 * kStageCols) {
            stage_commit(tile, p0, lane);  // (wave_sync before and after: this wave's rows)
            __syncthreads();               // every wave is done reading the previous query piece
            commit_q(q0);
            __syncthreads();               // the query piece is complete
            if (k0 + 2 * kStageCols < d) {
                issue(p0, sr, k0 + 2 * kStageCols);
                issue_q(q0, k0 + 2 * kStageCols);
            }
            mfma_piece();
            if (k0 + kStageCols < d) {
                stage_commit(tile, p1, lane);
                __syncthreads();
                commit_q(q1);
                __syncthreads();
                if (k0 + 3 * kStageCols < d) {
                    issue(p1, sr, k0 + 3 * kStageCols);
                    issue_q(q1, k0 + 3 * kStageCols);
                }
                mfma_piece();
            }
        }
    } else {  // rows not 16-B aligned: scalar staging, no prefetch (rare dims)
        for (int k0 = 0; k0 < d; k0 += kStageCols) {
            stage_rows(tile, rp, k0, d, lane);
            __syncthreads();
            for (int s = wave * 8; s < wave * 8 + 8; ++s) {  // query rows, one scalar column per lane; 8 rows per wave
                const int qi = s < a.nq ? a.qlist[s] : -1;
                const int k = k0 + lane;
                qtile[s * kStageLd + lane] = (qi >= 0 && k < d) ? a.q[(int64_t)qi * d + k] : 0.0f;
            }
            __syncthreads();
            mfma_piece();
        }
    }

    // ---- epilogue.  C/D layout: column (query) = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) within each block of 32.
    wave_sync();  // (the ids parked at the start: at least one block barrier lies between, this keeps the compiler honest)
    if (lq >= a.nq || wpos0 >= a.row1) return;
    const int q = a.qlist[lq];
    const uint64_t tk = a.st.thr_key[q];
    const int32_t tr = a.st.thr_row[q];
    const float qn = a.st.qn[q];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int li = 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (wpos0 + li >= a.row1) continue;  // idle slot
            const int32_t row = wid[li];
            const float dot = acc[rb][r];
            const float nc = a.nrm2[row];
            const uint64_t key = dist_to_key(distance_from(a.metric, dot, qn, nc));
            if (!row_is_dead(nc) && (key < tk || (key == tk && row < tr))) {
                const int slot = atomicAdd(&a.st.cnt[q], 1);
                if (slot < a.cap) {
                    a.cand_row[(int64_t)q * a.cap + slot] = row;
                    a.cand_val[(int64_t)q * a.cap + slot] = dot;
                }
            }
        }
}

}  // namespace mi355
