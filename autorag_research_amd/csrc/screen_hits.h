// screen_hits.h -- the hit paths of the screen kernels: what happens to the values of one 32 x 32 accumulator block that
// pass their query's threshold.  Three forms, one section each, and every function here is reached from a library kernel:
//   1. the direct append        k_screen, k_screen_stream   one returning global atomic per lane with hits, in the epilogue
//   2. the per-wave queue       k_screen256c                (query, row, value) entries in LDS, appended out of line
//   3. the hit-lane queue       k_screen_rq                 a hit lane's sixteen accumulators in LDS, five stores, no call
// Forms 2 and 3 exist because their kernels test INSIDE a persistent loop with LDS-DMA in flight, where a returning vector-memory
// instruction waits for the whole prefetch (vmcnt completes in order).  The forms that were measured and not adopted (the
// append inline at every test site, the branch-free stores, ...) live with the timing builds: tools/screen_hits_abl.h.
// C/D layout of a block throughout: column (query) = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) for register r;
// rbase = first row of the block + 4 * (lane >> 5).
#pragma once
#include "screen_common.h"

namespace mi355 {

// ==== 1. The direct append (k_screen, k_screen_stream: the test runs once per tile, behind the K loop) =========================

// Fused epilogue of one 32x32 accumulator block, shared by both kernels.
template <bool I8>
__device__ __forceinline__ void screen_emit_block(const ScreenArgs& a, f32x16 acc, int q, int64_t rbase, float th,
                                                  I8Blk blk) {
    // fast path (almost always): one max over the lane's 16 rows and one compare
    bool any;
    if constexpr (I8) {
        const i32x16 v = __builtin_bit_cast(i32x16, acc);
        int m = v[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) m = max(m, v[r]);
        any = i8_value(m, blk) >= th;
    } else {
        float m = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[r]);
        any = m >= th;
    }
    if (!any) return;
    // hit path: collect the lane's hits in a mask, reserve all their slots with ONE atomic, then store.
    // (int8: rows outside the int8 shadow may show up here with a stale 0 -- k_prune drops them.)
    unsigned mask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = rbase + (r & 3) + 8 * (r >> 2);
        bool hit;
        if constexpr (I8) hit = i8_value(__builtin_bit_cast(i32x16, acc)[r], blk) >= th;
        else hit = acc[r] >= th;
        if (hit && row < a.row_end) mask |= 1u << r;
    }
    if (mask == 0) return;
    int slot = atomicAdd(&a.cnt[q], __builtin_popcount(mask));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if ((mask >> r) & 1u) {
            if (slot < a.cap) {
                float val;
                if constexpr (I8) val = i8_value(__builtin_bit_cast(i32x16, acc)[r], blk);
                else val = acc[r];
                a.cand_row[(int64_t)q * a.cap + slot] = (int32_t)(rbase + (r & 3) + 8 * (r >> 2));
                a.cand_val[(int64_t)q * a.cap + slot] = val;
            }
            ++slot;
        }
    }
}

// first chunk: every (query,row) becomes a candidate at slot row-row0 (counts are set by the host)
template <bool I8>
__device__ __forceinline__ void screen_emit_all_block(const ScreenArgs& a, f32x16 acc, int q, int64_t rbase, I8Blk blk) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = rbase + (r & 3) + 8 * (r >> 2);
        if (row < a.row_end) {
            float val;
            if constexpr (I8) {
                val = a.flag8[row] ? __builtin_nanf("") : i8_value(__builtin_bit_cast(i32x16, acc)[r], blk);
            } else {
                val = acc[r];
            }
            a.cand_row[(int64_t)q * a.cap + (row - a.row0)] = (int32_t)row;
            a.cand_val[(int64_t)q * a.cap + (row - a.row0)] = val;
        }
    }
}

// Starter (run_screen: "sampled threshold estimator"; k_screen only): the wave's 64 rows x 64 queries sub-tile -> for each of
// its queries the LARGEST value over the 64 rows and its row, stored at slot (slab index) of the query's list: no thresholds,
// no atomics, S / 64 candidates per query from a sample of S rows.  The exact re-score of the best of them (k_prune,
// thr_only) gives a first threshold that is valid whatever the sample missed: any k exact scores bound the k-th best
// from below.  int8: v = fma((float)acc, m, ek) is monotone in acc (m >= 0), so a block's largest value comes from its
// largest accumulator.  acc[i] = the two row blocks of query block j.
template <bool I8>
__device__ __forceinline__ void screen_emit_slab_max(const ScreenArgs& a, const f32x16 (&acc)[2], int q, int64_t slab_row0,
                                                     int lane, const I8Blk (&blk)[2]) {
    float best = -__builtin_inff();
    int64_t best_row = slab_row0;
    if (a.moments != nullptr) {  // wave-uniform: a speculative pass's sample moments (no atomics: one writer per query and slab)
        // sum and sum of squares of the screen's ESTIMATE of the similarity, over the slab's rows below row_end: the bf16 value
        // itself; int8: S_q S_g acc WITHOUT the group's share e_g kq of the bound, which the compared value carries on top.  The
        // model threshold is verified against exact similarities (k_finalize), so it has to be predicted in their units: with
        // e_g kq left in (0.28 of a standard deviation at d = 768) the prediction sits that much too high, and a sixth of the
        // headline's queries missed.  NaN images (bf16, irregular rows) are left out; stale zeros of rows outside the int8
        // shadow stay in: nothing rigorous reads this
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t rb = slab_row0 + 32 * i + 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v;
                if constexpr (I8) v = (float)__builtin_bit_cast(i32x16, acc[i])[r] * blk[i].m;
                else v = acc[i][r];
                if (rb + (r & 3) + 8 * (r >> 2) < a.row_end && v == v) {
                    s1 += v;
                    s2 = __builtin_fmaf(v, v, s2);
                }
            }
        }
        s1 += __shfl_xor(s1, 32, kWave);
        s2 += __shfl_xor(s2, 32, kWave);
        if (lane < 32) {
            const int64_t slot = (slab_row0 - a.row0) / kSlabRows;
            if (slot < a.moment_slabs) {
                float* mo = a.moments + ((int64_t)q * a.moment_slabs + slot) * 2;
                mo[0] = s1;
                mo[1] = s2;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t rbase = slab_row0 + 32 * i + 4 * (lane >> 5);
        int br = 0;
        float bv;
        if constexpr (I8) {
            const i32x16 v = __builtin_bit_cast(i32x16, acc[i]);
            int m = v[0];
#pragma unroll
            for (int r = 1; r < 16; ++r)
                if (v[r] > m) {
                    m = v[r];
                    br = r;
                }
            bv = i8_value(m, blk[i]);
        } else {
            float m = acc[i][0];
            if (!(m == m)) m = -__builtin_inff();  // (NaN image of an irregular row: never a maximum)
#pragma unroll
            for (int r = 1; r < 16; ++r)
                if (acc[i][r] > m) {
                    m = acc[i][r];
                    br = r;
                }
            bv = m;
        }
        const int64_t row = rbase + (br & 3) + 8 * (br >> 2);
        if (row < a.row_end && bv > best) {
            best = bv;
            best_row = row;
        }
    }
    // the other half of the wave holds the other 32 rows of the same query column
    const float ov = __shfl_xor(best, 32, kWave);
    const int orow = __shfl_xor((int)best_row, 32, kWave);
    if (ov > best || (ov == best && orow < (int)best_row)) {
        best = ov;
        best_row = orow;
    }
    if (lane < 32) {
        const int64_t slot = (slab_row0 - a.row0) / kSlabRows;
        a.cand_row[(int64_t)q * a.cap + slot] = (int32_t)best_row;
        a.cand_val[(int64_t)q * a.cap + slot] = best;
    }
}

// ==== 2. The per-wave candidate queue (k_screen256c) ==========================================================================
// Hits are appended with wave-level bookkeeping only (ballot + mbcnt, count in an SGPR): no atomics, and no
// vector-memory instruction, so the in-flight LDS-DMA prefetch of the next tile is never waited for (vmcnt
// completes in order: waiting for a global atomic's return would wait for the whole prefetch).  A wave flushes its
// queue to the global candidate lists between two tiles when it is more than half full, and when the workgroup is done.
constexpr int kWaveQueueCap = 320;  // entries (q, row, value) per wave; 8 waves x 320 x 12 B = 30 KiB

// flush a wave's queue: one global atomic per entry.  Inlined at ONE site per tile -- a call would make the register
// allocator spill the accumulators around it.
__device__ __forceinline__ void wave_queue_flush(const ScreenArgs& a, const int32_t* que, int n) {
    const int lane = threadIdx.x & 63;
    for (int e = lane; e < n; e += kWave) {
        const int q = que[e];
        const int slot = atomicAdd(&a.cnt[q], 1);
        if (slot < a.cap) {
            a.cand_row[(int64_t)q * a.cap + slot] = que[kWaveQueueCap + e];
            a.cand_val[(int64_t)q * a.cap + slot] = __int_as_float(que[2 * kWaveQueueCap + e]);
        }
    }
}

// The append path, OUT OF LINE: one copy per kernel instead of one per test site.  Inlined at the 12 test sites of the kernel's
// K-step it made the loop body ~60 KB of code -- the hot path hopping over a dozen cold blocks, more than the instruction cache
// holds -- and cost 20 % of the kernel although it almost never runs.  A call spills the caller's live registers around the
// call site only, i.e. on the rare path.  Returns the wave's new queue fill.
// A hit costs the whole workgroup this traversal (the other waves wait at the next K-step barrier), so it is kept short: one
// compare + one scalar branch per group of four accumulator registers (int8: against the block's integer threshold, the
// conservative image of the caller's float test), then per register of a group with a hit; the row bound is only tested in the
// hit branch (rows past row_end exist in the last tile of a chunk only, and their values are finite garbage at worst).
// The queue is written with inline-asm LDS stores on purpose: for compiler-visible LDS accesses the waitcnt insertion assumes
// they may alias the in-flight LDS-DMA and puts s_waitcnt vmcnt(0) in front (tests/test_build_pipeline.py checks the generated
// code).  No wait after the stores: LDS operations of one wave execute in order, the flush's reads come later in the same wave.
template <bool I8>
__device__ __forceinline__ int screen_queue_hits_body(f32x16 acc, int any_i, int q, int rbase, int row_end, float th,
                                                     float m, float ek, unsigned a_q, int que_n, int* status) {
    const bool any = any_i != 0;
    bool gany[4];
    int thi = 0;
    if constexpr (I8) {
        const i32x16 v = __builtin_bit_cast(i32x16, acc);
        thi = i8_block_threshold(th, m, ek);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            gany[i] = any && max(max(v[4 * i], v[4 * i + 1]), max(v[4 * i + 2], v[4 * i + 3])) >= thi;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            gany[i] = fmaxf(fmaxf(acc[4 * i], acc[4 * i + 1]), fmaxf(acc[4 * i + 2], acc[4 * i + 3])) >= th;
    }
    const unsigned a_r = a_q + 4u * kWaveQueueCap, a_v = a_q + 8u * kWaveQueueCap;
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
        if (__builtin_amdgcn_ballot_w64(gany[gi]) == 0) continue;  // wave-uniform: no hit in this group of four
#pragma unroll
        for (int ri = 0; ri < 4; ++ri) {
            const int r = 4 * gi + ri;
            bool hit;
            if constexpr (I8) hit = any && __builtin_bit_cast(i32x16, acc)[r] >= thi;
            else hit = acc[r] >= th;
            if (__builtin_amdgcn_ballot_w64(hit) == 0) continue;  // wave-uniform
            const int row = rbase + (r & 3) + 8 * (r >> 2);
            hit = hit && row < row_end;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
            if (hit) {
                const unsigned e = (unsigned)que_n +
                                   __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
                float val;
                if constexpr (I8) val = __builtin_fmaf((float)__builtin_bit_cast(i32x16, acc)[r], m, ek);
                else val = acc[r];
                if (e < (unsigned)kWaveQueueCap) {
                    asm volatile("ds_write_b32 %0, %1" ::"v"(a_q + 4u * e), "v"(q) : "memory");
                    asm volatile("ds_write_b32 %0, %1" ::"v"(a_r + 4u * e), "v"(row) : "memory");
                    asm volatile("ds_write_b32 %0, %1" ::"v"(a_v + 4u * e), "v"(val) : "memory");
                } else {  // queue full: the query is re-screened by the host
                    __hip_atomic_fetch_or(&status[q], kStOverflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            que_n += __builtin_popcountll(bal);  // may run past the capacity: the flush clamps
        }
    }
    return que_n;
}
// (the body is a function of its own for the form that inlines it at every test site: tools/screen_hits_abl.h)
template <bool I8>
__device__ __attribute__((noinline)) int screen_queue_hits(f32x16 acc, int any_i, int q, int rbase, int row_end, float th,
                                                            float m, float ek, unsigned a_q, int que_n, int* status) {
    return screen_queue_hits_body<I8>(acc, any_i, q, rbase, row_end, th, m, ek, a_q, que_n, status);
}
// the test itself, inline: 15 max + the compare; the call only when some lane passes
template <bool I8>
__device__ __forceinline__ void screen_test_block(int* status, f32x16 acc, int q, int rbase, int row_end, float th, I8Blk blk,
                                                  int32_t* que, int& que_n) {
    bool any;
    if constexpr (I8) {
        const i32x16 v = __builtin_bit_cast(i32x16, acc);
        int g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = max(max(v[4 * i], v[4 * i + 1]), max(v[4 * i + 2], v[4 * i + 3]));
        any = i8_value(max(max(g[0], g[1]), max(g[2], g[3])), blk) >= th;
    } else {
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = fmaxf(fmaxf(acc[4 * i], acc[4 * i + 1]), fmaxf(acc[4 * i + 2], acc[4 * i + 3]));
        any = fmaxf(fmaxf(g[0], g[1]), fmaxf(g[2], g[3])) >= th;
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0) return;  // wave-uniform: almost always taken
    que_n = screen_queue_hits<I8>(acc, any ? 1 : 0, q, rbase, row_end, th, blk.m, blk.ek, lds_addr(que), que_n, status);
}

// ==== 3. The queue of hit lanes (k_screen_rq; round 5) ========================================================================
// What a hit cost before (tools/screen_ab THRZ, profiles/r05_hit_path.txt): the out-of-line append is entered through the
// calling convention's `s_waitcnt vmcnt(0)` -- the wave waits for every LDS-DMA piece it has in flight, the youngest issued a
// few hundred cycles earlier -- and then walks its sixteen registers with a scalar branch each, while the other seven waves of
// the workgroup wait at the next K-step barrier: 0.22 ns per hit chip-wide in a hit-dense chunk (3 hits per block), 0.67 ns
// in the last chunks (one hit per ten blocks: one call per hit) -- ~0.55 ms of a 6.9 ms pass at N = 10 M.
// Now a block with a hit costs the hot loop five LDS stores and no call: every lane whose float test passed writes ITS OWN
// sixteen accumulators + (query, first row, m, ek) -- 80 bytes -- to entry `rank` of the wave's queue (ballot + mbcnt; inline
// asm stores, no vector memory, no wait).  The queue is expanded into candidates at a tile's start once it holds more than 24
// entries, and at the kernel's end: one LANE per entry, all entries in parallel.
constexpr int kLaneQueueCap = 64;          // entries per wave: a block's hit lanes always fit an empty queue (one lane = one entry at the flush)
constexpr int kLaneQueueEntryBytes = 80;   // 16 accumulators (64 B, entry e at 64 e) + (q, rbase, m, ek) (16 B, at 64 cap + 16 e)
constexpr int kLaneQueueBytes = kLaneQueueCap * kLaneQueueEntryBytes;  // 5 KiB per wave
constexpr int kLaneQueueFlushAt = 24;

__device__ __forceinline__ void lds_store16(unsigned addr, i32x4 v) {
    asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}

// entry `lane` of the wave's queue as both flushes read it: where its sixteen accumulators are, its (query, first row, m, ek)
// and the thresholds its values are tested against again (int8: the block's integer threshold)
struct LaneQueueEntry {
    const __attribute__((address_space(3))) int* acc;
    int q, rbase;
    float m, ek, th;
    int thi;
};
template <bool I8>
__device__ __forceinline__ LaneQueueEntry lane_queue_entry(const ScreenArgs& a, unsigned lq_addr, int lane) {
    const __attribute__((address_space(3))) int* e =
        (const __attribute__((address_space(3))) int*)(unsigned long)(lq_addr + (unsigned)lane * 64u);
    const __attribute__((address_space(3))) int* em =
        (const __attribute__((address_space(3))) int*)(unsigned long)(lq_addr + (unsigned)(kLaneQueueCap * 64) + (unsigned)lane * 16u);
    const int q = em[0], rbase = em[1];
    const float m = __int_as_float(em[2]), ek = __int_as_float(em[3]);
    const float th = a.thr[q];
    int thi = 0;
    if constexpr (I8) thi = i8_block_threshold(th, m, ek);
    return LaneQueueEntry{e, q, rbase, m, ek, th, thi};
}

// expand entries [0, n) of the wave's lane queue into the global candidate lists (lane e = entry e).  INLINED at one site per
// tile (a call there made the allocator park query fragments in scratch and reload them inside the hot loop; at a tile's
// start two accumulator blocks are dead, which is the room this body lives in).  The caller has waited for its LDS-DMA before.
template <bool I8>
__device__ __forceinline__ void lane_queue_flush(const ScreenArgs& a, unsigned lq_addr, int n, int row_end) {
    const int lane = threadIdx.x & 63;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the entries were written with inline-asm stores the compiler does not track)
    if (lane < n) {
        const LaneQueueEntry t = lane_queue_entry<I8>(a, lq_addr, lane);
        // sixteen values in four 16-byte reads, ONE returning atomic per entry (it reserves the slots of all its hits: the
        // atomic's round trip is the flush's longest step), then the stores
        typedef __attribute__((address_space(3))) const i32x4 lds_i32x4;
        i32x4 w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = ((lds_i32x4*)t.acc)[i];
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int v = w[r >> 2][r & 3];
            bool hit;
            if constexpr (I8) hit = v >= t.thi;
            else hit = __int_as_float(v) >= t.th;
            if (hit && t.rbase + (r & 3) + 8 * (r >> 2) < row_end) mask |= 1u << r;
        }
        if (mask != 0) {
            int slot = atomicAdd(&a.cnt[t.q], (int)__builtin_popcount(mask));
            int32_t* const cr = a.cand_row + (int64_t)t.q * a.cap;
            float* const cv = a.cand_val + (int64_t)t.q * a.cap;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if ((mask >> r) & 1u) {
                    if (slot < a.cap) {
                        const int v = w[r >> 2][r & 3];
                        cr[slot] = t.rbase + (r & 3) + 8 * (r >> 2);
                        cv[slot] = I8 ? __builtin_fmaf((float)v, t.m, t.ek) : __int_as_float(v);
                    }
                    ++slot;
                }
            }
        }
    }
}

// The same expansion with a small register footprint (the sixteen values read back one at a time in a rolled loop, one atomic
// per hit): for the test sites, where every accumulator is live and the unrolled body above would spill.  It runs when a
// block's hit lanes do not fit the queue any more -- the queue is flushed at a tile's start whenever it holds more than
// kLaneQueueFlushAt entries, so ONE tile has to bring more than 64 - 24 hit lanes to one wave: thresholds still loose (small k
// over few rows, the chunks right behind an emit-all ladder) or a burst of near-duplicate rows.
template <bool I8>
__device__ __forceinline__ void lane_queue_flush_small(const ScreenArgs& a, unsigned lq_addr, int n, int row_end) {
    const int lane = threadIdx.x & 63;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < n) {
        const LaneQueueEntry t = lane_queue_entry<I8>(a, lq_addr, lane);
#pragma unroll 1
        for (int r = 0; r < 16; ++r) {
            const int v = t.acc[r];
            bool hit;
            if constexpr (I8) hit = v >= t.thi;
            else hit = __int_as_float(v) >= t.th;
            const int row = t.rbase + (r & 3) + 8 * (r >> 2);
            if (hit && row < row_end) {
                const int slot = atomicAdd(&a.cnt[t.q], 1);
                if (slot < a.cap) {
                    a.cand_row[(int64_t)t.q * a.cap + slot] = row;
                    a.cand_val[(int64_t)t.q * a.cap + slot] = I8 ? __builtin_fmaf((float)v, t.m, t.ek) : __int_as_float(v);
                }
            }
        }
    }
}

// The block's largest value, in four PARTS of two v_max3 each (k_screen_rq issues one part behind each of four MFMAs: a test in
// one piece is ~14 dependent vector instructions during which its wave feeds the matrix pipe nothing -- and the other wave of
// the SIMD, in lockstep behind the same barriers, is at its own test).  `g` = the running maximum (int32 bits / float bits).
// (Written as chains on purpose; screen_test_block's 4 x 4 tree is the other kernel's form.)
template <bool I8, int PART>
__device__ __forceinline__ int screen_block_max_part(const f32x16& acc, int g) {
    if constexpr (I8) {
        const i32x16 v = __builtin_bit_cast(i32x16, acc);
        if constexpr (PART == 0) return max(max(max(v[0], v[1]), v[2]), v[3]);
        else return max(max(max(max(g, v[4 * PART]), v[4 * PART + 1]), v[4 * PART + 2]), v[4 * PART + 3]);  // two v_max3_i32
    } else {
        if constexpr (PART == 0) return __float_as_int(fmaxf(fmaxf(fmaxf(acc[0], acc[1]), acc[2]), acc[3]));
        else return __float_as_int(fmaxf(fmaxf(fmaxf(fmaxf(__int_as_float(g), acc[4 * PART]), acc[4 * PART + 1]), acc[4 * PART + 2]), acc[4 * PART + 3]));
    }
}

// the test of one 32 x 32 block, given its largest value, + the enqueue of its hit lanes: the five stores behind a wave-uniform
// branch.  `lq_n` = entries in the wave's queue (wave-uniform).
// What a hit costs is NOT its instructions but the barrier: the eight waves of a workgroup meet every K-step, so whatever delays
// ONE wave -- even a taken branch alone, measured -- is paid by all eight, and with one hit per 3 ... 30 blocks some wave of the
// eight has one at most test sites (profiles/r05_hit_path.txt: this queue behind a branch costs the same as the out-of-line
// append it replaced; k_screen_rq's answer is its hand-over schedule -- all tests of a tile between two barriers).
template <bool I8>
__device__ __forceinline__ void screen_test_block_lq_max(const ScreenArgs& a, int row_end, f32x16 acc, int gmax, int q, int rbase, float th,
                                                         I8Blk blk, unsigned lq_addr, int& lq_n) {
    bool any;
    if constexpr (I8) any = i8_value(gmax, blk) >= th;
    else any = __int_as_float(gmax) >= th;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(any);
    const int n = __builtin_popcountll(bal);
    const i32x16 v = __builtin_bit_cast(i32x16, acc);
    if (__builtin_expect(bal != 0, 0)) {  // wave-uniform, rare
        if (__builtin_expect(lq_n + n > kLaneQueueCap, 0)) {  // a burst the per-tile flush did not foresee: make room now
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            lane_queue_flush_small<I8>(a, lq_addr, lq_n, row_end);
            lq_n = 0;
        }
        if (any) {
            const unsigned e = (unsigned)lq_n + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
            const unsigned addr = lq_addr + (e << 6);
#pragma unroll
            for (int i = 0; i < 4; ++i) lds_store16(addr + 16u * i, i32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]});
            lds_store16(lq_addr + (unsigned)(kLaneQueueCap * 64) + (e << 4), i32x4{q, rbase, (int)__float_as_uint(blk.m), (int)__float_as_uint(blk.ek)});
        }
        lq_n += n;
    }
}
// ... the same with the maximum taken here, in one piece (k_screen_rq with its split tests off)
template <bool I8>
__device__ __forceinline__ void screen_test_block_lq(const ScreenArgs& a, int row_end, f32x16 acc, int q, int rbase, float th, I8Blk blk,
                                                     unsigned lq_addr, int& lq_n) {
    int g = screen_block_max_part<I8, 0>(acc, 0);
    g = screen_block_max_part<I8, 1>(acc, g);
    g = screen_block_max_part<I8, 2>(acc, g);
    g = screen_block_max_part<I8, 3>(acc, g);
    screen_test_block_lq_max<I8>(a, row_end, acc, g, q, rbase, th, blk, lq_addr, lq_n);
}

}  // namespace mi355
