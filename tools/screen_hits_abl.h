// tools/screen_hits_abl.h -- the A/B forms of the hit paths in csrc/screen_hits.h, for the timing builds of tools/screen_ab.hip
// (tools/k_screen256c_abl.h, tools/k_screen_rq_abl.h).  Measured and not adopted: the library launches none of them, and its
// headers carry only the forms it runs.  Each form keeps its verdict in its comment.
#pragma once
#include "screen_hits.h"

namespace mi355 {

// k_screen256c ABL bit 12: the append path INLINE at every test site but marked unlikely, so that block placement moves the
// twelve copies behind the loop -- no call, no argument moves, and above all no function entry: the calling convention opens
// every device function with s_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0), which makes a wave with a hit wait for every LDS-DMA
// piece it has in flight.  (The block test is screen_test_block's.)
template <bool I8>
__device__ __forceinline__ void screen_test_block_cold(int* status, f32x16 acc, int q, int rbase, int row_end, float th, I8Blk blk,
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
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(any) != 0, 0))
        que_n = screen_queue_hits_body<I8>(acc, any ? 1 : 0, q, rbase, row_end, th, blk.m, blk.ek, lds_addr(que), que_n, status);
}

// k_screen_rq ABL bits 8, 9 = MODE of the hit-lane queue's test: 0 = the library's (the stores behind a wave-uniform branch),
// 1 = bookkeeping without the stores, 2 = BRANCH-FREE: the five stores always issued under EXEC = hit lanes (uniform cost for
// every wave; measured +15 % with the thresholds parked: stores under an empty EXEC are not free -- not adopted), 3 = as 0 with
// the block laid out as the FALL-THROUGH path -- the common case takes one short forward branch over it and a hit never leaves
// the loop's code for a cold block at the kernel's end and back.
template <bool I8, int MODE>
__device__ __forceinline__ void screen_test_block_lq_max_abl(const ScreenArgs& a, int row_end, f32x16 acc, int gmax, int q, int rbase,
                                                             float th, I8Blk blk, unsigned lq_addr, int& lq_n, int& lq_ovf) {
    if constexpr (MODE == 0) {
        screen_test_block_lq_max<I8>(a, row_end, acc, gmax, q, rbase, th, blk, lq_addr, lq_n);
        return;
    }
    bool any;
    if constexpr (I8) any = i8_value(gmax, blk) >= th;
    else any = __int_as_float(gmax) >= th;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(any);
    const int n = __builtin_popcountll(bal);
    const i32x16 v = __builtin_bit_cast(i32x16, acc);
    if constexpr (MODE == 3) {
        if (__builtin_expect(bal != 0, 1)) {  // wave-uniform, rare
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
        return;
    }
    // does the block's hit lanes fit?  (Never false in practice -- see kLaneQueueFlushAt.)  If not, nothing is stored and the
    // wave remembers it in `lq_ovf`: at the next tile start it flags its 32 queries kStOverflow (the host re-screens them).
    const bool fits = lq_n + n <= kLaneQueueCap;
    const unsigned long long mask = fits ? bal : 0ull;   // s_cselect: no branch
    lq_ovf |= fits ? 0 : 1;
    const unsigned e = (unsigned)lq_n + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
    if constexpr (MODE == 2) {
        const unsigned addr = lq_addr + (e << 6), addr_m = lq_addr + (unsigned)(kLaneQueueCap * 64) + (e << 4);
        const i32x4 meta{q, rbase, (int)__float_as_uint(blk.m), (int)__float_as_uint(blk.ek)};
        unsigned long long saved;
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_and_b64 exec, exec, %[mask]\n\t"
            "ds_write_b128 %[ad], %[v0]\n\t"
            "ds_write_b128 %[ad], %[v1] offset:16\n\t"
            "ds_write_b128 %[ad], %[v2] offset:32\n\t"
            "ds_write_b128 %[ad], %[v3] offset:48\n\t"
            "ds_write_b128 %[am], %[mt]\n\t"
            "s_mov_b64 exec, %[sv]"
            : [sv] "=&s"(saved)
            : [mask] "s"(mask), [ad] "v"(addr), [am] "v"(addr_m), [v0] "v"(i32x4{v[0], v[1], v[2], v[3]}),
              [v1] "v"(i32x4{v[4], v[5], v[6], v[7]}), [v2] "v"(i32x4{v[8], v[9], v[10], v[11]}),
              [v3] "v"(i32x4{v[12], v[13], v[14], v[15]}), [mt] "v"(meta)
            : "memory");
    }
    lq_n += fits ? n : 0;
}
// ... the same with the maximum taken here, in one piece
template <bool I8, int MODE>
__device__ __forceinline__ void screen_test_block_lq_abl(const ScreenArgs& a, int row_end, f32x16 acc, int q, int rbase, float th,
                                                         I8Blk blk, unsigned lq_addr, int& lq_n, int& lq_ovf) {
    int g = screen_block_max_part<I8, 0>(acc, 0);
    g = screen_block_max_part<I8, 1>(acc, g);
    g = screen_block_max_part<I8, 2>(acc, g);
    g = screen_block_max_part<I8, 3>(acc, g);
    screen_test_block_lq_max_abl<I8, MODE>(a, row_end, acc, g, q, rbase, th, blk, lq_addr, lq_n, lq_ovf);
}

}  // namespace mi355
