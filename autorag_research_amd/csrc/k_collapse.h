// k_collapse.h -- at most `cap` entries per source in a ranked list.
//
// One workgroup of 256 threads per list walks the rule in include/mi355dr.h ("source-capped lists and search") without
// walking: the list's w (value, id) entries stay where they are, and only their keys -- keys[id], the source of an entry -- go
// into LDS, as (key, position) with the has-no-key bit in the position word.  One bitonic sort by (has a key first, key asc,
// position asc) puts the entries of a source side by side in list order, so the entry at sorted index i is struck iff it has
// a key, i >= cap, and the entry at i - cap has the same key: runs are contiguous, and every keyed entry stands in front of
// every entry without one.  The verdicts go back by position into one flag byte per slot, a block-wide prefix sum over the
// flags gives every kept entry its output slot, and the values are copied as the 64 bits they came with.  Plain sort kernel:
// no communication between workgroups, no global atomics, every loop bounded by the padded width np <= kSortMax.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kCollapseThreads = 256;
constexpr uint32_t kCollapseNoKey = 0x80000000u;  // in the position word: the entry has no key (it sorts behind every key)
constexpr unsigned char kCollapseEntry = 2, kCollapseKept = 1;  // a slot's flag byte

inline int collapse_pow2(int64_t n) {  // next_pow2 for the host's sizing
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// key[np] int64 | position[np] uint32 | the scan's 256 partial sums | flag[np] bytes
__host__ __device__ inline size_t collapse_lds_bytes(int np) {
    return (size_t)np * (sizeof(int64_t) + sizeof(uint32_t) + 1) + kCollapseThreads * sizeof(int32_t);
}

// (has a key first, key asc, position asc); positions are distinct, so no two entries compare equal
__device__ __forceinline__ bool collapse_before(int64_t k1, uint32_t p1, int64_t k2, uint32_t p2) {
    const uint32_t n1 = p1 & kCollapseNoKey, n2 = p2 & kCollapseNoKey;
    if (n1 != n2) return n1 < n2;
    return k1 < k2 || (k1 == k2 && p1 < p2);
}
__device__ __forceinline__ void bitonic_asc_collapse(int64_t* key, uint32_t* pos, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int p = i ^ j;
                if (p > i) {
                    const bool asc = ((i & k) == 0);
                    const int64_t ka = key[i], kb = key[p];
                    const uint32_t pa = pos[i], pb = pos[p];
                    if (asc ? collapse_before(kb, pb, ka, pa) : collapse_before(ka, pa, kb, pb)) {
                        key[i] = kb;
                        key[p] = ka;
                        pos[i] = pb;
                        pos[p] = pa;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// the key of an entry with id `id` (>= 0), *has = false when it has none
__device__ __forceinline__ int64_t collapse_key_of(const int64_t* __restrict__ keys, int64_t keys_len, int64_t id, bool* has) {
    int64_t key = -1;
    if (keys && id < keys_len) key = keys[id];
    *has = key >= 0;
    return key;
}

// grid: one workgroup per list.  vals / ids: [gridDim.x, w], list s of the launch.  lines: null, or [gridDim.x] -- list s
// writes line lines[s] of every output instead of line s (the re-searched queries of a block, k_gather_queries' map).  np: the
// padded width the launch's LDS was sized for, a power of two >= w.  out_vals / out_ids: [lines, k_out]; out_keys / out_pos
// [lines, k_out] and out_count / out_entries [lines]: each may be null.
__global__ __launch_bounds__(kCollapseThreads) void k_collapse_lists(const uint64_t* __restrict__ vals, const int64_t* __restrict__ ids,
                                                                     int w, int np, const int32_t* __restrict__ lines,
                                                                     const int64_t* __restrict__ keys, int64_t keys_len, int cap,
                                                                     int k_out, uint64_t* __restrict__ out_vals,
                                                                     int64_t* __restrict__ out_ids, int64_t* __restrict__ out_keys,
                                                                     int32_t* __restrict__ out_pos, int32_t* __restrict__ out_count,
                                                                     int32_t* __restrict__ out_entries) {
    extern __shared__ __align__(16) unsigned char collapse_smem[];
    const int tid = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x;
    const int64_t line = lines ? (int64_t)lines[s] : s;
    int64_t* key = (int64_t*)collapse_smem;
    uint32_t* pos = (uint32_t*)(key + np);
    int32_t* part = (int32_t*)(pos + np);
    unsigned char* flag = (unsigned char*)(part + kCollapseThreads);
    const uint64_t* lv = vals + s * w;
    const int64_t* li = ids + s * w;

    // ---- 1: (key, position) per slot; a slot without an id is no entry and, like an entry without a key, sorts last
    for (int i = tid; i < np; i += kCollapseThreads) {
        const int64_t id = i < w ? li[i] : -1;
        bool has = false;
        int64_t k = 0;
        if (id >= 0) k = collapse_key_of(keys, keys_len, id, &has);
        key[i] = has ? k : 0;
        pos[i] = (uint32_t)i | (has ? 0u : kCollapseNoKey);
        flag[i] = id >= 0 ? (kCollapseEntry | kCollapseKept) : 0;
    }
    __syncthreads();
    // ---- 2: the entries of a key side by side, in list order
    bitonic_asc_collapse(key, pos, np);
    // ---- 3: the cap-th predecessor has my key: struck (every slot in front of a keyed one is keyed)
    for (int i = tid; i < np; i += kCollapseThreads) {
        const uint32_t p = pos[i];
        if (!(p & kCollapseNoKey) && i >= cap && key[i - cap] == key[i]) flag[p] = kCollapseEntry;
    }
    __syncthreads();
    // ---- 4: prefix sum over positions, per thread a run of `per` slots: kept in the low half, entries in the high half
    const int per = np >= kCollapseThreads ? np / kCollapseThreads : 1;
    const int i0 = tid * per;
    int32_t mine = 0;
    if (i0 < np)
        for (int j = 0; j < per; ++j) {
            const unsigned f = flag[i0 + j];
            mine += (int32_t)(f & kCollapseKept) + ((int32_t)(f >> 1) << 16);
        }
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kCollapseThreads; d <<= 1) {
        const int32_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const int32_t total = part[kCollapseThreads - 1];
    const int kept = total & 0xFFFF, entries = total >> 16;
    // ---- 5: the first k_out kept entries in list order, with the bits they came with; NaN / -1 behind them
    uint64_t* ov = out_vals + line * k_out;
    int64_t* oi = out_ids + line * k_out;
    int64_t* ok = out_keys ? out_keys + line * k_out : nullptr;
    int32_t* op = out_pos ? out_pos + line * k_out : nullptr;
    if (i0 < np) {
        int slot = (part[tid] - mine) & 0xFFFF;
        for (int j = 0; j < per && slot < k_out; ++j) {
            const int i = i0 + j;
            if (!(flag[i] & kCollapseKept)) continue;
            const int64_t id = li[i];  // (a kept slot is an entry: i < w)
            ov[slot] = lv[i];
            oi[slot] = id;
            if (ok) {
                bool has = false;
                const int64_t k = collapse_key_of(keys, keys_len, id, &has);
                ok[slot] = has ? k : -1;
            }
            if (op) op[slot] = i;
            ++slot;
        }
    }
    for (int t = kept + tid; t < k_out; t += kCollapseThreads) {
        ov[t] = 0x7FF8000000000000ull;
        oi[t] = -1;
        if (ok) ok[t] = -1;
        if (op) op[t] = -1;
    }
    if (tid == 0) {
        if (out_count) out_count[line] = kept;
        if (out_entries) out_entries[line] = entries;
    }
}

}  // namespace mi355
