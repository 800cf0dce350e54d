// index.h -- the opaque handle behind mi355dr_index and the host-side error helpers (internal).
#pragma once
#include <climits>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "dev_common.h"
#include "mi355dr.h"

namespace mi355 {
// Owner of one device allocation (Pinned: of one pinned host allocation), released on destruction.  Kernels and copies take the
// raw pointer, `p` (or the buffer itself: it converts).  grow() gets the new block BEFORE it lets go of the old one: when it
// fails, the buffer is what it was -- still valid, still its old size.  The old contents are not carried over.
template <class T, bool Pinned = false>
struct DevBuf {
    T* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }
    hipError_t grow(size_t want) {  // at least `want` bytes
        if (want <= bytes) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, want) : hipMalloc(&q, want);
        if (e != hipSuccess) return e;
        release();
        p = (T*)q;
        bytes = want;
        return hipSuccess;
    }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
    operator T*() const { return p; }
};
template <class T>
using HostBuf = DevBuf<T, true>;

// Owner of one HIP event, created on first use
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct EventPair {
    hipEvent_t a, b;
    int big;  // 1: the launch went to k_screen256c or k_screen_rq (the dominant kernel), 0: k_screen
};
// the timing pairs of option "profile": pooled (take_events) or behind a launch (drain_events), owned either way
struct EventPairs {
    std::vector<EventPair> v;
    ~EventPairs() {
        for (auto& p : v) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
    }
};
struct MultiVecStore;  // mi355dr_maxsim.hip
struct SparseStore;    // mi355dr_sparse.hip
// What one search pass has decided, once, before its first launch (mi355dr.hip decide_pass): every function of the pass takes
// it, or the field it needs, as a parameter -- none reads a decision from the handle
struct Pass {
    int k = 0;
    int level = 0;           // 0: a first attempt; 1 .. 3: the fix-up passes of complete_block (bf16 bound, slower chunk growth)
    bool screening = false;  // the pass screens; else the exact scan (path = scan, a forced scan, no screen that can serve)
    bool i8 = false;         // the screen's element type: int8, else bf16 (also what k_prep_queries quantises for)
    bool wide = false;       // its prunes take the two-wave form (screening passes at 33 <= k <= 128)
    int cap = 0;             // candidate slots per query = the lists' stride
    // one screen launch over all rows at a threshold the starter's sample PREDICTS, verified against the pass's own k-th best
    // (DESIGN.md 4.3): a first attempt that screens behind the starter, at a k with an admissible m(k), on a corpus of at least
    // spec_min_rows rows, with option "speculate" on and the index not on speculation probation
    bool speculative = false;
    bool spec_eligible = false;  // ... all of that but the probation
    int spec_m = 0;         // rows the model threshold expects above it (dev_common.h kSpecM)
    const char* refused = nullptr;  // not null: no pass may run, MI355DR_E_UNSUPPORTED with this text
};
// one block between enqueue_block() and complete_block() (mi355dr.hip)
struct Pending {
    bool active = false;
    Event done;
    HostBuf<int> status_host;     // pinned [kQBlockMax + 1]: the block's per-query status words + their OR
    hipStream_t stream = nullptr;
    const float* q_dev = nullptr; // the caller's queries (valid until the wait: a fix-up gathers from them)
    int B = 0;
    Pass pass;                    // what the block was enqueued under
    double* out_dist = nullptr;
    int64_t* out_rows = nullptr;
};
// buffers of the sub-block that the fix-ups of a level-L block search (complete_block grows all four before it uses one)
struct RetryBufs {
    DevBuf<float> q;       // [kQBlockMax, dim] queries being re-screened / re-scanned
    DevBuf<double> dist;   // [kQBlockMax, kKMax]
    DevBuf<int64_t> rows;
    DevBuf<int> map;       // [kQBlockMax] position of each sub-block query in its block
};
constexpr int kPendingRing = 4;

// ---- per-family scratch of the derived searches: plain owners, each grown by its reserve() at the start of a call (or block).
// A reserve() that fails leaves what it already grew: the buffers are only ever larger.  None of them stages results for the
// host (mi355dr_index::out_*_dev does), except the grouped search's [G, k], which is not block-shaped.
template <class... Bufs>
hipError_t grow_each(size_t n, Bufs&... bufs) {  // every buffer to at least n of ITS elements, in order, up to the first failure
    hipError_t e = hipSuccess;
    (void)(((e = bufs.grow(n * sizeof(*bufs.p))) == hipSuccess) && ...);
    return e;
}
// MMR (mi355dr_search_mmr / mi355dr_mmr_select): one block's candidate lists in the total order
// [nb, stride] and the kernel's pair counter
struct MmrBufs {
    DevBuf<double> cand_dist;
    DevBuf<int64_t> cand_rows;
    DevBuf<unsigned long long> pairs_dev;
    hipError_t reserve(size_t nb, size_t stride) {
        hipError_t e = grow_each(nb * stride, cand_dist, cand_rows);
        if (!e) e = grow_each(1, pairs_dev);
        return e;
    }
};
// grouped search (mi355dr_search_groups* / mi355dr_merge_groups_device): the call's group offsets
// [G + 1], the sub-queries' lists [S, fetch_k] and the host form's result staging [G, k] / [G] (k up to 4096, G unbounded:
// not block-shaped, so it grows here; the count is int32 as in the C ABI)
struct GroupBufs {
    DevBuf<int32_t> offsets, count;
    DevBuf<double> cand_dist, out_dist;
    DevBuf<int64_t> cand_rows, out_rows;
    hipError_t reserve(size_t G, size_t S, size_t fetch_k, size_t k, bool host) {  // (the merge alone: S = 0, host = false)
        hipError_t e = grow_each(G + 1, offsets);
        if (!e) e = grow_each(S * fetch_k, cand_dist, cand_rows);
        if (!e && host) e = grow_each(G * k, out_dist, out_rows);
        if (!e && host) e = grow_each(G, count);
        return e;
    }
};
// hybrid fusion (mi355dr_fuse_lists): the host form's staging -- both lists [B, w_l], their maps and
// the results [B, k_out] / [B] (B unbounded: not block-shaped, so it grows here).  The device form needs none of it
struct FuseBufs {
    DevBuf<double> vals[2], out_vals;
    DevBuf<int64_t> ids[2], map[2], out_ids;
    DevBuf<int32_t> count;
    hipError_t reserve(size_t B, const int* w, const int64_t* map_len, size_t k_out) {
        hipError_t e = hipSuccess;
        for (int l = 0; l < 2 && !e; ++l) {
            e = grow_each(B * (size_t)w[l], vals[l], ids[l]);
            if (!e) e = grow_each((size_t)map_len[l], map[l]);
        }
        if (!e) e = grow_each(B * k_out, out_vals, out_ids);
        if (!e) e = grow_each(B, count);
        return e;
    }
};
// source-capped lists and search (mi355dr_collapse_lists* / mi355dr_search_collapsed*).  The host list
// form's staging: the lists [B, w], the key table, the results [B, k_out] / [B] (B unbounded: not block-shaped, so it grows
// here).  The search forms' block state: the candidate lists [nb, max_fetch], the host form's copy of the block's queries (a
// fix-up of the inner search overwrites qdev), the gathered queries of a re-search, their slot-to-line list, the kernel's
// (kept, entries), and the host form's key table and its staging of the results' keys
struct CollapseBufs {
    DevBuf<double> vals, out_vals, cand_dist;
    DevBuf<int64_t> ids, keys, out_ids, out_keys, cand_rows;
    DevBuf<int32_t> out_pos, count, entries, lines, kept;
    DevBuf<float> q_all, q_sub;
    hipError_t reserve_lists(size_t B, size_t w, size_t keys_len, size_t k_out) {
        hipError_t e = grow_each(B * w, vals, ids);
        if (!e) e = grow_each(keys_len, keys);
        if (!e) e = grow_each(B * k_out, out_vals, out_ids, out_keys, out_pos);
        if (!e) e = grow_each(B, count, entries);
        return e;
    }
    hipError_t reserve_search(size_t nb, size_t max_fetch, size_t k, size_t dim, size_t host_keys_len, bool host) {
        hipError_t e = grow_each(nb * max_fetch, cand_dist, cand_rows);
        if (!e) e = grow_each(nb * dim, q_sub);
        if (!e) e = grow_each(nb, lines, kept, entries);
        if (!e && host) e = grow_each(nb * dim, q_all);
        if (!e && host) e = grow_each(host_keys_len, keys);
        if (!e && host) e = grow_each(nb * k, out_keys);
        return e;
    }
    size_t bytes() const {
        return vals.bytes + out_vals.bytes + cand_dist.bytes + ids.bytes + keys.bytes + out_ids.bytes + out_keys.bytes +
               cand_rows.bytes + out_pos.bytes + count.bytes + entries.bytes + lines.bytes + kept.bytes + q_all.bytes +
               q_sub.bytes;
    }
};
// range search (mi355dr_search_range*): one block's result buffers [nb, R slots] with their per-query
// words, the radii, the redo list of `pairs` pairs, the two device counters and the sub-block of the queries the ordinary
// search serves (fb_*: map, gathered queries, lists [nb, m])
struct RangeBufs {
    DevBuf<uint64_t> key, rkey;
    DevBuf<int32_t> row, xfrom;
    DevBuf<unsigned long long> count, stat;
    DevBuf<double> radius, fb_dist;
    DevBuf<int> redo, flag, fb_map;
    DevBuf<int64_t> fb_rows;
    DevBuf<float> fb_q;
    int collect_lds = 0;  // dynamic LDS k_range_collect is registered for (0: not yet)
    hipError_t reserve(size_t nb, size_t R, size_t m, size_t pairs, size_t dim) {
        hipError_t e = grow_each(nb * R, key, row);
        if (!e) e = grow_each(nb, count, rkey, xfrom, radius, flag, fb_map);
        if (!e) e = grow_each(2, stat);
        if (!e) e = grow_each(2 + 2 * pairs, redo);
        if (!e) e = grow_each(nb * dim, fb_q);
        if (!e) e = grow_each(nb * m, fb_dist, fb_rows);
        return e;
    }
};
// search by stored row (mi355dr_search_rows* / mi355dr_search_range_rows*): one block's ids, gathered
// query vectors [nb, dim] and validity words, the inner pass's lists [nb, stride = k + 1] / counts, the range form's (slot, row)
// pairs with their row-with-itself distances and the radii, the skipped-slot counter
struct RowQueryBufs {
    DevBuf<int64_t> ids, pair_row, cand_rows, cand_count;
    DevBuf<float> q, self_dot;
    DevBuf<int> valid;
    DevBuf<int32_t> pair_q;
    DevBuf<double> cand_dist, self_dist, radius;
    DevBuf<unsigned long long> skipped_dev;
    hipError_t reserve(size_t nb, size_t stride, size_t dim, bool range) {
        hipError_t e = grow_each(nb, ids, valid, pair_q, pair_row);
        if (!e) e = grow_each(nb * dim, q);
        if (!e) e = grow_each(nb * stride, cand_dist, cand_rows);
        if (!e) e = grow_each(1, skipped_dev);
        if (!e && range) e = grow_each(nb, cand_count, self_dot, self_dist, radius);
        return e;
    }
};
// search by examples / feedback (mi355dr_combine_rows* / mi355dr_search_examples* / mi355dr_search_feedback*; DESIGN.md
// section 4.8n): one block's listed ids [nb, mp] / [nb, mn], the combined query vectors [nb, dim] and validity words, the inner
// passes' lists [nb, stride], the feedback host form's copy of the block's queries (a fix-up of pass 1 overwrites qdev) and
// the two counters of k_combine_rows (skipped positions, invalid slots)
struct ExampleBufs {
    DevBuf<int64_t> pos, neg, cand_rows;
    DevBuf<float> q, base;
    DevBuf<int> valid;
    DevBuf<double> cand_dist;
    DevBuf<unsigned long long> counters;
    hipError_t reserve(size_t nb, size_t mp, size_t mn, size_t stride, size_t dim, bool own_base) {
        hipError_t e = grow_each(nb * mp, pos);
        if (!e) e = grow_each(nb * mn, neg);
        if (!e) e = grow_each(nb, valid);
        if (!e) e = grow_each(nb * dim, q);
        if (!e) e = grow_each(nb * stride, cand_dist, cand_rows);
        if (!e) e = grow_each(2, counters);
        if (!e && own_base) e = grow_each(nb * dim, base);
        return e;
    }
};
// row-sharded derived searches (mi355dr_search_*_sharded_device / mi355dr_mmr_select_sharded): this
// rank's payload of an all-gather and the gathered payloads of all ranks (packed lists, query rows, host candidate lists: one
// collective at a time, in stream order), the MMR candidate stage and its gathered form, the counter k_rows_gather's own
// "outside this shard" count goes to (not a stat: rows_skipped counts slots NO rank owned)
struct ShardBufs {
    DevBuf<int64_t> send, recv;
    DevBuf<float> stage, stage_all;
    DevBuf<unsigned long long> local_skipped;
};
}  // namespace mi355

struct mi355dr_index {
    int device = 0, dim = 0, dpad = 0, metric = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    mi355dr_index() = default;
    // every member below that holds device memory, pinned memory or an event releases it itself; the stream goes first
    ~mi355dr_index() {
        if (stream) (void)hipStreamDestroy(stream);
    }

    // corpus (single-vector)
    int64_t n = 0, cap_rows = 0;
    mi355::DevBuf<float> rows;
    mi355::DevBuf<uint16_t> shadow;
    mi355::DevBuf<float> nrm2;
    mi355::DevBuf<int32_t> irr_rows;
    mi355::DevBuf<int> irr_count;
    int irr_n = 0;
    mi355::DevBuf<unsigned> n2max_dev;  // largest regular |c|^2 (float bits)
    float cmax = 0.0f;              // its square root, inflated: inner-product thresholds
    mi355::DevBuf<unsigned> bf16_res2_dev;  // largest squared residual norm |c_hat - bf16(c_hat)|^2 over the rows (float bits)
    float bf16_ec = 0.00390625f;        // its square root, inflated: the corpus half of the bf16 screen bound
    // int8 screen: second shadow, one step for the whole corpus; rows it cannot hold are flagged and listed
    int dpad8 = 0;
    mi355::DevBuf<int8_t> shadow8;     // [cap_rows, dpad8]
    mi355::DevBuf<uint8_t> flag8;      // [cap_rows]
    mi355::DevBuf<mi355::I8Group> grp8;  // [cap_rows / 32] int8 step + residual norm per group of 32 rows
    mi355::DevBuf<int32_t> irr8_rows;  // [kIrrCap] irregular + loose rows
    mi355::DevBuf<int> irr8_count;
    int irr8_n = 0;
    // removed rows (mi355dr_remove_rows): slots that stay, marked in nrm2 (dev_common.h kDeadNrm2) and in neither list
    mi355::DevBuf<int> dead_count;
    int64_t dead_n = 0;

    // per-search state (sized for one block of kQBlockMax queries)
    bool qstate_ready = false;
    mi355::QueryState st{};      // what the kernels take by value: views of st_mem, filled by ensure_qstate
    mi355::DevBuf<void> st_mem[sizeof(mi355::QueryState) / sizeof(void*)];  // one owner per pointer of st, in its order
    mi355::DevBuf<float> qdev;       // [kQBlockMax, dim]
    mi355::DevBuf<int32_t> cand_row; // [kQBlockMax, cap]
    mi355::DevBuf<float> cand_val;
    mi355::DevBuf<int> qlist_dev;    // [2 * kQBlockMax] second half: overflow re-runs of the exact scan
    int* status_or_dev = nullptr;    // = st.status + kQBlockMax
    mi355::HostBuf<int> status_host;  // pinned [kQBlockMax + 1]
    // THE result staging of every host form (search, subset, MMR, range, by-row; mi355dr.hip block_outputs / block_return): one
    // block's [nb <= kQBlockMax, width <= kKMax] distances and rows and its [nb] counts.  One set is enough because only an
    // OUTERMOST entry point stages, and it holds `mu` from before its first block until its last copy has landed.  Inner passes
    // never stage: range_block under the by-row search, search_block under range_block's fallback, under MMR and under the
    // grouped search, and complete_block's fix-up levels each write to the *_cand_*, rng.fb_* or retry[] buffer they were given.
    mi355::DevBuf<double> out_dist_dev;    // [kQBlockMax, kKMax]
    mi355::DevBuf<int64_t> out_rows_dev;   // [kQBlockMax, kKMax]
    mi355::DevBuf<int64_t> out_count_dev;  // [kQBlockMax]
    mi355::DevBuf<unsigned long long> stat_dev;  // [2*kQBlockMax]: per query (candidates, re-scored)
    mi355::DevBuf<int> prune_skip;   // [2 + 2*kQBlockMax] hand-over lists of k_prune (PruneArgs::skip_list)
    mi355::DevBuf<int32_t> subset_ids;  // the listed rows of the mi355dr_search_subset call in progress: local, ascending, unique
    mi355::MmrBufs mmr;      // per-family scratch of the derived searches (above): grown by each family's reserve()
    mi355::GroupBufs grp;
    mi355::FuseBufs fuse;
    mi355::CollapseBufs clp;
    mi355::RangeBufs rng;
    mi355::RowQueryBufs rowq;
    mi355::ExampleBufs exq;
    mi355::ShardBufs shd;
    // a view (mi355dr_view_create; DESIGN.md "Views"): a read-only index built from listed rows / documents of a parent.  The
    // maps are null on every other index: the result-writing kernels then add row_offset instead
    bool is_view = false;
    mi355::DevBuf<int64_t> view_row_map;  // [n] the parent's global id of view row j (k_finalize)
    mi355::DevBuf<int64_t> view_doc_map;  // [n_docs] the same for the documents (k_ms_final, k_ms_write_out)
    int64_t view_rows = 0, view_docs = 0;  // what the build kept (stats "view_rows" / "view_docs")
    int prune_parity = 0;

    // options
    int path = 0;  // MI355DR_PATH_AUTO
    int screen_dtype = 0;  // MI355DR_SCREEN_AUTO
    int i8_backoff = 0, i8_probation = 0;  // demotion is not for ever: after i8_probation more blocks at such a k AUTO tries int8 again;
                                           // the wait doubles (16 ... 4096 blocks) every time that try overflows again
    // speculative passes (Pass::speculative): a block of which more than 1 % missed or overflowed suspends them for spec_probation
    // first attempts -- 16 at first, doubling up to 4096 with every block that fails again; option "speculate" re-arms
    int speculate = 1;
    int64_t spec_min_rows = (int64_t)1 << 20;  // 64 samples: smaller corpora keep the ladder
    int spec_shift_milli = 0;  // lab: added to zq in thousandths of the sample's standard deviation (makes the model wrong on purpose)
    int spec_backoff = 0, spec_probation = 0;
    mi355::DevBuf<float> spec_moments;  // [kQBlockMax, kSpecSlabsMax, 2] the starter's per-slab sums (screen_hits.h)
    int i8_demoted_k = INT_MAX;  // AUTO saw the int8 bound overflow on this corpus' score distribution at this k: bf16 from there up
    double i8_min_budget = 0.25;  // AUTO keeps the int8 screen while growth_budget(k, int8) stays above this (k <= 133)
    mi355::RetryBufs retry[3];  // one set per level: the nested call owns the next
    // blocks in flight: sequence numbers [seq_done, seq_next) live in pend[seq % kPendingRing]; sub_pend[level]: the
    // synchronous blocks of level `level` (search_block)
    mi355::Pending pend[mi355::kPendingRing];
    mi355::Pending sub_pend[4];
    int64_t seq_next = 0, seq_done = 0;
    // k of the most recent top-k pass (enqueue_block, subset_block).  No pass reads it: between searches, stat
    // "screen_dtype_active" and the debug entry points decide as a first attempt at this k would (idle_i8)
    int last_pass_k = 10;
    int maxsim_coop = -1;       // exact MaxSim on candidate lists: one workgroup per candidate (1), one wave (0), by document length (-1)
    int maxsim_persistent = 0;  // MaxSim screen (dims <= 128): persistent workgroups walking the docs in rounds.  A/B on one box
                                // (interleaved A/B through this option, 1 M text docs / 100 k pages): text +-0, pages 4 % SLOWER -- off
    // MaxSim screen, 9..16 column blocks: the workgroup-cooperative form (k_maxsim_wg.h).  -1 (default): yes, per-document epilogue
    // by document length; 1: parked epilogue; 2: immediate epilogue; 0: one wave per document with the query fragments in LDS
    // (k_maxsim16_d128<NCB, 8>) -- option "maxsim_wg", A/B and tests
    int maxsim_wg = -1;
    int maxsim_tighten = 1;  // MaxSim fast path: narrow the candidate band with the exact distances of the screen's top-k (0: band 2E)
    int maxsim_aligned = 1;  // k_maxsim16_wg: when every query of a pass is one column block, a wave sums its own two queries (0: A/B)
    int maxsim_wg_min = 8;   // fewest column blocks of a pass that take the workgroup form (8: short documents only; 9)
    int maxsim_wg_pipe = 1;  // k_maxsim16_wg, 4 blocks per stage: fold block j under the MFMAs of block j + 1 (0: the unpipelined form, A/B)
    // MaxSim screen, aligned passes that take the workgroup form: the granule-packed bf16 copy (k_maxsim_wg8.h; a second shadow,
    // built on first use).  -1 (default): when it removes at least 5 % of the padded copy's blocks and its memory is there; 1: always; 0: never
    int maxsim_pack8 = -1;
    int maxsim_wg_bps = 4;  // k_maxsim16_wg: 32-token blocks per ring stage (2: 7 stages of 16 KiB, 4: 4 stages of 32 KiB); option, A/B
    int maxsim_pass_groups = 4;  // groups of <= 4 queries one pass of the MaxSim screen serves (1 .. 4; option "maxsim_pass_groups", A/B and tests)
    int maxsim_screen = 1; // 1: bf16 MFMA screen + exact re-score of the candidates, 0: exact kernel over every doc
    // mi355dr_search_maxsim_subset: the list form of the screen (1), the exact list path (0), or (-1, default) the screen from
    // maxsim_subset_screen_min listed documents with vectors on (512: the screen beat the exact list path at every measured list
    // size, the smallest was 1 000 documents -- DESIGN.md 4.8d, profiles/maxsim_subset_time_1m.txt)
    int maxsim_subset_screen = -1;
    int64_t maxsim_subset_screen_min = 512;
    int64_t row_offset = 0;
    int round_a = 0;      // k_prune: rows re-scored before the cut is known (0 = max(32, 2k)); tuning option "round_a"
    int screen_rq = 1;      // query blocks above 128, int8 shadow of <= 768 B per row: k_screen_rq (query operand in registers) instead of k_screen256c (option "screen_rq")
    int screen_stream = 1;  // query blocks of at most 64: k_screen_stream instead of k_screen (option "screen_stream", A/B and tests)
    int prefilter16 = 0;  // int8 screen: bf16 second screen of the surviving candidates inside k_prune (option "prefilter16";
                          // off: measured +1.4 % at 1.25 M rows, +0.2 % at 10 M -- the prune is bound by batch latency, not bytes)
    int profile = 0;
    int starter = 1;          // pass schedule: sampled threshold estimator instead of the smallest chunks (option "starter", A/B and tests)
    // 1 (default): the general-form prune is launched behind every one-wave prune (4 us when it finds nothing to do); 0: the
    // one-wave form alone, what it cannot hold (> 1024 entries) is flagged and re-screened -- measured at N = 10 M, k = 10: a few
    // queries per block exceed the 1024 entries in some chunk, and their re-screen pass costs 0.25 ms per block (0.85 ms with
    // carried survivors in the lists), against 20 us of companion launches
    int prune_companion = 1;
    int scan_dma = 1;         // exact scan: the LDS-DMA form (k_scan32) when dim % 32 == 0 (option "scan_dma", A/B and tests)
    int defer_round_b = 1;    // k_prune before the pass's last one carries the survivors of its cut over instead of re-scoring them
    int chunk0_set = 0;       // the first chunk's size was set by the caller: emit-all ladder, no starter
    int64_t chunk0_rows = 1024;
    int64_t chunk_growth = 3;
    int chunk_growth_set = 0;  // the option was set by the caller: no small-block override
    int64_t small_chunk_rows = 16384;  // chunks up to this many rows go through the 128x128 kernel (dense hits: per-lane appends)
    int cap = mi355::kCandCap;
    int cap_set = 0;          // option "cand_cap" was set by the caller: every pass uses it (else wide-prune passes use kCandCapWide)
    // 33 <= k <= 128: the two-wave prune (k_prune_wide.h: 4096 entries, round A of up to 128 rows, no companion launch), the
    // starter over a 64 k-row sample and chunk ratios up to 4 (option "prune_wide"; 0 = the round-5 schedule, A/B and tests)
    int prune_wide = 1;
    // k_screen_rq: the waves of a workgroup flush their hit-lane queues at the same tiles, every `period` tiles with
    // period = the largest power of two below screen_flush_lanes / (expected hit lanes per wave and tile) (1 ... 64);
    // option "screen_flush_sync" (0 = every wave on its own, round 5), "screen_flush_lanes" (tuning)
    int screen_flush_sync = 1, screen_flush_lanes = 48, screen_flush_alone = 40;
    int wide_inflation_x10 = 100;  // growth budget of the two-wave prune's passes: inflation of the int8 bound it plans for, x 10 (tuning)
    // pass schedule: ratio of chunk i = (geometric mean) x taper^((n-1)/2 - i) -- early chunks (cheap hits, loose bound) larger,
    // late chunks (expensive hits) smaller; 100 = uniform ratios (option "chunk_taper_x100")
    int chunk_taper_x100 = 0;   // 0 = auto: 120 for passes of the two-wave prune (measured -1 % at k = 100), 100 otherwise (k = 10: no gain)
    int64_t compact_slice_rows = 65536;  // mi355dr_compact: destination rows per slice of its staging buffer (option "compact_slice_rows", 32 ... 2^22)
    int64_t view_slice_rows = 65536;  // mi355dr_view_create on THIS index: rows per slice of its staging buffer (option "view_slice_rows", 32 ... 2^22)
    // mi355dr_search_range*: rows per screen launch / exact-scan span (option "range_chunk_rows": 10 M rows are 5 launches, each
    // long enough to run at the long screens' rate) and slots of a query's result buffer (option "range_slots", 16 ... 4096 =
    // what the finishing sort holds; never below the call's max_results)
    int64_t range_chunk_rows = (int64_t)1 << 21;
    int range_slots = mi355::kSortMax;
    // mi355dr_search_mmr_sharded_device / mi355dr_mmr_select_sharded: most bytes of the GATHERED candidate-vector stage (option
    // "shard_stage_bytes"; a block of queries is selected in sub-blocks sized to it, never below one query)
    int64_t shard_stage_bytes = (int64_t)256 << 20;
    int64_t starter_rows_wide = 65536;  // the starter's sample at 33 <= k <= 128 (option "starter_rows_wide", tuning: 4096 ... 262144)

    // stats
    int64_t s_screen_launches = 0, s_screen_ns = 0, s_screen_rows = 0, s_fallback_queries = 0, s_chunks = 0,
            s_passes = 0, s_starters = 0;
    int64_t s_big_launches = 0, s_big_ns = 0, s_big_rows = 0;  // the k_screen256c / k_screen_rq share of the three above
    int screen_rq_split_tests = 1;  // k_screen_rq: a block test's maxima ride the MFMAs of the other row half (0: in one piece; d = 768 only, A/B; option "screen_rq_split_tests")
    int64_t debug_park = 0;     // diagnostic (option "debug_park_thresholds" = rows): k_screen_rq launches of at least that many rows run with every threshold at +inf -- what such a launch costs without hits; results are wrong while it is set
    mi355::DevBuf<float> park_thr;  // [kQBlockMax] +inf
    int screen_drift = 3;   // k_screen_rq: tiles a workgroup may run ahead of its slowest sibling (0 = no limiter; option "screen_drift")
    mi355::DevBuf<int> rq_progress;  // [kRqProgressWords] the limiter's progress words
    int rq_epoch = 0;            // launch stamp of the last k_screen_rq launch (1 ... 4095)
    int64_t s_rq_launches = 0;  // of them: k_screen_rq launches (stat "screen_rq_launches")
    // speculative passes, and their queries that missed the verification / overflowed a list (both also count as retry_queries)
    int64_t s_spec_passes = 0, s_spec_miss_queries = 0, s_spec_overflow_queries = 0;
    int64_t s_retry_queries = 0;  // queries whose candidate list overflowed and that were re-screened with the bf16 bound
    int64_t s_ms_screened = 0, s_ms_candidates = 0, s_ms_fallbacks = 0;  // MaxSim: queries screened, docs re-scored, full re-runs
    // option "profile": HIP-event time of the MaxSim screen launches (k_maxsim16*) and of the exact launches on candidate lists
    int64_t s_ms_screen_ns = 0, s_ms_screen_launches = 0, s_ms_exact_ns = 0, s_ms_exact_launches = 0, s_ms_pack_ns = 0;
    int64_t s_ms_packed_launches = 0;  // screen launches that took the granule-packed copy (k_maxsim_wg8.h)
    int64_t s_ms_packed_blocks = 0;    // ... and the 32-token blocks of that copy (0: none built)
    int64_t s_ms_packed_built = 0;     // blocks k_ms_pack8 has written since the index was created (a store that grows is packed from its new granules on)
    int64_t s_ms_set_docs = 0;         // documents rewritten by mi355dr_set_multivec ...
    int64_t s_ms_moved_blocks = 0;     // ... and the blocks its relayouts copied (k_ms_relayout; the in-place path moves none)
    int64_t s_compactions = 0;         // mi355dr_compact calls that moved rows ...
    int64_t s_compact_moved_rows = 0;  // ... and the rows they copied (k_compact_gather)
    int64_t s_subset_searches = 0;       // mi355dr_search_subset / _device calls ...
    int64_t s_subset_rows_scored = 0;    // ... the (query, listed row) pairs their gathered scans scored ...
    int64_t s_subset_rerun_queries = 0;  // ... and the queries whose list overflowed in a chunk that was then re-run in list-sized pieces
    // mi355dr_search_maxsim_subset: calls, listed documents with vectors, queries served by the list screen / by the exact list
    // path (fallbacks included), queries whose candidate list overflowed
    int64_t s_mss_searches = 0, s_mss_docs = 0, s_mss_screened = 0, s_mss_exact = 0, s_mss_fallbacks = 0;
    // mi355dr_maxsim_align: calls, (query, document) pairs scored; mi355dr_maxsim_map: calls, floats written
    int64_t s_msa_calls = 0, s_msa_pairs = 0, s_msm_calls = 0, s_msm_values = 0;
    // mi355dr_search_mmr* / mi355dr_mmr_select: calls, queries, (picked row, unselected candidate) dots of k_mmr_select
    int64_t s_mmr_searches = 0, s_mmr_queries = 0, s_mmr_pairs = 0;
    // mi355dr_search_groups*: calls, sub-queries; groups merged by them and by mi355dr_merge_groups_device
    int64_t s_group_searches = 0, s_group_subqueries = 0, s_groups_merged = 0;
    // mi355dr_fuse_lists*: calls, queries
    int64_t s_fuse_calls = 0, s_fuse_queries = 0;
    // mi355dr_collapse_lists* / mi355dr_search_collapsed*: list calls; search calls, their queries, (query, round) re-searches,
    // queries returned truncated
    int64_t s_collapse_calls = 0, s_collapse_searches = 0, s_collapse_queries = 0, s_collapse_researched = 0, s_collapse_truncated = 0;
    // mi355dr_search_range*: calls, queries, rows in range (the counts, summed); screen path: candidates taken from the screens
    // and of them re-scored; (query, chunk) pairs run again on the exact path; queries whose list the ordinary search served
    int64_t s_range_searches = 0, s_range_queries = 0, s_range_in_range = 0, s_range_candidates = 0, s_range_rescored = 0,
            s_range_redo_chunks = 0, s_range_fallback_queries = 0;
    // mi355dr_search_rows* / mi355dr_search_range_rows*: calls, slots, slots whose id was outside the shard or a removed row
    int64_t s_rows_searches = 0, s_rows_queries = 0, s_rows_skipped = 0;
    // mi355dr_combine_rows* / mi355dr_search_examples* / mi355dr_search_feedback*: calls of the three, their slots, example
    // positions skipped, slots answered NaN / -1; of the calls, the feedback ones
    int64_t s_examples_searches = 0, s_examples_queries = 0, s_examples_skipped = 0, s_examples_skipped_slots = 0,
            s_feedback_searches = 0;
    // the row-sharded derived searches: calls per family, bytes this rank received through their all-gathers
    int64_t s_shard_range_searches = 0, s_shard_rows_searches = 0, s_shard_mmr_searches = 0, s_shard_gather_bytes = 0;
    // the row-sharded sparse forms: calls of the four searches, calls of the two score forms (their gathers add to the above)
    int64_t s_shard_sparse_searches = 0, s_shard_sparse_scores = 0;
    // mi355dr_search_sparse* / mi355dr_search_bm25*: calls, queries, postings accumulated by k_sparse_score, (query, launch)
    // candidate lists that overflowed and were run again in pieces
    int64_t s_sparse_searches = 0, s_sparse_queries = 0, s_sparse_postings_scored = 0, s_sparse_overflows = 0;
    int sparse_tile_docs = 2048;  // documents per LDS tile of k_sparse_score (option "sparse_tile_docs": a power of two, 256 .. 8192;
                                  // 2048 was the fastest of 1024 .. 8192 at 3, 8 and 24 terms per query: DESIGN.md section 4.8j)
    int sparse_cand_cap = 2048;   // slots of a query's sparse candidate list (option "sparse_cand_cap", 16 .. 2048)
    // mi355dr_search_*_subset: a list of at most this many local documents (and at most sparse_cand_cap) is looked up pair by
    // pair (k_sparse_pairs), a longer one runs the filtered tile pass (option "sparse_subset_pairs_max", 0 .. sparse_cand_cap;
    // 0: always the tile pass).  2048: the largest list measured and the largest the candidate list admits -- at 1 M documents
    // and 8-term queries the pair pass took 0.88 / 0.93 / 1.15 / 1.40 ms per block at m = 64 / 256 / 1024 / 2048 where the
    // tile pass took 1.57 / 3.06 / 6.56 / 8.51 ("Within a listed subset")
    int64_t sparse_subset_pairs_max = 2048;
    // the *_subset forms: calls of the four searches, calls of the two score forms, (query, document) pairs given to
    // k_sparse_pairs, tiles launched by the filtered k_sparse_score (grid.x, summed over launches)
    int64_t s_sparse_subset_searches = 0, s_sparse_subset_scores = 0, s_sparse_subset_pairs = 0, s_sparse_subset_tiles = 0;
    // the first search after add / set / remove of sparse documents rebuilds the overlay alone while the moved documents'
    // postings are at most this many percent of the base layout's, else the whole layout (option "sparse_overlay_max_pct",
    // 0 .. 100; 0: always the whole layout).  25: the largest size measured, where the overlay build still cost a quarter of
    // the full build's time and the steady block time was below an untouched store's; above it
    // nothing was measured
    int sparse_overlay_max_pct = 25;
    // layout builds of the sparse store by kind, and documents given to mi355dr_set_sparse / mi355dr_remove_sparse
    int64_t s_sparse_full_builds = 0, s_sparse_overlay_builds = 0, s_sparse_sets = 0;
    int64_t s_ms_screen_cols = 0;  // query-vector columns (whole blocks of 32) the screen launches multiplied every token by
    mi355::Event ms_ev[4];
    // which MaxSim screen launch ran last, written on the host next to the launch (mi355dr_debug_maxsim_pass reports it).
    // family: MI355DR_MS_FORM_* (include/mi355dr.h); bps / pipe / now: the workgroup forms' blocks per stage, software pipeline,
    // epilogue at once
    struct MsScreenForm {
        int family = 0, ncb = 0, waves = 0, bps = 0, pipe = 0, now = 0, grid = 0, reserved = 0;
    } last_screen_form;
    mi355::EventPairs ev_pool, ev_pending;
    mi355::Event t0, t1;

    // RCCL communicator of a row-sharded index (mi355dr_comm.hip)
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    mi355dr_allgather_fn comm_custom = nullptr;  // the host's own all-gather instead of RCCL (mi355dr_comm_init_custom)
    void* comm_custom_user = nullptr;
    // two of each: block i's all-gather + merge run on comm_stream under block i + 1's search (mi355dr_search_sharded_device)
    int64_t* comm_packed[2] = {nullptr, nullptr};      // [2, kQBlockMax, k] this rank's packed block
    int64_t* comm_packed_all[2] = {nullptr, nullptr};  // [world, 2, kQBlockMax, k]
    hipStream_t comm_stream = nullptr;
    hipEvent_t comm_done[2] = {nullptr, nullptr};      // gather + merge of the block that used buffer b have been enqueued / finished
    bool comm_done_armed[2] = {false, false};
    size_t comm_cap = 0;

    // multi-vector store (MaxSim), owned by mi355dr_maxsim.hip
    mi355::MultiVecStore* mv = nullptr;
    // sparse store (tokenised documents, BM25), owned by mi355dr_sparse.hip
    mi355::SparseStore* sp = nullptr;
};


namespace mi355 {

int fail(mi355dr_index* idx, int code, const std::string& msg);  // mi355dr.hip
// A view is read-only and speaks the parent's ids: the entry points that write, and those that take global ids or a
// communicator (ask_parent), start with `if (idx->is_view) return view_refuses(...)` under the handle's mutex
inline int view_refuses(mi355dr_index* idx, const char* what, bool ask_parent = false) {
    return fail(idx, MI355DR_E_INVALID, std::string(what) + (ask_parent ? ": not on a view (it is a read-only snapshot under the parent's ids) -- ask the parent index"
                                                                        : ": a view is read-only"));
}
void multivec_destroy(mi355dr_index* idx);                       // mi355dr_maxsim.hip
// room for n_blocks 32-token blocks and n_docs documents, the store created if there is none (mi355dr_view_create reserves once)
int multivec_reserve(mi355dr_index* idx, int64_t n_blocks, int64_t n_docs);  // mi355dr_maxsim.hip
int64_t multivec_bytes(const mi355dr_index* idx);                // mi355dr_maxsim.hip: stat "hbm_bytes_resident"
void sparse_destroy(mi355dr_index* idx);                         // mi355dr_sparse.hip
int64_t sparse_bytes(const mi355dr_index* idx);                  // mi355dr_sparse.hip: stat "hbm_bytes_resident"
enum { kSparseStatDocs, kSparseStatTotalLen, kSparseStatPostings, kSparseStatVocab, kSparseStatOverlayPostings, kSparseStatDeadPostings };
int64_t sparse_stat(const mi355dr_index* idx, int which);        // mi355dr_sparse.hip: the store's own figures (0 without a store)
int drain_searches(mi355dr_index* idx);                          // mi355dr.hip: blocks in flight finished (under the handle's mutex)
// mi355dr.hip: mi355dr_merge_topk_packed_device for a caller that holds the handle's mutex -- the gathered packed blocks
// [world][2][B][k] merged into [B, k] on `stream`.  merge_topk_reserve: the one allocation the merge may make (the per-search
// state), for a caller that wants it made before its first collective
int merge_topk_reserve(mi355dr_index* idx);
int merge_topk_packed(mi355dr_index* idx, const int64_t* packed_all_dev, int world, int B, int k, double* out_dist_dev,
                      int64_t* out_rows_dev, hipStream_t stream);
void comm_destroy(mi355dr_index* idx);                           // mi355dr_comm.hip
// one all-gather over the index's communicator (RCCL, or the host's transport): bytes_per_rank (a multiple of 8) from every
// rank's send_dev into recv_dev, rank-major; ordered on `stream` (a host transport may instead be complete on return)
int comm_all_gather(mi355dr_index* idx, const void* send_dev, void* recv_dev, size_t bytes_per_rank, hipStream_t stream);  // mi355dr_comm.hip
// read-only view of the multi-vector store for kernels outside mi355dr_maxsim.hip (GQR refinement)
struct MultiVecView {
    const float* tok;             // [blocks*32, dpad] device
    const int64_t* blk_off;       // [n_docs+1] device
    const int64_t* blk_off_host;  // same, host
    const int32_t* tok_cnt_host;  // [n_docs] token vectors of each doc, host
    int dpad;
    int64_t n_docs;
};
bool multivec_view(const mi355dr_index* idx, MultiVecView* out);  // false: no store yet

// Column order inside every group of 8 dims, for BOTH stored token rows and the staged query rows:
// position j holds original column kPerm[j] = {0,4,2,6,1,5,3,7}[j].  A lane of the lower half (k-slot 0 of the
// 32x32x2 MFMA) reads positions 0..3 = columns (0,4,2,6), a lane of the upper half positions 4..7 = (1,5,3,7),
// so issuing the MFMAs on components x, z, y, w walks k = (0|1), (2|3), (4|5), (6|7): ascending, no lane swaps.
__host__ __device__ inline int ms_perm(int j) {
    constexpr int P[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    return (j & ~7) | P[j & 7];
}

// one query vector (d values) -> its row of a query image: the store's column order, zero-padded to dpad
template <class T>
inline void multivec_pack_query_row(const T* src, int d, int dpad, T* dst) {
    for (int c = 0; c < dpad; ++c) {
        const int oc = ms_perm(c);
        dst[c] = oc < d ? src[oc] : T(0);
    }
}

#define HIPCHECK(idx, expr)                                                                              \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            char buf__[512];                                                                             \
            snprintf(buf__, sizeof(buf__), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                     __LINE__);                                                                          \
            return mi355::fail(idx, e__ == hipErrorOutOfMemory ? MI355DR_E_NOMEM : MI355DR_E_HIP, buf__); \
        }                                                                                                \
    } while (0)

#define CHECK(expr)                          \
    do {                                     \
        int rc__ = (expr);                   \
        if (rc__ != MI355DR_OK) return rc__; \
    } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

}  // namespace mi355
